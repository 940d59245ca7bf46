// TEST INFRASTRUCTURE -- CPU shim of the range-sensor launch (isaacgymloco_amd/csrc/ls_raycast.h): the same per-ray function the HIP kernel
// lsim_k_raycast calls, over the same (block, lane) -> (env, ray) map, with the lanes looped.  Compile with -DLS_RAYCAST_COUNTERS to have the
// cells-walked / triangles-tested counters in state[2], state[3].  The entry points carry the signatures of include/lsim.h (the stream is ignored).
#define LS_EMU 1
#include "../../isaacgymloco_amd/csrc/ls_raycast.h"

extern "C" int emu_raycast_sizes(size_t* state_bytes) {
    if (!state_bytes) return LSIM_E_INVALID;
    *state_bytes = LSIM_RAYCAST_STATE_WORDS * sizeof(int64_t);
    return LSIM_OK;
}

extern "C" int emu_raycast(const lsim_raycast_t* rcp, void* /*stream*/) {
    const int rv = ls_rc_validate(rcp);
    if (rv != LSIM_OK) return rv;
    const lsim_raycast_t& rc = *rcp;
    const int bpe = ls_rc_blocks_per_env(rc);
    const long long blocks = (long long)bpe * ls_rc_env_slots(rc);
    for (long long b = 0; b < blocks; ++b) {
        const int slot = (int)(b / bpe), chunk = (int)(b - (long long)slot * bpe);
        const int env = slot * rc.env_stride;
        for (int lane = 0; lane < LS_RC_BLOCK; ++lane) {
            const int r = chunk * LS_RC_BLOCK + lane;
            if (r >= rc.num_rays || env >= rc.num_envs) continue;
            ls_rc_ray(rc, env, r);
        }
    }
    return LSIM_OK;
}
