// TEST INFRASTRUCTURE -- CPU shim of the shaded-frame launch (isaacgymloco_amd/csrc/ls_sensor_shade.h): the same per-block and per-pixel
// functions the HIP kernel lsim_k_sensor_shade calls, over the same (block, lane) -> (env, pixel) map, the lanes looped and each
// __syncthreads() a loop boundary.  The entry points carry the signatures of include/lsim.h (the stream is ignored).
#define LS_EMU 1
#include "../../isaacgymloco_amd/csrc/ls_sensor_shade.h"
#include <string.h>

extern "C" int emu_sensor_shade_sizes(size_t* state_bytes, size_t* palette_bytes) {
    if (!state_bytes || !palette_bytes) return LSIM_E_INVALID;
    *state_bytes = LSIM_RAYCAST_STATE_WORDS * sizeof(int64_t);
    *palette_bytes = LS_SS_LABELS * sizeof(uint32_t);
    return LSIM_OK;
}

extern "C" int emu_sensor_shade(const lsim_sensor_shade_t* ssp, void* /*stream*/) {
    const int rv = ls_ss_validate(ssp);
    if (rv != LSIM_OK) return rv;
    const lsim_sensor_shade_t& ss = *ssp;
    const lsim_raycast_bodies_t& rb = ss.rb;
    const int bpe = ls_rc_blocks_per_env(rb.rc);
    const long long blocks = (long long)bpe * ls_rc_env_slots(rb.rc);
    for (long long b = 0; b < blocks; ++b) {
        const int slot = (int)(b / bpe), chunk = (int)(b - (long long)slot * bpe);
        const int env = slot * rb.rc.env_stride;
        if (env >= rb.rc.num_envs) continue;
        LsRcbShared sh;
        memset(&sh, 0xFF, sizeof sh);            // LDS is not initialised
        for (int lane = 0; lane < LSIM_NUM_LEGS; ++lane) ls_rcb_fk(rb, sh, env, lane);
        for (int lane = 0; lane < LS_RC_BLOCK; ++lane) if (lane < sh.nprims) ls_rcb_prim(rb, sh, env, lane);
        for (int lane = 0; lane < LS_RC_BLOCK; ++lane) {
            const int r = chunk * LS_RC_BLOCK + lane;
            if (r < rb.rc.num_rays) ls_ss_pixel(ss, sh, env, r);
        }
    }
    return LSIM_OK;
}
