// TEST INFRASTRUCTURE -- CPU shim of the body-aware range-sensor launch (isaacgymloco_amd/csrc/ls_raycast_bodies.h): the same per-block and
// per-ray functions the HIP kernel lsim_k_raycast_bodies calls, over the same (block, lane) -> (env, ray) map, the lanes looped and each
// __syncthreads() a loop boundary.  The entry points carry the signatures of include/lsim.h (the stream is ignored); the test-only
// emu_raycast_bodies_poses runs the same loops and also writes the block's 17 body poses (8 floats each: base-relative position, quaternion)
// of every env it renders to `bodies_out`, so that the forward kinematics can be tested on its own.  Compile with -DLS_RAYCAST_COUNTERS for the counters.
#define LS_EMU 1
#include "../../isaacgymloco_amd/csrc/ls_raycast_bodies.h"
#include <string.h>

extern "C" int emu_raycast_bodies_sizes(size_t* state_bytes, size_t* robot_bytes) {
    if (!state_bytes || !robot_bytes) return LSIM_E_INVALID;
    *state_bytes = LSIM_RAYCAST_STATE_WORDS * sizeof(int64_t);
    *robot_bytes = sizeof(lsim_raycast_robot);
    return LSIM_OK;
}

extern "C" int emu_raycast_bodies_poses(const lsim_raycast_bodies_t* rbp, float* bodies_out) {
    const int rv = ls_rcb_validate(rbp);
    if (rv != LSIM_OK) return rv;
    const lsim_raycast_bodies_t& rb = *rbp;
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
        if (bodies_out) memcpy(bodies_out + (size_t)env * LSIM_NUM_BODIES * LS_RCB_BODY_WORDS, sh.body, sizeof sh.body);
        for (int lane = 0; lane < LS_RC_BLOCK; ++lane) {
            const int r = chunk * LS_RC_BLOCK + lane;
            if (r < rb.rc.num_rays) ls_rcb_ray(rb, sh, env, r);
        }
    }
    return LSIM_OK;
}

extern "C" int emu_raycast_bodies(const lsim_raycast_bodies_t* rb, void* /*stream*/) { return emu_raycast_bodies_poses(rb, nullptr); }
