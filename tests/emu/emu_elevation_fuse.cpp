// TEST INFRASTRUCTURE -- CPU shim of the fused elevation-map launch and of the map rows with a confidence
// (isaacgymloco_amd/csrc/ls_elevation_fuse.h): the same per-lane functions the HIP kernels lsim_k_elevation_map_fused and
// lsim_k_map_rows_fused call, over the same block -> env map, the lanes looped, each __syncthreads() a loop boundary and the three LDS arrays
// plain arrays.  The entry points carry the signatures of include/lsim.h (the stream is ignored).
#define LS_EMU 1
#include "../../isaacgymloco_amd/csrc/ls_elevation_fuse.h"
#include <string.h>

extern "C" int emu_elevation_map_fused(const lsim_elevation_map_fused_t* efp, void* /*stream*/) {
    const int rv = ls_ef_validate(efp);
    if (rv != LSIM_OK) return rv;
    const lsim_elevation_map_fused_t& ef = *efp;
    const lsim_elevation_map_t& em = ef.em;
    const uint32_t tick_mod = ls_em_tick_mod(em);
    const float rinv = ls_em_rinv(em);
    const int slots = ls_em_env_slots(em);
    static uint32_t lds[3 * 64 * 64];
    const int G2 = em.size * em.size;
    uint32_t* keys = lds;
    int32_t* sum = (int32_t*)(lds + G2);
    int32_t* cnt = (int32_t*)(lds + 2 * G2);
    for (int slot = 0; slot < slots; ++slot) {
        const int env = slot * em.env_stride;
        bool fill;
        const bool due = ls_sensor_due(em.flags, em.episode_length, em.period, em.stagger, env, tick_mod, fill);
        const LsEmPose s = ls_em_pose(em, env, rinv);
        memset(lds, 0xA5, sizeof lds);           // LDS is not initialised
        if (fill) for (int lane = 0; lane < LS_EM_BLOCK; ++lane) ls_em_clear(em, env, lane);
        if (due && s.ok) {
            for (int lane = 0; lane < LS_EM_BLOCK; ++lane) ls_ef_lds_clear(em, keys, sum, cnt, lane);
            for (int lane = 0; lane < LS_EM_BLOCK; ++lane) ls_ef_pass_max(em, s, env, lane, rinv, keys);
            for (int lane = 0; lane < LS_EM_BLOCK; ++lane) ls_ef_pass_sum(ef, s, env, lane, rinv, keys, sum, cnt);
            for (int lane = 0; lane < LS_EM_BLOCK; ++lane) ls_ef_commit(ef, s, env, lane, keys, sum, cnt);
        }
        if (!s.ok) ls_rc_count((long long*)em.state, 1);
        for (int lane = 0; lane < LS_EM_BLOCK; ++lane) ls_ef_scan(ef, s, env, lane, rinv);
    }
    return LSIM_OK;
}

extern "C" int emu_map_rows_fused(const lsim_map_rows_fused_t* mfp, void* /*stream*/) {
    const int rv = ls_mf_validate(mfp);
    if (rv != LSIM_OK) return rv;
    const long long elements = ls_mr_elements(mfp->mr);
    for (long long i = 0; i < elements; ++i) ls_mf_element(*mfp, i);
    return LSIM_OK;
}
