// TEST INFRASTRUCTURE -- CPU shim of the elevation-map launch (isaacgymloco_amd/csrc/ls_elevation_map.h): the same per-lane functions the HIP
// kernel lsim_k_elevation_map calls, over the same block -> env map, the lanes looped, each __syncthreads() a loop boundary and the LDS keys a
// plain array.  The entry point carries the signature of include/lsim.h (the stream is ignored).
#define LS_EMU 1
#include "../../isaacgymloco_amd/csrc/ls_elevation_map.h"
#include <string.h>

extern "C" int emu_elevation_map(const lsim_elevation_map_t* emp, void* /*stream*/) {
    const int rv = ls_em_validate(emp);
    if (rv != LSIM_OK) return rv;
    const lsim_elevation_map_t& em = *emp;
    const uint32_t tick_mod = ls_em_tick_mod(em);
    const float rinv = ls_em_rinv(em);
    const int slots = ls_em_env_slots(em);
    static uint32_t keys[64 * 64];
    for (int slot = 0; slot < slots; ++slot) {
        const int env = slot * em.env_stride;
        bool fill;
        const bool due = ls_sensor_due(em.flags, em.episode_length, em.period, em.stagger, env, tick_mod, fill);
        const LsEmPose s = ls_em_pose(em, env, rinv);
        memset(keys, 0xA5, sizeof keys);         // LDS is not initialised
        if (fill) for (int lane = 0; lane < LS_EM_BLOCK; ++lane) ls_em_clear(em, env, lane);
        if (due && s.ok) {
            for (int lane = 0; lane < LS_EM_BLOCK; ++lane) ls_em_keys_clear(em, keys, lane);
            for (int lane = 0; lane < LS_EM_BLOCK; ++lane) ls_em_insert(em, s, env, lane, rinv, keys);
            for (int lane = 0; lane < LS_EM_BLOCK; ++lane) ls_em_commit(em, s, env, lane, keys);
        }
        if (!s.ok) ls_rc_count((long long*)em.state, 1);
        for (int lane = 0; lane < LS_EM_BLOCK; ++lane) ls_em_scan(em, s, env, lane, rinv);
    }
    return LSIM_OK;
}
