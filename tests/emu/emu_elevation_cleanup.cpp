// TEST INFRASTRUCTURE -- CPU shim of the elevation map's visibility clean-up (isaacgymloco_amd/csrc/ls_elevation_cleanup.h): the same
// per-lane functions the HIP kernel lsim_k_elevation_map_cleanup calls, over the same block -> env map, the lanes looped, each
// __syncthreads() a loop boundary and the two LDS arrays plain arrays.  The entry point carries the signature of include/lsim.h (the stream
// is ignored).  emu_elevation_cleanup_point is a hook for the test that pins this launch's point routine to the map's own.
#define LS_EMU 1
#include "../../isaacgymloco_amd/csrc/ls_elevation_cleanup.h"
#include <string.h>

extern "C" int emu_elevation_map_cleanup(const lsim_elevation_map_cleanup_t* ecp, void* /*stream*/) {
    const int rv = ls_ec_validate(ecp);
    if (rv != LSIM_OK) return rv;
    const lsim_elevation_map_cleanup_t& ec = *ecp;
    const lsim_elevation_map_t& em = ec.em;
    const uint32_t tick_mod = ls_em_tick_mod(em);
    const float rinv = ls_em_rinv(em);
    const int slots = ls_em_env_slots(em);
    static uint32_t lds[2 * 64 * 64];
    const int G2 = em.size * em.size;
    float* thr = (float*)lds;
    int32_t* cnt = (int32_t*)(lds + G2);
    for (int slot = 0; slot < slots; ++slot) {
        const int env = slot * em.env_stride;
        bool fill;
        const bool due = ls_sensor_due(em.flags, em.episode_length, em.period, em.stagger, env, tick_mod, fill);
        memset(lds, 0xA5, sizeof lds);           // LDS is not initialised
        if (fill) {
            ec.cleared[env] = 0;
            continue;
        }
        if (!due) continue;
        const LsEmPose s = ls_em_pose(em, env, rinv);
        if (!s.ok) continue;
        for (int lane = 0; lane < LS_EM_BLOCK; ++lane) ls_ec_stage(ec, s, env, lane, thr, cnt);
        for (int lane = 0; lane < LS_EM_BLOCK; ++lane) ls_ec_rays(ec, s, env, lane, rinv, thr, cnt);
        for (int lane = 0; lane < LS_EM_BLOCK; ++lane) {
            const int n = ls_ec_sweep(ec, env, lane, cnt);
            if (n > 0) ls_ec_add(ec.cleared + env, n);
        }
    }
    return LSIM_OK;
}

// ray r of env: xyz = this launch's point at the ray's own range t (ls_ec_point), and ls_em_point's verdict on the same ray -- kept, and when
// kept its slot and height.  Returns 0 when the ray passes the range and label tests (xyz is written then), 1 when not, -1 on bad arguments.
extern "C" int emu_elevation_cleanup_point(const lsim_elevation_map_t* emp, int env, int r, float* xyz, int* kept, int* slot, float* z) {
    if (ls_em_validate(emp) != LSIM_OK || env < 0 || env >= emp->num_envs || r < 0 || r >= emp->num_rays) return -1;
    const lsim_elevation_map_t& em = *emp;
    const float rinv = ls_em_rinv(em);
    const LsEmPose s = ls_em_pose(em, env, rinv);
    const float* row = em.depth + (size_t)env * (size_t)em.depth_stride;
    const uint8_t* lab = em.labels ? em.labels + (size_t)env * (size_t)em.label_stride : (const uint8_t*)0;
    *kept = ls_em_point(em, s, row, lab, r, rinv, *slot, *z) ? 1 : 0;
    const float d = em.a * row[r] + em.b;
    const float t = em.inv_scale ? d * em.inv_scale[r] : d;
    if (!ls_rc_finite(d) || !(em.t_lo < t) || !(t < em.t_hi)) return 1;
    if (lab && lab[r] != (uint8_t)1) return 1;
    const LsRcV3 P = ls_ec_point(em, s, r, t);
    xyz[0] = P.x; xyz[1] = P.y; xyz[2] = P.z;
    return 0;
}
