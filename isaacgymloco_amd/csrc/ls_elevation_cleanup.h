// ls_elevation_cleanup.h -- the visibility clean-up of the elevation map (include/lsim.h, lsim_elevation_map_cleanup): a cell the newest
// capture's rays pass over on their way to ground further away, well below the height the map holds for it, is forgotten.  lsim.h states
// every formula; this file is that text in code.
//
// It stands on ls_elevation_map.h and changes nothing of it: the pose, the window's cell of a slot, the cell / slot helpers and the argument
// check are that file's.  The point of a ray is formed HERE by a routine of its own (ls_ec_point): the map launches keep their text byte for
// byte (DESIGN.md 7.20 records what folding it cost), and tests/test_elevation_cleanup.py pins this routine to ls_em_point bit for bit.
// tests/emu/emu_elevation_cleanup.cpp compiles this file with g++ under LS_EMU and runs the same per-lane functions, the lanes looped and the
// two LDS arrays plain arrays.
//
// Shape of the launch (lsim_k_elevation_map_cleanup): lsim_k_elevation_map's -- ONE workgroup of 256 lanes per visited env -- with
// 2 * G * G * 4 bytes of dynamic LDS (2, 8 or 32 KB): a float threshold and an int32 count per slot.
//   0. the pose and ls_sensor_due; a fresh env: lane 0 writes cleared[e] = 0, and the block is done; not due or a bad pose: done;
//   1. stage: the lanes sweep the slots (slot = lane, lane + 256, ...: coalesced), threshold and count 0 into LDS; barrier;
//   2. rays (r = lane, lane + 256, ...: the depth row is read coalesced): the segment from the camera to end_gap short of the ray's end,
//      walked through the grid cell by cell, one ds_add_u32 per window cell it passes below the threshold; barrier;
//   3. sweep: a slot with count >= min_rays gets stamp -1; a lane that forgot n > 0 slots adds n to cleared[e] (one integer atomic).
// Only 32-bit integer atomics, no float atomic: the counts do not depend on the order of the rays.  Every branch around a barrier is on
// values the whole workgroup shares (env, fill, due, the pose).
#pragma once
#include "ls_elevation_map.h"

#define LS_EC_STILL 9.5367431640625e-07f        // 2^-20 cells: an axis along which the segment moves less than this never steps

#if defined(LS_EMU) || !defined(__HIPCC__)
LS_RC_FN void ls_ec_add(int32_t* p, int32_t v) { *p += v; }
#else
LS_RC_FN void ls_ec_add(int32_t* p, int32_t v) { (void)atomicAdd(p, v); }
#endif

// the world point at range t on ray r: ls_em_point's operations in ls_em_point's order
LS_RC_FN LsRcV3 ls_ec_point(const lsim_elevation_map_t& em, const LsEmPose& s, int r, float t) {
    const LsRcV3 v = ls_rc_v3(em.dirs[3 * r] * t, em.dirs[3 * r + 1] * t, em.dirs[3 * r + 2] * t);
    const LsRcV3 m = ls_rc_rot(s.ax, s.ay, s.az, s.aw, v);
    const LsRcV3 b = ls_rc_rot(s.qx, s.qy, s.qz, s.qw, ls_rc_v3(s.mx + m.x, s.my + m.y, s.mz + m.z));
    return ls_rc_v3(s.px + b.x, s.py + b.y, s.pz + b.z);
}

// the camera's position: O = p + R(q) mpos
LS_RC_FN LsRcV3 ls_ec_origin(const LsEmPose& s) {
    const LsRcV3 b = ls_rc_rot(s.qx, s.qy, s.qz, s.qw, ls_rc_v3(s.mx, s.my, s.mz));
    return ls_rc_v3(s.px + b.x, s.py + b.y, s.pz + b.z);
}

// step 1: a threshold per slot (-inf where the slot does not know its window cell) and the counts to 0
LS_RC_FN void ls_ec_stage(const lsim_elevation_map_cleanup_t& ec, const LsEmPose& s, int env, int lane, float* thr, int32_t* cnt) {
    const lsim_elevation_map_t& em = ec.em;
    const int G = em.size, G2 = G * G;
    const size_t base = (size_t)env * (size_t)G2;
    for (int k = lane; k < G2; k += LS_EM_BLOCK) {
        float th = -INFINITY;
        if (em.stamp[base + (size_t)k] >= 0) {
            int ix, iy;
            ls_em_window_cell(s, G, k, ix, iy);
            if (em.cell[base + (size_t)k] == ls_em_pack(ix, iy)) {
                th = em.height[base + (size_t)k] - ec.clear_margin;
                if (ec.var) th = th - ec.clear_sigma * ls_sqrt_exact(ec.var[base + (size_t)k]);
            }
        }
        thr[k] = th;
        cnt[k] = 0;
    }
}

// one axis of the walk: the cell, the side it leaves by, and the parameter u of the next boundary
struct LsEcAxis { int i, b, step; float o, k, u; };
LS_RC_FN LsEcAxis ls_ec_axis(float o, float d) {
    LsEcAxis a;
    a.o = o;
    a.i = (int)floorf(o);
    a.step = 0; a.b = a.i; a.k = 0.0f; a.u = INFINITY;
    if (fabsf(d) >= LS_EC_STILL) {
        a.step = d > 0.0f ? 1 : -1;
        a.b = d > 0.0f ? a.i + 1 : a.i;
        a.k = ls_div_exact(1.0f, d);
        a.u = ((float)a.b - o) * a.k;
    }
    return a;
}
LS_RC_FN void ls_ec_advance(LsEcAxis& a) {
    a.i += a.step;
    a.b += a.step;
    a.u = ((float)a.b - a.o) * a.k;
}

// step 2: this lane's rays, each walked from the camera to end_gap short of its end
LS_RC_FN void ls_ec_rays(const lsim_elevation_map_cleanup_t& ec, const LsEmPose& s, int env, int lane, float rinv, const float* thr, int32_t* cnt) {
    const lsim_elevation_map_t& em = ec.em;
    const int G = em.size, half = G >> 1;
    const float* row = em.depth + (size_t)env * (size_t)em.depth_stride;
    const uint8_t* lab = em.labels ? em.labels + (size_t)env * (size_t)em.label_stride : (const uint8_t*)0;
    const LsRcV3 O = ls_ec_origin(s);
    const float ox = O.x * rinv, oy = O.y * rinv;
    if (!ls_rc_finite(O.x) || !ls_rc_finite(O.y) || !ls_rc_finite(O.z) || !ls_em_in_range(floorf(ox)) || !ls_em_in_range(floorf(oy))) return;
    for (int r = lane; r < em.num_rays; r += LS_EM_BLOCK) {
        const float d = em.a * row[r] + em.b;
        const float t = em.inv_scale ? d * em.inv_scale[r] : d;
        if (!ls_rc_finite(d) || !(em.t_lo < t) || !(t < em.t_hi)) continue;
        if (lab && lab[r] != (uint8_t)1) continue;
        if (!(t > ec.end_gap)) continue;
        const LsRcV3 E = ls_ec_point(em, s, r, t - ec.end_gap);
        if (!ls_rc_finite(E.x) || !ls_rc_finite(E.y) || !ls_rc_finite(E.z)) continue;
        const float ex = E.x * rinv, ey = E.y * rinv;
        if (!ls_em_in_range(floorf(ex)) || !ls_em_in_range(floorf(ey))) continue;
        const float hx = E.x - O.x, hy = E.y - O.y, dz = E.z - O.z;
        const float L = ls_sqrt_exact(hx * hx + hy * hy);
        LsEcAxis X = ls_ec_axis(ox, ex - ox), Y = ls_ec_axis(oy, ey - oy);
        float u_in = 0.0f;
        bool was_inside = false;
        for (int n = 0; n < 2 * G + 2; ++n) {
            const float u_out = fminf(fminf(X.u, Y.u), 1.0f);
            const int dx = X.i - s.cx, dy = Y.i - s.cy;
            const bool inside = dx >= -half && dx < half && dy >= -half && dy < half;
            if (was_inside && !inside) break;       // the window is convex: a segment that has left it does not come back
            was_inside = inside;
            if (u_out > u_in && inside) {
                const int slot = ls_em_slot(X.i, Y.i, G);
                const float hi = fmaxf(O.z + u_in * dz, O.z + u_out * dz);
                const float rho = u_out * L;
                if (hi + ec.clear_slope * rho < thr[slot]) ls_ec_add(cnt + slot, 1);
            }
            if (u_out >= 1.0f) break;
            if (X.u <= Y.u) ls_ec_advance(X); else ls_ec_advance(Y);
            u_in = u_out;
        }
    }
}

// step 3: the slots enough rays passed below are forgotten; returns how many of this lane's were
LS_RC_FN int ls_ec_sweep(const lsim_elevation_map_cleanup_t& ec, int env, int lane, const int32_t* cnt) {
    const lsim_elevation_map_t& em = ec.em;
    const int G2 = em.size * em.size;
    int32_t* st = em.stamp + (size_t)env * (size_t)G2;
    int n = 0;
    for (int k = lane; k < G2; k += LS_EM_BLOCK) {
        if (cnt[k] < ec.min_rays) continue;
        st[k] = -1;
        n += 1;
    }
    return n;
}

// ---- host side: the argument check shared by the library and the CPU shim (no launch happens before it passes)
static inline int ls_ec_validate(const lsim_elevation_map_cleanup_t* ec) {
    if (!ec) return LSIM_E_INVALID;
    const int rv = ls_em_validate(&ec->em);
    if (rv != LSIM_OK) return rv;
    if (!ls_rc_aligned(ec->cleared, 4) || (ec->var && !ls_rc_aligned(ec->var, 4))) return LSIM_E_INVALID;
    const float v[4] = {ec->clear_margin, ec->clear_slope, ec->clear_sigma, ec->end_gap};
    for (int k = 0; k < 4; ++k) if (!ls_rc_host_finite(v[k]) || !(v[k] >= 0.0f)) return LSIM_E_INVALID;
    if (ec->min_rays < 1) return LSIM_E_INVALID;
    return LSIM_OK;
}

#if defined(__HIPCC__) && !defined(LS_EMU)
__global__ __launch_bounds__(LS_EM_BLOCK) void lsim_k_elevation_map_cleanup(const lsim_elevation_map_cleanup_t ec, uint32_t tick_mod, float rinv) {
    extern __shared__ uint32_t ls_ec_lds[];
    const lsim_elevation_map_t& em = ec.em;
    const int G2 = em.size * em.size;
    float* thr = (float*)ls_ec_lds;
    int32_t* cnt = (int32_t*)(ls_ec_lds + G2);
    const int env = (int)blockIdx.x * em.env_stride, lane = (int)threadIdx.x;      // < num_envs: blockIdx.x <= (num_envs - 1) / env_stride
    bool fill;
    const bool due = ls_sensor_due(em.flags, em.episode_length, em.period, em.stagger, env, tick_mod, fill);
    if (fill) {                                 // the whole block: the map's launch of this tick empties the env
        if (lane == 0) ec.cleared[env] = 0;
        return;
    }
    if (!due) return;                           // the whole block again, before LDS and the barriers
    const LsEmPose s = ls_em_pose(em, env, rinv);
    if (!s.ok) return;                          // and again: the pose is the env's
    ls_ec_stage(ec, s, env, lane, thr, cnt);
    __syncthreads();
    ls_ec_rays(ec, s, env, lane, rinv, thr, cnt);
    __syncthreads();
    const int n = ls_ec_sweep(ec, env, lane, cnt);
    if (n > 0) (void)atomicAdd(ec.cleared + env, n);
}

extern "C" int lsim_elevation_map_cleanup(const lsim_elevation_map_cleanup_t* ec, void* stream) {
    const int rv = ls_ec_validate(ec);
    if (rv != LSIM_OK) return rv;
    const size_t lds = (size_t)2 * (size_t)ec->em.size * (size_t)ec->em.size * sizeof(uint32_t);      // at most 32 KB
    hipLaunchKernelGGL(lsim_k_elevation_map_cleanup, dim3((unsigned)ls_em_env_slots(ec->em)), dim3(LS_EM_BLOCK), lds, (hipStream_t)stream, *ec,
                       ls_em_tick_mod(ec->em), ls_em_rinv(ec->em));
    return hipGetLastError() == hipSuccess ? LSIM_OK : LSIM_E_HIP;
}
#endif
