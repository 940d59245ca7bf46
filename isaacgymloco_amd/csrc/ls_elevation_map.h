// ls_elevation_map.h -- the elevation map (include/lsim.h, lsim_elevation_map): per env a world-aligned toroidal G x G height grid, filled
// from the depth rows a capture just wrote and the robot's own pose, and sampled at the points of the height scan.  lsim.h states every
// formula; this file is that text in code.
//
// Self-contained like ls_sensor_mount_jitter.h (lsim.h, the helpers of ls_raycast.h, the visit rule of ls_sensor_model.h, ls_math.h and the C
// library): tests/emu/emu_elevation_map.cpp compiles this file with g++ under LS_EMU and runs the same per-lane functions, the lanes looped and
// the LDS array a plain array.
//
// Shape of the launch (lsim_k_elevation_map): ONE workgroup of 256 lanes per visited env, G * G * 4 bytes of dynamic LDS (1, 4 or 16 KB).
//   0. the pose (14 floats, the same for all lanes: scalar loads) and ls_sensor_due;
//   1. fill: the lanes sweep the env's G * G stamps to -1 (slot = lane, lane + 256, ...: coalesced);
//   2. due: the LDS keys to 0, barrier; the lanes loop over the rays (r = lane, lane + 256, ...: the depth row is read coalesced), each valid
//      ray one ds_max_u32 on its slot's key; barrier; the lanes sweep the slots and write the touched ones (three dword stores each);
//   3. barrier (the scan reads what lanes of this workgroup just wrote to global memory: __syncthreads orders it at workgroup scope);
//      lane j < P looks its scan point up: two dependent 4-byte loads (stamp, cell), a third for a known cell, one store each to scan, known.
// Every branch around a barrier is on values the whole workgroup shares (env, fill, due, the pose), so all lanes reach every barrier.
// Per env and launch: 4 R bytes read, at most 12 G^2 written, 12 P read; at N = 4096, R = 3072, G = 32 with every env due about 50 MB + 50 MB.
#pragma once
#include "ls_sensor_model.h"
#include "ls_math.h"

#define LS_EM_BLOCK 256

struct LsEmPose {
    float px, py, pz, qx, qy, qz, qw;           // root_states[e][0:7]
    float mx, my, mz, ax, ay, az, aw;           // assumed_mount[e][0:7]
    int cx, cy;                                 // the window's centre cell
    bool ok;                                    // every component finite
};

// floor(x * rinv) as a float, and whether it is a cell the packed word can hold
LS_RC_FN float ls_em_cellf(float x, float rinv) { return floorf(x * rinv); }
LS_RC_FN bool ls_em_in_range(float f) { return f > -32768.0f && f < 32768.0f; }       // false for NaN
LS_RC_FN uint32_t ls_em_pack(int ix, int iy) { return ((uint32_t)(ix + 32768) << 16) | (uint32_t)(iy + 32768); }
LS_RC_FN int ls_em_slot(int ix, int iy, int G) { return (ix & (G - 1)) * G + (iy & (G - 1)); }
LS_RC_FN uint32_t ls_em_bits(float v) { uint32_t u; __builtin_memcpy(&u, &v, 4); return u; }
LS_RC_FN uint32_t ls_em_key(float z) { const uint32_t u = ls_em_bits(z); return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
LS_RC_FN float ls_em_unkey(uint32_t k) { const uint32_t u = k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu); float v; __builtin_memcpy(&v, &u, 4); return v; }
#if defined(LS_EMU) || !defined(__HIPCC__)
LS_RC_FN void ls_em_max(uint32_t* p, uint32_t v) { if (v > *p) *p = v; }
#else
LS_RC_FN void ls_em_max(uint32_t* p, uint32_t v) { (void)atomicMax(p, v); }
#endif

LS_RC_FN LsEmPose ls_em_pose(const lsim_elevation_map_t& em, int env, float rinv) {
    const float* rs = em.root_states + (size_t)13 * (size_t)env;
    const float* mt = em.assumed_mount + (size_t)7 * (size_t)env;
    LsEmPose s;
    s.px = rs[0]; s.py = rs[1]; s.pz = rs[2]; s.qx = rs[3]; s.qy = rs[4]; s.qz = rs[5]; s.qw = rs[6];
    s.mx = mt[0]; s.my = mt[1]; s.mz = mt[2]; s.ax = mt[3]; s.ay = mt[4]; s.az = mt[5]; s.aw = mt[6];
    s.ok = ls_rc_finite(s.px) && ls_rc_finite(s.py) && ls_rc_finite(s.pz) && ls_rc_finite(s.qx) && ls_rc_finite(s.qy) && ls_rc_finite(s.qz) &&
           ls_rc_finite(s.qw) && ls_rc_finite(s.mx) && ls_rc_finite(s.my) && ls_rc_finite(s.mz) && ls_rc_finite(s.ax) && ls_rc_finite(s.ay) &&
           ls_rc_finite(s.az) && ls_rc_finite(s.aw);
    s.cx = s.cy = 0;
    if (s.ok) {
        s.cx = (int)fminf(fmaxf(ls_em_cellf(s.px, rinv), -40000.0f), 40000.0f);
        s.cy = (int)fminf(fmaxf(ls_em_cellf(s.py, rinv), -40000.0f), 40000.0f);
    }
    return s;
}

// step 1: a new episode starts with an empty map
LS_RC_FN void ls_em_clear(const lsim_elevation_map_t& em, int env, int lane) {
    const int G2 = em.size * em.size;
    int32_t* st = em.stamp + (size_t)env * (size_t)G2;
    for (int s = lane; s < G2; s += LS_EM_BLOCK) st[s] = -1;
}

LS_RC_FN void ls_em_keys_clear(const lsim_elevation_map_t& em, uint32_t* keys, int lane) {
    const int G2 = em.size * em.size;
    for (int s = lane; s < G2; s += LS_EM_BLOCK) keys[s] = 0u;
}

// ray r of the env as a point of the map (row, lab: the env's depth row and label row, or null).  false: not kept; true: its slot and world
// height.  Both passes of the fused map (ls_elevation_fuse.h) call it; ls_em_insert below holds the same text once more
LS_RC_FN bool ls_em_point(const lsim_elevation_map_t& em, const LsEmPose& s, const float* row, const uint8_t* lab, int r, float rinv, int& slot, float& zout) {
    const int G = em.size, half = G >> 1;
    const float d = em.a * row[r] + em.b;
    const float t = em.inv_scale ? d * em.inv_scale[r] : d;
    if (!ls_rc_finite(d) || !(em.t_lo < t) || !(t < em.t_hi)) return false;
    if (lab && lab[r] != (uint8_t)1) return false;
    const LsRcV3 v = ls_rc_v3(em.dirs[3 * r] * t, em.dirs[3 * r + 1] * t, em.dirs[3 * r + 2] * t);
    const LsRcV3 m = ls_rc_rot(s.ax, s.ay, s.az, s.aw, v);
    const LsRcV3 b = ls_rc_rot(s.qx, s.qy, s.qz, s.qw, ls_rc_v3(s.mx + m.x, s.my + m.y, s.mz + m.z));
    const float x = s.px + b.x, y = s.py + b.y, z = s.pz + b.z;
    if (!ls_rc_finite(x) || !ls_rc_finite(y) || !ls_rc_finite(z)) return false;
    const float fx = ls_em_cellf(x, rinv), fy = ls_em_cellf(y, rinv);
    if (!ls_em_in_range(fx) || !ls_em_in_range(fy)) return false;
    const int ix = (int)fx, iy = (int)fy, dx = ix - s.cx, dy = iy - s.cy;
    if (dx < -half || dx >= half || dy < -half || dy >= half) return false;
    slot = ls_em_slot(ix, iy, G);
    zout = z;
    return true;
}

// step 2, first half: this lane's rays into the keys.  The loop body is ls_em_point's text ONCE MORE, with `continue` for `return false` and
// the maximum taken where the point is kept: called through ls_em_point, the compiler carries "kept" as a lane mask out of five nested
// regions and takes the maximum behind them (16 instructions, 2 VGPRs and 8 SGPRs more), and lsim_elevation_map measured 2.6 - 2.8 % slower
// (profiles/elevation_refactor_ab.json).  The copy serves this launch alone: the fused kernel forms the point with
// ls_em_point in both of its passes.  What pins the two texts to each other bit for bit is the fused map with band 0 and gate 0, whose
// maxima come from ls_em_point and which must equal this launch's map: tests/test_elevation_fuse.py::
// test_band_zero_gate_zero_is_the_plain_map_bit_for_bit and ::test_identity_on_general_poses, and on the device tests/test_gpu_elevation_fuse.py::
// test_identity_against_the_librarys_plain_map_on_the_exact_scenes and ::test_general_poses_identity_and_the_references_bracket.
LS_RC_FN void ls_em_insert(const lsim_elevation_map_t& em, const LsEmPose& s, int env, int lane, float rinv, uint32_t* keys) {
    const int G = em.size, half = G >> 1;
    const float* row = em.depth + (size_t)env * (size_t)em.depth_stride;
    const uint8_t* lab = em.labels ? em.labels + (size_t)env * (size_t)em.label_stride : (const uint8_t*)0;
    for (int r = lane; r < em.num_rays; r += LS_EM_BLOCK) {
        const float d = em.a * row[r] + em.b;
        const float t = em.inv_scale ? d * em.inv_scale[r] : d;
        if (!ls_rc_finite(d) || !(em.t_lo < t) || !(t < em.t_hi)) continue;
        if (lab && lab[r] != (uint8_t)1) continue;
        const LsRcV3 v = ls_rc_v3(em.dirs[3 * r] * t, em.dirs[3 * r + 1] * t, em.dirs[3 * r + 2] * t);
        const LsRcV3 m = ls_rc_rot(s.ax, s.ay, s.az, s.aw, v);
        const LsRcV3 b = ls_rc_rot(s.qx, s.qy, s.qz, s.qw, ls_rc_v3(s.mx + m.x, s.my + m.y, s.mz + m.z));
        const float x = s.px + b.x, y = s.py + b.y, z = s.pz + b.z;
        if (!ls_rc_finite(x) || !ls_rc_finite(y) || !ls_rc_finite(z)) continue;
        const float fx = ls_em_cellf(x, rinv), fy = ls_em_cellf(y, rinv);
        if (!ls_em_in_range(fx) || !ls_em_in_range(fy)) continue;
        const int ix = (int)fx, iy = (int)fy, dx = ix - s.cx, dy = iy - s.cy;
        if (dx < -half || dx >= half || dy < -half || dy >= half) continue;
        ls_em_max(keys + ls_em_slot(ix, iy, G), ls_em_key(z));
    }
}

// slot k = (sx, sy) holds the one cell (ix, iy) of the window centred on the pose that maps to it
LS_RC_FN void ls_em_window_cell(const LsEmPose& s, int G, int k, int& ix, int& iy) {
    const int wx = s.cx - (G >> 1), wy = s.cy - (G >> 1);
    const int sx = k / G, sy = k - sx * G;
    ix = wx + ((sx - wx) & (G - 1));
    iy = wy + ((sy - wy) & (G - 1));
}

// step 2, second half: the touched slots
LS_RC_FN void ls_em_commit(const lsim_elevation_map_t& em, const LsEmPose& s, int env, int lane, const uint32_t* keys) {
    const int G = em.size, G2 = G * G;
    const size_t base = (size_t)env * (size_t)G2;
    for (int k = lane; k < G2; k += LS_EM_BLOCK) {
        const uint32_t key = keys[k];
        if (key == 0u) continue;
        int ix, iy;
        ls_em_window_cell(s, G, k, ix, iy);
        em.height[base + (size_t)k] = ls_em_unkey(key);
        em.stamp[base + (size_t)k] = (int32_t)(em.tick & 0x7FFFFFFF);        // the low 31 bits: a stamp is never negative
        em.cell[base + (size_t)k] = ls_em_pack(ix, iy);
    }
}

// scan point j of an env with a finite pose, turned by the yaw alone: the slot of its cell where the map (base: the env's first slot) knows
// that cell, or -1.  `stamp` is the slot's (set for a slot that is returned): the fused scan ages the variance by it, and a second load of it
// there is not merged with this one by the compiler
LS_RC_FN int ls_em_lookup(const lsim_elevation_map_t& em, const LsEmPose& s, int j, size_t base, float rinv, int32_t& stamp) {
    const float n = ls_div_exact(1.0f, ls_sqrt_exact(s.qz * s.qz + s.qw * s.qw));
    const LsRcV3 o = ls_rc_rot(0.0f, 0.0f, s.qz * n, s.qw * n, ls_rc_v3(em.pts[2 * j], em.pts[2 * j + 1], 0.0f));
    const float fx = ls_em_cellf(s.px + o.x, rinv), fy = ls_em_cellf(s.py + o.y, rinv);
    if (!ls_em_in_range(fx) || !ls_em_in_range(fy)) return -1;
    const int ix = (int)fx, iy = (int)fy, k = ls_em_slot(ix, iy, em.size);
    stamp = em.stamp[base + (size_t)k];
    return stamp >= 0 && em.cell[base + (size_t)k] == ls_em_pack(ix, iy) ? k : -1;
}

// step 3: this lane's scan points
LS_RC_FN void ls_em_scan(const lsim_elevation_map_t& em, const LsEmPose& s, int env, int lane, float rinv) {
    const size_t base = (size_t)env * (size_t)(em.size * em.size);
    float* scan = em.scan + (size_t)env * (size_t)em.scan_stride;
    uint8_t* known = em.known + (size_t)env * (size_t)em.known_stride;
    for (int j = lane; j < em.num_points; j += LS_EM_BLOCK) {
        if (!s.ok) {
            scan[j] = 0.0f;
            known[j] = (uint8_t)0;
            continue;
        }
        int32_t stamp;
        const int k = ls_em_lookup(em, s, j, base, rinv, stamp);
        float h = s.pz - em.unknown_drop;
        uint8_t kn = (uint8_t)0;
        if (k >= 0) {
            h = em.height[base + (size_t)k];
            kn = (uint8_t)1;
        }
        scan[j] = h;
        known[j] = kn;
    }
}

// ---- host side: the argument check shared by the library and the CPU shim (no launch happens before it passes)
static inline int ls_em_validate(const lsim_elevation_map_t* em) {
    if (!em) return LSIM_E_INVALID;
    if (!ls_rc_aligned(em->root_states, 4) || !ls_rc_aligned(em->assumed_mount, 4) || !ls_rc_aligned(em->dirs, 4) || !ls_rc_aligned(em->depth, 4) ||
        !ls_rc_aligned(em->pts, 4) || !ls_rc_aligned(em->height, 4) || !ls_rc_aligned(em->stamp, 4) || !ls_rc_aligned(em->cell, 4) ||
        !ls_rc_aligned(em->scan, 4)) return LSIM_E_INVALID;
    if (em->inv_scale && !ls_rc_aligned(em->inv_scale, 4)) return LSIM_E_INVALID;
    if (!em->known || !ls_rc_aligned(em->episode_length, 8) || !ls_rc_aligned(em->state, 8)) return LSIM_E_INVALID;
    if (em->size != 16 && em->size != 32 && em->size != 64) return LSIM_E_INVALID;
    if (!ls_rc_host_finite(em->res) || !(em->res > 0.0f) || !ls_rc_host_finite(em->a) || !ls_rc_host_finite(em->b) ||
        !ls_rc_host_finite(em->unknown_drop)) return LSIM_E_INVALID;
    if (!(em->t_lo >= 0.0f) || !(em->t_lo < em->t_hi)) return LSIM_E_INVALID;
    if (em->num_points < 1 || em->num_points > LSIM_ELEVATION_MAP_MAX_POINTS || em->num_rays < 1 || em->num_rays > LSIM_RAYCAST_MAX_RAYS) return LSIM_E_INVALID;
    if (em->depth_stride < (int64_t)em->num_rays || (em->labels && em->label_stride < em->num_rays)) return LSIM_E_INVALID;
    if (em->scan_stride < em->num_points || em->known_stride < em->num_points) return LSIM_E_INVALID;
    if (em->tick < 0 || em->period < 1 || em->stagger < 0 || em->stagger > 1 || em->env_stride < 1 || em->num_envs < 1) return LSIM_E_INVALID;
    if (!ls_sensor_flags_ok(em->flags)) return LSIM_E_INVALID;
    return LSIM_OK;
}
static inline int ls_em_env_slots(const lsim_elevation_map_t& em) { return ls_sensor_env_slots(em.num_envs, em.env_stride); }
static inline uint32_t ls_em_tick_mod(const lsim_elevation_map_t& em) { return ls_sensor_tick_mod(em.tick, em.period); }
static inline float ls_em_rinv(const lsim_elevation_map_t& em) { return (float)(1.0 / (double)em.res); }

#if defined(__HIPCC__) && !defined(LS_EMU)
__global__ __launch_bounds__(LS_EM_BLOCK) void lsim_k_elevation_map(const lsim_elevation_map_t em, uint32_t tick_mod, float rinv) {
    extern __shared__ uint32_t ls_em_keys[];
    const int env = (int)blockIdx.x * em.env_stride, lane = (int)threadIdx.x;      // < num_envs: blockIdx.x <= (num_envs - 1) / env_stride
    bool fill;
    const bool due = ls_sensor_due(em.flags, em.episode_length, em.period, em.stagger, env, tick_mod, fill);
    const LsEmPose s = ls_em_pose(em, env, rinv);
    if (fill) ls_em_clear(em, env, lane);
    if (due && s.ok) {
        ls_em_keys_clear(em, ls_em_keys, lane);
        __syncthreads();
        ls_em_insert(em, s, env, lane, rinv, ls_em_keys);
        __syncthreads();
        ls_em_commit(em, s, env, lane, ls_em_keys);
    }
    __syncthreads();
    if (!s.ok && lane == 0) ls_rc_count((long long*)em.state, 1);
    ls_em_scan(em, s, env, lane, rinv);
}

extern "C" int lsim_elevation_map(const lsim_elevation_map_t* em, void* stream) {
    const int rv = ls_em_validate(em);
    if (rv != LSIM_OK) return rv;
    const size_t lds = (size_t)em->size * (size_t)em->size * sizeof(uint32_t);
    hipLaunchKernelGGL(lsim_k_elevation_map, dim3((unsigned)ls_em_env_slots(*em)), dim3(LS_EM_BLOCK), lds, (hipStream_t)stream, *em,
                       ls_em_tick_mod(*em), ls_em_rinv(*em));
    return hipGetLastError() == hipSuccess ? LSIM_OK : LSIM_E_HIP;
}
#endif
