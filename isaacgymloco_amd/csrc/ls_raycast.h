// ls_raycast.h -- range sensors (include/lsim.h, lsim_raycast): rays against the terrain mesh, one launch for all envs and rays.
//
// Self-contained on purpose (only lsim.h and the C library), as ls_eval.h: the launch works on the raw pointers of an lsim_raycast, so
// tests/emu/emu_raycast.cpp compiles this file with g++ under LS_EMU and runs the same per-ray code over plain arrays.
//
// Shape of the launch (lsim_k_raycast): blocks of LS_RC_BLOCK = 256 lanes over the rays of ONE env, lane = ray (consecutive r), so
//   * env, and with it the base pose and the mount, depend on blockIdx alone: the compiler keeps them in SGPRs and fetches them with scalar
//     loads (no readfirstlane needed: nothing per-lane enters the address); every lane then rotates its own dirs[r] (a coalesced 12-byte read);
//   * a wave is 64 consecutive rays: one row of a 64-wide image, or 64 neighbouring azimuths of a lidar ring -- neighbouring rays walk
//     neighbouring cells, so the lanes of a wave leave the walk within a few cells of each other and re-use each other's mesh lines in L1 / L2;
//   * out[env][r] is one coalesced 4-byte store per lane, 256 bytes per wave.
// The walk (ls_rc_cast) is a 2-D DDA over the cells that the ray's ground projection crosses, front to back; per cell ONE word decides most of
// the work (the dz byte: nothing of the 4 x 4 vertex block reaches up to the ray -> skip; bit 20 clear: the cell's own two triangles; set: the
// triangles of the 3 x 3 cells around, which is what a displacement of at most one cell can stretch over this cell).  A triangle is never
// clipped to the cell that led to it: a hit found early is a hit, and the walk ends at the first cell whose exit lies behind the best hit.
// The ray itself (pose, non-finite rule, counters, cast, scale) is ONE function, ls_rc_value, taking the sensor-frame direction and scale as
// arguments: ls_rc_ray hands it the tables' and stores; the two capture kernels (ls_sensor_model.h, ls_sensor_instrument.h) call it
// directly.  ls_rc_grid is the one grid computation of the four ray launches and ls_rc_block their one block -> (env, ray) map.
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/lsim.h"

#if defined(LS_EMU) || !defined(__HIPCC__)
#define LS_RC_FN static inline
#else
#define LS_RC_FN __device__ __forceinline__
#endif

#define LS_RC_BLOCK 256
#ifndef LSIM_MESH_DZ_UNIT
#define LSIM_MESH_DZ_UNIT 4             // ls_api_impl.h: height steps per unit of a word's dz byte
#endif
#define LS_RC_ZMARGIN 1e-3f             // metres the ray must clear a block's top by before the block is skipped (covers the rounding of the span ends)
#define LS_RC_EDGE_EPS 3.814697265625e-6f    // 2^-18, lsim.h: the inclusive-edge slack relative to |edge| * |o - a|
#define LS_RC_BIG 3.0e38f

struct LsRcV3 { float x, y, z; };
struct LsRcCount { int cells, tris; };    // debug counters of one ray (written to state[2], state[3] only under LS_RAYCAST_COUNTERS)

LS_RC_FN LsRcV3 ls_rc_v3(float x, float y, float z) { LsRcV3 v; v.x = x; v.y = y; v.z = z; return v; }
LS_RC_FN LsRcV3 ls_rc_sub(LsRcV3 a, LsRcV3 b) { return ls_rc_v3(a.x - b.x, a.y - b.y, a.z - b.z); }
LS_RC_FN LsRcV3 ls_rc_cross(LsRcV3 a, LsRcV3 b) { return ls_rc_v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
LS_RC_FN float ls_rc_dot(LsRcV3 a, LsRcV3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
LS_RC_FN float ls_rc_maxabs(LsRcV3 a) { return fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fabsf(a.z)); }
LS_RC_FN bool ls_rc_finite(float v) { return fabsf(v) <= 3.402823466e38f; }
// R(q) v = v + 2 w (u x v) + 2 u x (u x v)
LS_RC_FN LsRcV3 ls_rc_rot(float qx, float qy, float qz, float qw, LsRcV3 v) {
    const LsRcV3 u = ls_rc_v3(qx, qy, qz);
    LsRcV3 t = ls_rc_cross(u, v);
    t = ls_rc_v3(2.0f * t.x, 2.0f * t.y, 2.0f * t.z);
    const LsRcV3 c = ls_rc_cross(u, t);
    return ls_rc_v3(v.x + qw * t.x + c.x, v.y + qw * t.y + c.y, v.z + qw * t.z + c.z);
}
LS_RC_FN LsRcV3 ls_rc_vertex(const lsim_raycast_t& rc, int word, int a, int b) {
    const float dx = (float)(((word >> 16) & 3) - 1), dy = (float)(((word >> 18) & 3) - 1);
    return ls_rc_v3(((float)a + dx) * rc.horizontal_scale - rc.border_size, ((float)b + dy) * rc.horizontal_scale - rc.border_size,
                    (float)(int16_t)(word & 0xFFFF) * rc.vertical_scale);
}

// triangle (a, b, c), either face, inclusive edges (lsim.h states the rule): the smaller of `best` and the hit's t in [near, best]
LS_RC_FN float ls_rc_tri(LsRcV3 o, LsRcV3 d, LsRcV3 a, LsRcV3 b, LsRcV3 c, float near, float best) {
    const LsRcV3 e1 = ls_rc_sub(b, a), e2 = ls_rc_sub(c, a);
    const LsRcV3 n = ls_rc_cross(e1, e2);
    if (ls_rc_dot(n, n) < 1e-16f) return best;            // collapsed: does not exist
    const float nd = ls_rc_dot(n, d);
    if (!(fabsf(nd) >= 1e-30f)) return best;              // parallel
    const LsRcV3 s = ls_rc_sub(o, a), q = ls_rc_cross(s, d);
    const float sg = nd < 0.0f ? -1.0f : 1.0f;
    const float U = -ls_rc_dot(e2, q) * sg, V = ls_rc_dot(e1, q) * sg, W = fabsf(nd) - U - V;
    const float m1 = ls_rc_maxabs(e1), m2 = ls_rc_maxabs(e2), ms = ls_rc_maxabs(s);
    const float E1 = LS_RC_EDGE_EPS * m1 * ms, E2 = LS_RC_EDGE_EPS * m2 * ms;
    if (U < -E2 || V < -E1 || W < -(E1 + E2 + 0.25f * LS_RC_EDGE_EPS * m1 * m2)) return best;
    const float t = -ls_rc_dot(n, s) / nd;
    return (t >= near && t <= best) ? t : best;
}

// the two triangles of cell (ci, cj): (p00, p11, p01) then (p00, p10, p11), the order of ls_wall_cell
LS_RC_FN float ls_rc_cell(const lsim_raycast_t& rc, LsRcV3 o, LsRcV3 d, int ci, int cj, float near, float best, LsRcCount& cnt) {
    const int32_t* row = rc.mesh + (size_t)ci * (size_t)rc.grid_cols + (size_t)cj;
    const LsRcV3 p00 = ls_rc_vertex(rc, row[0], ci, cj), p10 = ls_rc_vertex(rc, row[rc.grid_cols], ci + 1, cj);
    const LsRcV3 p01 = ls_rc_vertex(rc, row[1], ci, cj + 1), p11 = ls_rc_vertex(rc, row[rc.grid_cols + 1], ci + 1, cj + 1);
    cnt.tris += 2;
    // rolled on purpose, as in ls_wall_cell: two inlined copies of the triangle test per cell cost code and registers
#pragma unroll 1
    for (int t = 0; t < 2; ++t) best = ls_rc_tri(o, d, p00, t == 0 ? p11 : p10, t == 0 ? p01 : p11, near, best);
    return best;
}

LS_RC_FN int ls_rc_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the ray's result before scaling: smallest t in [near, far] on the terrain, or far
LS_RC_FN float ls_rc_cast(const lsim_raycast_t& rc, LsRcV3 o, LsRcV3 d, LsRcCount& cnt) {
    const float near = rc.near, far = rc.far;
    float best = far;
    if (rc.mesh_type == 0 || !rc.mesh) {
        if (fabsf(d.z) >= 1e-30f) {
            const float t = -o.z / d.z;
            if (t >= near && t <= far) best = t;
        }
        return best;
    }
    const int rows = rc.grid_rows, cols = rc.grid_cols;
    const float ihs = 1.0f / rc.horizontal_scale;
    const float gx = (o.x + rc.border_size) * ihs, gy = (o.y + rc.border_size) * ihs, ux = d.x * ihs, uy = d.y * ihs;   // in cells
    const float X = (float)(rows - 1), Y = (float)(cols - 1);
    const float ix = ux != 0.0f ? 1.0f / ux : 0.0f, iy = uy != 0.0f ? 1.0f / uy : 0.0f;
    float t0 = near, t1 = far;
    // the footprint's slabs: the part [t0, t1] of [near, far] above the grid
    if (ux != 0.0f) { const float ta = -gx * ix, tb = (X - gx) * ix; t0 = fmaxf(t0, fminf(ta, tb)); t1 = fminf(t1, fmaxf(ta, tb)); }
    else if (gx < 0.0f || gx > X) return best;
    if (uy != 0.0f) { const float ta = -gy * iy, tb = (Y - gy) * iy; t0 = fmaxf(t0, fminf(ta, tb)); t1 = fminf(t1, fmaxf(ta, tb)); }
    else if (gy < 0.0f || gy > Y) return best;
    if (!(t0 <= t1)) return best;
    int i = ls_rc_clampi((int)floorf(gx + ux * t0), 0, rows - 2), j = ls_rc_clampi((int)floorf(gy + uy * t0), 0, cols - 2);
    const int sx = ux > 0.0f ? 1 : -1, sy = uy > 0.0f ? 1 : -1;
    float tc = t0;
    for (int it = 0; it < rows + cols; ++it) {      // every pass moves i or j one cell in a fixed direction: at most rows + cols - 3 passes
        // the t at which the ray leaves cell (i, j) through its x / y side, from the cell index (no running sum: no drift); a vertical ray has neither
        const float tx = ux != 0.0f ? ((float)(i + (sx > 0 ? 1 : 0)) - gx) * ix : LS_RC_BIG;
        const float ty = uy != 0.0f ? ((float)(j + (sy > 0 ? 1 : 0)) - gy) * iy : LS_RC_BIG;
        const float te = fmaxf(fminf(fminf(tx, ty), t1), tc);
        const int w = rc.mesh[(size_t)i * (size_t)cols + (size_t)j];
        const int dz = (int)((uint32_t)w >> 24);
        const float top = ((float)(int16_t)(w & 0xFFFF) + (float)(dz * LSIM_MESH_DZ_UNIT)) * rc.vertical_scale;
        const float zlow = fminf(o.z + d.z * tc, o.z + d.z * te);
        cnt.cells += 1;
        if (dz < 255 && zlow - top > LS_RC_ZMARGIN) {
            // above everything in the 4 x 4 vertex block while over this cell: nothing to test
        } else if (!(w & (1 << 20))) {
            best = ls_rc_cell(rc, o, d, i, j, near, best, cnt);
        } else {
            // rolled on purpose, as ls_wall_serial: nine inlined copies of the cell test cost code and registers
#pragma unroll 1
            for (int c = 0; c < 9; ++c) {
                const int ci = i - 1 + c / 3, cj = j - 1 + c % 3;
                if (ci < 0 || cj < 0 || ci > rows - 2 || cj > cols - 2) continue;
                best = ls_rc_cell(rc, o, d, ci, cj, near, best, cnt);
            }
        }
        if (te >= best || te >= t1) break;
        if (tx <= ty) i += sx; else j += sy;
        if (i < 0 || j < 0 || i > rows - 2 || j > cols - 2) break;
        tc = te;
    }
    return best;
}

#if defined(LS_EMU) || !defined(__HIPCC__)
LS_RC_FN void ls_rc_count(long long* p, long long v) { *p += v; }
#else
LS_RC_FN void ls_rc_count(long long* p, long long v) { (void)atomicAdd((unsigned long long*)p, (unsigned long long)v); }
#endif

// THE terrain ray: the scaled range of one ray of env -- pose, cast, scale; hit = (t < far), label 1 / 0.  `s` points to the ray's direction in
// the sensor frame (3 floats) and `sc` to its scale (NULL: 1): the table callers pass rc.dirs + 3 r and rc.scale + r, the instrument the pair
// ls_si_ray made.  They come as pointers so that both are read where ls_rc_ray always read them, between the pose's scalar loads and the
// cast: with that lsim_k_raycast compiles to the instructions it had when this text was its own.  Every launch that casts a ray at the
// terrain alone calls this one function: lsim_k_raycast through ls_rc_ray, lsim_k_sensor_capture and lsim_k_sensor_capture_inst directly,
// and the CPU shims of all three.
LS_RC_FN float ls_rc_value(const lsim_raycast_t& rc, int env, const float* s, const float* sc, bool& hit, int& label) {
    const float* rs = rc.root_states + (size_t)13 * (size_t)env;
    const float* mt = rc.mount + (size_t)7 * (size_t)env;
    const LsRcV3 mp = ls_rc_rot(rs[3], rs[4], rs[5], rs[6], ls_rc_v3(mt[0], mt[1], mt[2]));
    const LsRcV3 o = ls_rc_v3(rs[0] + mp.x, rs[1] + mp.y, rs[2] + mp.z);
    const LsRcV3 ds = ls_rc_rot(mt[3], mt[4], mt[5], mt[6], ls_rc_v3(s[0], s[1], s[2]));
    const LsRcV3 d = ls_rc_rot(rs[3], rs[4], rs[5], rs[6], ds);
    const float scale = sc ? *sc : 1.0f;
    long long* state = (long long*)rc.state;
    float t = rc.far;
    if (ls_rc_finite(o.x) && ls_rc_finite(o.y) && ls_rc_finite(o.z) && ls_rc_finite(d.x) && ls_rc_finite(d.y) && ls_rc_finite(d.z)) {
        LsRcCount cnt;
        cnt.cells = 0; cnt.tris = 0;
        t = ls_rc_cast(rc, o, d, cnt);
#if defined(LS_RAYCAST_COUNTERS)
        ls_rc_count(state + 2, cnt.cells);
        ls_rc_count(state + 3, cnt.tris);
#endif
    } else {
        ls_rc_count(state, 1);
    }
    hit = t < rc.far;
    label = hit ? 1 : 0;
    return t * scale;
}

// ray r of env: the value at the tables' direction and scale, stored
LS_RC_FN void ls_rc_ray(const lsim_raycast_t& rc, int env, int r) {
    bool hit;
    int label;
    rc.out[(size_t)env * (size_t)rc.out_stride + (size_t)r] = ls_rc_value(rc, env, rc.dirs + 3 * r, rc.scale ? rc.scale + r : nullptr, hit, label);
}

// ---- host side: argument checks shared by the library and the CPU shim (no launch happens before they pass)
static inline bool ls_rc_aligned(const void* p, size_t a) { return p && ((uintptr_t)p & (a - 1)) == 0; }
static inline bool ls_rc_host_finite(float v) { return v == v && v <= 3.402823466e38f && v >= -3.402823466e38f; }
static inline int ls_rc_validate(const lsim_raycast_t* rc) {
    if (!rc) return LSIM_E_INVALID;
    if (!ls_rc_aligned(rc->root_states, 4) || !ls_rc_aligned(rc->mount, 4) || !ls_rc_aligned(rc->dirs, 4)) return LSIM_E_INVALID;
    if (rc->scale && !ls_rc_aligned(rc->scale, 4)) return LSIM_E_INVALID;
    if (!ls_rc_aligned(rc->out, 16) || !ls_rc_aligned(rc->state, 8)) return LSIM_E_INVALID;
    if (rc->num_envs < 1 || rc->num_rays < 1 || rc->num_rays > LSIM_RAYCAST_MAX_RAYS || rc->env_stride < 1) return LSIM_E_INVALID;
    if (rc->out_stride < rc->num_rays || (rc->out_stride & 3) != 0) return LSIM_E_INVALID;
    if (rc->mesh_type < 0 || rc->mesh_type > 2) return LSIM_E_INVALID;
    if (rc->mesh_type != 0) {
        if (!ls_rc_aligned(rc->mesh, 4) || rc->grid_rows < 2 || rc->grid_cols < 2) return LSIM_E_INVALID;
        if (!ls_rc_host_finite(rc->horizontal_scale) || !(rc->horizontal_scale > 0.0f) || !ls_rc_host_finite(rc->vertical_scale) ||
            !(rc->vertical_scale > 0.0f) || !ls_rc_host_finite(rc->border_size)) return LSIM_E_INVALID;
    }
    if (!(rc->near >= 0.0f) || !(rc->near < rc->far) || !ls_rc_host_finite(rc->far)) return LSIM_E_INVALID;
    return LSIM_OK;
}
static inline int ls_rc_blocks_per_env(const lsim_raycast_t& rc) { return (rc.num_rays + LS_RC_BLOCK - 1) / LS_RC_BLOCK; }
static inline int ls_rc_env_slots(const lsim_raycast_t& rc) { return (rc.num_envs + rc.env_stride - 1) / rc.env_stride; }
// the grid of the four ray launches: blocks per env, and blocks = that times the env slots; false when a grid does not hold them
static inline bool ls_rc_grid(const lsim_raycast_t& rc, int& blocks_per_env, unsigned& blocks) {
    blocks_per_env = ls_rc_blocks_per_env(rc);
    const long long n = (long long)blocks_per_env * ls_rc_env_slots(rc);
    blocks = (unsigned)n;
    return n <= 0x7fffffffLL;
}

#if defined(__HIPCC__) && !defined(LS_EMU)
// the map of all four ray kernels: block -> env (blockIdx alone: block-uniform), lane -> ray r of that env
__device__ __forceinline__ void ls_rc_block(const lsim_raycast_t& rc, int blocks_per_env, int& env, int& r) {
    const int slot = (int)blockIdx.x / blocks_per_env, chunk = (int)blockIdx.x - slot * blocks_per_env;
    env = slot * rc.env_stride;
    r = chunk * LS_RC_BLOCK + (int)threadIdx.x;
}

__global__ __launch_bounds__(LS_RC_BLOCK) void lsim_k_raycast(const lsim_raycast_t rc, int blocks_per_env) {
    int env, r;
    ls_rc_block(rc, blocks_per_env, env, r);
    if (r >= rc.num_rays || env >= rc.num_envs) return;
    ls_rc_ray(rc, env, r);
}

extern "C" int lsim_raycast_sizes(size_t* state_bytes) {
    if (!state_bytes) return LSIM_E_INVALID;
    *state_bytes = LSIM_RAYCAST_STATE_WORDS * sizeof(int64_t);
    return LSIM_OK;
}
extern "C" int lsim_raycast(const lsim_raycast_t* rc, void* stream) {
    const int rv = ls_rc_validate(rc);
    if (rv != LSIM_OK) return rv;
    int bpe;
    unsigned blocks;
    if (!ls_rc_grid(*rc, bpe, blocks)) return LSIM_E_INVALID;
    hipLaunchKernelGGL(lsim_k_raycast, dim3(blocks), dim3(LS_RC_BLOCK), 0, (hipStream_t)stream, *rc, bpe);
    return hipGetLastError() == hipSuccess ? LSIM_OK : LSIM_E_HIP;
}
#endif
