// ls_sensor_shade.h -- shaded colour frames (include/lsim.h, lsim_sensor_shade): behind an lsim_raycast_bodies, the surface normal at every
// hit, whether the sun reaches that point, and a colour per pixel.  One launch for all envs and pixels.
//
// Self-contained like ls_raycast_bodies.h (only lsim.h, the two ray headers and the C library): tests/emu/emu_sensor_shade.cpp compiles this
// file with g++ under LS_EMU and runs the same per-block and per-pixel code over plain arrays.
//
// Shape of the launch (lsim_k_sensor_shade): lsim_k_raycast_bodies' -- blocks of 256 lanes over the pixels of ONE env, lane = pixel, the
// ls_rcb_block prologue (forward kinematics and the posed primitives in LDS, 3 KB), env and with it pose and mount block-uniform.
//   * The face of the hit is FOUND AGAIN, not carried over: the ray launch keeps its instructions (nothing is added to what it stores).
//     Terrain: the triangles of the 3 x 3 cells around the hit point's cell, each through ls_rc_tri itself with the ray's own o and d, the
//     first one nearest to the stored range -- 18 triangle tests at most, against a walk of tens of cells.  Body: the primitives of the
//     labelled body through ls_rcb_entry, primitive index wave-uniform as in ls_rcb_cast (an LDS broadcast, no divergence on `kind`).
//   * The shadow ray is ls_rcb_cast and then ls_rc_cast, called as they are with near = 0 and far = shadow_far (a copy of the struct with
//     other bounds, as ls_rcb_ray hands the walk a shorter `far`); the bodies first, so a pixel under the robot walks no cell.  A pixel of
//     the sky or one turned away from the sun casts none.
//   * rgba[e][r] is one coalesced 4-byte store per lane, surface[e][r] one 16-byte store per lane.
#pragma once
#include "ls_raycast_bodies.h"

#define LS_SS_LABELS (2 + LSIM_NUM_BODIES)

struct alignas(16) LsSsF4 { float x, y, z, w; };

LS_RC_FN LsRcV3 ls_ss_scaled(LsRcV3 v, float s) { return ls_rc_v3(v.x * s, v.y * s, v.z * s); }
LS_RC_FN LsRcV3 ls_ss_along(LsRcV3 o, LsRcV3 d, float t) { return ls_rc_v3(o.x + t * d.x, o.y + t * d.y, o.z + t * d.z); }
LS_RC_FN LsRcV3 ls_ss_unit(LsRcV3 v) { return ls_ss_scaled(v, 1.0f / sqrtf(ls_rc_dot(v, v))); }

// step 3: the triangle of the terrain hit -- t of that face (t0 when none is found) and its unit normal turned against the ray
LS_RC_FN LsRcV3 ls_ss_terrain_normal(const lsim_raycast_t& rc, LsRcV3 o, LsRcV3 d, float t0, float& t) {
    t = t0;
    LsRcV3 m = ls_rc_v3(0.0f, 0.0f, 1.0f);
    if (rc.mesh_type != 0 && rc.mesh) {
        const int rows = rc.grid_rows, cols = rc.grid_cols;
        const LsRcV3 p0 = ls_ss_along(o, d, t0);
        const int i = ls_rc_clampi((int)floorf((p0.x + rc.border_size) / rc.horizontal_scale), 0, rows - 2);
        const int j = ls_rc_clampi((int)floorf((p0.y + rc.border_size) / rc.horizontal_scale), 0, cols - 2);
        float nearest = LS_RC_BIG;
        // rolled on purpose, as the walk's 3 x 3 loop
#pragma unroll 1
        for (int c = 0; c < 9; ++c) {
            const int ci = i - 1 + c / 3, cj = j - 1 + c % 3;
            if (ci < 0 || cj < 0 || ci > rows - 2 || cj > cols - 2) continue;
            const int32_t* row = rc.mesh + (size_t)ci * (size_t)cols + (size_t)cj;
            const LsRcV3 p00 = ls_rc_vertex(rc, row[0], ci, cj), p10 = ls_rc_vertex(rc, row[cols], ci + 1, cj);
            const LsRcV3 p01 = ls_rc_vertex(rc, row[1], ci, cj + 1), p11 = ls_rc_vertex(rc, row[cols + 1], ci + 1, cj + 1);
#pragma unroll 1
            for (int k = 0; k < 2; ++k) {
                const LsRcV3 b = k == 0 ? p11 : p10, cc = k == 0 ? p01 : p11;
                const float tk = ls_rc_tri(o, d, p00, b, cc, rc.near, LS_RC_BIG);
                const float gap = fabsf(tk - t0);
                if (gap < nearest) { nearest = gap; t = tk; m = ls_rc_cross(ls_rc_sub(b, p00), ls_rc_sub(cc, p00)); }
            }
        }
    }
    LsRcV3 n = ls_ss_unit(m);
    if (ls_rc_dot(m, d) > 0.0f) n = ls_rc_v3(-n.x, -n.y, -n.z);
    return n;
}

// ray (o', d) in the frame of the posed primitive p of LsRcbShared: ls_rcb_cast's two products
LS_RC_FN void ls_ss_local(const float* p, LsRcV3 o, LsRcV3 d, LsRcV3& ol, LsRcV3& dl) {
    const LsRcV3 v = ls_rc_v3(o.x - p[0], o.y - p[1], o.z - p[2]);
    ol = ls_rc_v3(v.x * p[3] + v.y * p[4] + v.z * p[5], v.x * p[6] + v.y * p[7] + v.z * p[8], v.x * p[9] + v.y * p[10] + v.z * p[11]);
    dl = ls_rc_v3(d.x * p[3] + d.y * p[4] + d.z * p[5], d.x * p[6] + d.y * p[7] + d.z * p[8], d.x * p[9] + d.y * p[10] + d.z * p[11]);
}

// the outward unit normal of a primitive at the point x of its surface, in its own frame
LS_RC_FN LsRcV3 ls_ss_prim_normal(int kind, LsRcV3 x, float s0, float s1, float s2) {
    if (kind == LSIM_RAYCAST_PRIM_SPHERE) return ls_ss_unit(x);
    if (kind == LSIM_RAYCAST_PRIM_BOX) {
        const float g0 = fabsf(x.x) - s0, g1 = fabsf(x.y) - s1, g2 = fabsf(x.z) - s2;
        if (g0 >= g1 && g0 >= g2) return ls_rc_v3(x.x < 0.0f ? -1.0f : 1.0f, 0.0f, 0.0f);
        if (g1 >= g2) return ls_rc_v3(0.0f, x.y < 0.0f ? -1.0f : 1.0f, 0.0f);
        return ls_rc_v3(0.0f, 0.0f, x.z < 0.0f ? -1.0f : 1.0f);
    }
    if (kind == LSIM_RAYCAST_PRIM_CYLINDER) {
        const float rho = sqrtf(x.x * x.x + x.y * x.y);
        if (rho - s0 >= fabsf(x.z) - s1) return ls_rc_v3(x.x / rho, x.y / rho, 0.0f);
        return ls_rc_v3(0.0f, 0.0f, x.z < 0.0f ? -1.0f : 1.0f);
    }
    const float zc = fminf(fmaxf(x.z, -s1), s1);
    return ls_ss_unit(ls_rc_v3(x.x, x.y, x.z - zc));
}

// step 4: the primitive of body `body` that gave the hit -- its t_in and the outward normal there in world orientation; false: none
LS_RC_FN bool ls_ss_body_normal(const LsRcbShared& sh, LsRcV3 o, LsRcV3 d, int body, float t0, float& t, LsRcV3& n) {
    const int np = sh.nprims;
    float nearest = LS_RC_BIG;
    int which = -1;
#pragma unroll 1
    for (int i = 0; i < np; ++i) {
        const int kb = sh.kind[i];
        if (kb < 0 || (kb >> 8) != body) continue;
        const float* p = sh.prim[i];
        LsRcV3 ol, dl;
        ls_ss_local(p, o, d, ol, dl);
        const float ti = ls_rcb_entry(kb & 0xFF, ol, dl, p[12], p[13], p[14]);
        const float gap = fabsf(ti - t0);
        if (gap < nearest) { nearest = gap; t = ti; which = i; }
    }
    if (which < 0) return false;
    const float* p = sh.prim[which];
    LsRcV3 ol, dl;
    ls_ss_local(p, o, d, ol, dl);
    const LsRcV3 nl = ls_ss_prim_normal(sh.kind[which] & 0xFF, ls_ss_along(ol, dl, t), p[12], p[13], p[14]);
    n = ls_rc_v3(nl.x * p[3] + nl.y * p[6] + nl.z * p[9], nl.x * p[4] + nl.y * p[7] + nl.z * p[10], nl.x * p[5] + nl.y * p[8] + nl.z * p[11]);
    return true;
}

LS_RC_FN uint32_t ls_ss_channel(uint32_t byte, float gain) {
    const float v = fminf(fmaxf((float)byte * (1.0f / 255.0f) * gain, 0.0f), 1.0f);
    return (uint32_t)floorf(255.0f * v + 0.5f);
}

// pixel r of env: steps 1 - 6 of lsim.h, stored
LS_RC_FN void ls_ss_pixel(const lsim_sensor_shade_t& ss, const LsRcbShared& sh, int env, int r) {
    const lsim_raycast_bodies_t& rb = ss.rb;
    const lsim_raycast_t& rc = rb.rc;
    // the ray: ls_rcb_ray's expressions
    const float* rs = rc.root_states + (size_t)13 * (size_t)env;
    const float* mt = rc.mount + (size_t)7 * (size_t)env;
    float qx = rs[3], qy = rs[4], qz = rs[5], qw = rs[6];
    if (rb.flags & LSIM_RAYCAST_FRAME_YAW) {
        const float n = 1.0f / sqrtf(qz * qz + qw * qw);
        qx = 0.0f; qy = 0.0f; qz *= n; qw *= n;
    }
    const LsRcV3 mp = ls_rc_rot(qx, qy, qz, qw, ls_rc_v3(mt[0], mt[1], mt[2]));
    const LsRcV3 o = ls_rc_v3(rs[0] + mp.x, rs[1] + mp.y, rs[2] + mp.z);
    const LsRcV3 ds = ls_rc_rot(mt[3], mt[4], mt[5], mt[6], ls_rc_v3(rc.dirs[3 * r], rc.dirs[3 * r + 1], rc.dirs[3 * r + 2]));
    const LsRcV3 d = ls_rc_rot(qx, qy, qz, qw, ds);
    const LsRcV3 sun = ls_rc_v3(ss.sun[0], ss.sun[1], ss.sun[2]);
    int label = (int)rb.labels[(size_t)env * (size_t)rb.label_stride + (size_t)r];
    if (label >= LS_SS_LABELS) label = 0;
    const bool joints_ok = (sh.bad[0] | sh.bad[1] | sh.bad[2] | sh.bad[3]) == 0;
    if (!(joints_ok && ls_rc_finite(o.x) && ls_rc_finite(o.y) && ls_rc_finite(o.z) && ls_rc_finite(d.x) && ls_rc_finite(d.y) && ls_rc_finite(d.z))) {
        ls_rc_count((long long*)rc.state, 1);
        label = 0;
    }
    LsRcV3 n = ls_rc_v3(0.0f, 0.0f, 0.0f);
    float t = 0.0f, light = 0.0f;
    if (label != 0) {
        const float raw = rc.out[(size_t)env * (size_t)rc.out_stride + (size_t)r];
        const float t0 = rc.scale ? raw / rc.scale[r] : raw;
        if (label == 1) n = ls_ss_terrain_normal(rc, o, d, t0, t);
        else if (!ls_ss_body_normal(sh, mp, d, label - 2, t0, t, n)) label = 0;
    }
    uint32_t albedo = ss.palette[label];
    float k = 1.0f, dark = 1.0f;
    if (label != 0) {
        const float c = ls_rc_dot(n, sun);
        if (c > 0.0f) {
            light = 1.0f;
            if (ss.shade_flags & LSIM_SHADE_SHADOWS) {
                const LsRcV3 lift = ls_ss_scaled(n, ss.shadow_bias);
                const LsRcV3 pr = ls_ss_along(mp, d, t), pw = ls_ss_along(o, d, t);
                int met = 0, tested = 0;
                (void)ls_rcb_cast(sh, ls_rc_v3(pr.x + lift.x, pr.y + lift.y, pr.z + lift.z), sun, 0.0f, ss.shadow_far, met, tested);
                if (met == 0) {
                    LsRcCount cnt;
                    cnt.cells = 0; cnt.tris = 0;
                    lsim_raycast_t walk = rc;           // the shared walk over [0, shadow_far]
                    walk.near = 0.0f;
                    walk.far = ss.shadow_far;
                    met = ls_rc_cast(walk, ls_rc_v3(pw.x + lift.x, pw.y + lift.y, pw.z + lift.z), sun, cnt) < ss.shadow_far ? 1 : 0;
                }
                if (met != 0) light = 0.0f;
            }
        }
        k = ss.ambient + (1.0f - ss.ambient) * light * c;
        if (label == 1 && ss.checker > 0.0f) {
            const LsRcV3 pw = ls_ss_along(o, d, t);
            const int cells = (int)floorf(pw.x / ss.checker) + (int)floorf(pw.y / ss.checker);
            if (cells & 1) dark = ss.checker_gain;
        }
    }
    uint32_t word = (albedo & 0xFFFFFFu) | 0xFF000000u;
    if (label != 0) {
        const float g = k * dark;
        word = ls_ss_channel(albedo & 0xFFu, g) | (ls_ss_channel((albedo >> 8) & 0xFFu, g) << 8) | (ls_ss_channel((albedo >> 16) & 0xFFu, g) << 16) | 0xFF000000u;
    }
    ss.rgba[(size_t)env * (size_t)ss.rgba_stride + (size_t)r] = word;
    if (ss.surface) {
        LsSsF4 s;
        s.x = n.x; s.y = n.y; s.z = n.z; s.w = light;
        ((LsSsF4*)ss.surface)[(size_t)env * (size_t)rc.num_rays + (size_t)r] = s;
    }
}

// ---- host side: argument checks shared by the library and the CPU shim (no launch happens before they pass)
static inline bool ls_ss_host_nonneg(float v) { return ls_rc_host_finite(v) && v >= 0.0f; }
static inline int ls_ss_validate(const lsim_sensor_shade_t* ss) {
    if (!ss) return LSIM_E_INVALID;
    const int rv = ls_rcb_validate(&ss->rb);
    if (rv != LSIM_OK) return rv;
    if (!ss->rb.labels) return LSIM_E_INVALID;
    if (!ls_rc_aligned(ss->rgba, 16) || !ls_rc_aligned(ss->palette, 4) || (ss->surface && !ls_rc_aligned(ss->surface, 16))) return LSIM_E_INVALID;
    if (ss->rgba_stride < ss->rb.rc.num_rays || (ss->rgba_stride & 3) != 0) return LSIM_E_INVALID;
    if (!ls_rcb_host_finite3(ss->sun, 3)) return LSIM_E_INVALID;
    const float len2 = ss->sun[0] * ss->sun[0] + ss->sun[1] * ss->sun[1] + ss->sun[2] * ss->sun[2];
    if (!(fabsf(len2 - 1.0f) <= 1e-3f) || !(ss->sun[2] > 0.0f)) return LSIM_E_INVALID;
    if (!(ss->ambient >= 0.0f && ss->ambient <= 1.0f)) return LSIM_E_INVALID;
    if (!ls_ss_host_nonneg(ss->checker) || !ls_ss_host_nonneg(ss->checker_gain) || !ls_ss_host_nonneg(ss->shadow_bias) || !ls_ss_host_nonneg(ss->shadow_far)) return LSIM_E_INVALID;
    if (ss->shade_flags & ~(uint32_t)LSIM_SHADE_SHADOWS) return LSIM_E_INVALID;
    return LSIM_OK;
}

#if defined(__HIPCC__) && !defined(LS_EMU)
__global__ __launch_bounds__(LS_RC_BLOCK) void lsim_k_sensor_shade(const lsim_sensor_shade_t ss, int blocks_per_env) {
    __shared__ LsRcbShared sh;
    int env, r;
    ls_rc_block(ss.rb.rc, blocks_per_env, env, r);
    if (env >= ss.rb.rc.num_envs) return;       // the whole block: env is blockIdx's
    ls_rcb_block(ss.rb, sh, env, (int)threadIdx.x);
    if (r < ss.rb.rc.num_rays) ls_ss_pixel(ss, sh, env, r);
}

extern "C" int lsim_sensor_shade_sizes(size_t* state_bytes, size_t* palette_bytes) {
    if (!state_bytes || !palette_bytes) return LSIM_E_INVALID;
    *state_bytes = LSIM_RAYCAST_STATE_WORDS * sizeof(int64_t);
    *palette_bytes = LS_SS_LABELS * sizeof(uint32_t);
    return LSIM_OK;
}
extern "C" int lsim_sensor_shade(const lsim_sensor_shade_t* ss, void* stream) {
    const int rv = ls_ss_validate(ss);
    if (rv != LSIM_OK) return rv;
    int bpe;
    unsigned blocks;
    if (!ls_rc_grid(ss->rb.rc, bpe, blocks)) return LSIM_E_INVALID;
    hipLaunchKernelGGL(lsim_k_sensor_shade, dim3(blocks), dim3(LS_RC_BLOCK), 0, (hipStream_t)stream, *ss, bpe);
    return hipGetLastError() == hipSuccess ? LSIM_OK : LSIM_E_HIP;
}
#endif
