// ls_sensor_stereo.h -- stereo artefacts (include/lsim.h, lsim_sensor_stereo): behind a capture, the pixels of a z-depth image that a stereo pair
// reports no depth for (occlusion shadows, ranges below the minimum) become holes of the frame history, and pixels at a depth edge lose
// their depth or take the foreground's.  lsim.h states every formula; this file is that text in code.
//
// Self-contained like ls_elevation_map.h (lsim.h, the helpers of ls_raycast.h, the due rule of ls_sensor_model.h, ls_math.h and the C library):
// tests/emu/emu_sensor_stereo.cpp compiles this file with g++ under LS_EMU and runs the same per-lane functions, the lanes looped, each
// __syncthreads() a loop boundary and the LDS a plain array.
//
// Shape of the launch (lsim_k_sensor_stereo): ONE workgroup of 256 lanes per visited env, 16 + 12 R + (R rounded up to 4) bytes of dynamic
// LDS (39 952 B for the 64 x 48 image: four workgroups per CU).
//   0. ls_sensor_due first: the block of an env that is not due ends before LDS and before any barrier (the capture's step 0);
//   1. stage (ls_st_stage): the lanes sweep the image (r = lane, lane + 256, ...: the depth row, the labels and inv_scale are read coalesced)
//      and write Z and u to LDS -- both NaN for a pixel that is not valid, so that every comparison with it is false -- and whether the
//      pixel is too near into its outcome byte; barrier;
//   2. decide (ls_st_decide): every pixel from LDS alone -- the window loop over u along the row (lane = consecutive column: consecutive LDS
//      words, no bank conflict), the (2 radius + 1)^2 neighbourhood of Z, one Philox block for an edge pixel -- and, for a fattened pixel,
//      the GATHER of its foreground's value from slot K - 1 of hist.  The outcome (a byte) and the value go to LDS, the two counts to two
//      LDS words with one integer atomic per lane that has something to count; barrier;
//   3. store (ls_st_store): the slots of the rewritten pixels.  No lane stores to hist before the barrier and none reads hist behind it, so
//      whether a foreground pixel is itself rewritten plays no part; lanes 0 and 1 add the two counts to state, one atomic per word.
// Every branch around a barrier is on values the whole workgroup shares (env, due).  No floating-point atomic; two launches write the same bits.
#pragma once
#include "ls_sensor_model.h"
#include "ls_math.h"

#define LS_ST_BLOCK 256
#define LS_ST_KEEP 0
#define LS_ST_HOLE 1
#define LS_ST_FATTEN 2

struct LsStLds {
    uint32_t* cnt;      // [4] holes, fattened, two words of padding
    float* Z;           // [R] the depth, NaN where the pixel is not valid
    float* u;           // [R] the second imager's column, NaN likewise
    float* val;         // [R] the value a rewritten pixel takes
    uint8_t* code;      // [R rounded up to 4] LS_ST_KEEP / _HOLE / _FATTEN
};
static inline size_t ls_st_lds_bytes(long long R) { return (size_t)(16 + 12 * R + ((R + 3) & ~3LL)); }
LS_RC_FN LsStLds ls_st_carve(void* base, int R) {
    LsStLds l;
    l.cnt = (uint32_t*)base;
    l.Z = (float*)base + 4;
    l.u = l.Z + R;
    l.val = l.u + R;
    l.code = (uint8_t*)(l.val + R);
    return l;
}
#if defined(LS_EMU) || !defined(__HIPCC__)
LS_RC_FN void ls_st_add(uint32_t* p, uint32_t v) { *p += v; }
#else
LS_RC_FN void ls_st_add(uint32_t* p, uint32_t v) { (void)atomicAdd(p, v); }
#endif
LS_RC_FN int ls_st_imin(int a, int b) { return a < b ? a : b; }
LS_RC_FN int ls_st_imax(int a, int b) { return a > b ? a : b; }
LS_RC_FN float ls_st_nan() { const uint32_t b = 0x7FC00000u; float v; __builtin_memcpy(&v, &b, 4); return v; }

// what the env's instrument row changes: the focal length (step 2) and the slots the capture wrote (step 8)
LS_RC_FN float ls_st_fbe(const lsim_sensor_stereo_t& st, int env) {
    if (!st.inst) return st.fb;
    const float T = st.inst[(size_t)8 * (size_t)env + 4];
    return T != 1.0f ? ls_div_exact(st.fb, T) : st.fb;
}
LS_RC_FN int ls_st_first_slot(const lsim_sensor_stereo_t& st, int env, bool fill) {
    if (fill) return 0;
    if (!st.inst) return st.latency + st.frames - 1;
    const int L = ls_st_imin(ls_st_imax((int)st.inst[(size_t)8 * (size_t)env], 0), st.latency);
    return L + st.frames - 1;
}

// step 1: Z and u of this lane's pixels
LS_RC_FN void ls_st_stage(const lsim_sensor_stereo_t& st, int env, int lane, float fbe, const LsStLds& l) {
    const int W = st.width, R = W * st.height;
    const float* row = st.depth + (size_t)env * (size_t)st.depth_stride;
    const uint8_t* lab = st.labels ? st.labels + (size_t)env * (size_t)st.label_stride : (const uint8_t*)0;
    for (int r = lane; r < R; r += LS_ST_BLOCK) {
        const float Z = row[r];
        const float t = st.inv_scale ? Z * st.inv_scale[r] : Z;
        const bool valid = ls_rc_finite(Z) && st.t_lo < t && t < st.t_hi && (!lab || lab[r] != (uint8_t)0);
        const int c = r - (r / W) * W;
        const float delta = ls_div_exact(fbe, Z);
        l.Z[r] = valid ? Z : ls_st_nan();
        l.u[r] = valid ? (float)c - delta : ls_st_nan();
        l.code[r] = (uint8_t)(valid && delta > st.max_disparity);        // too near (step 4), kept for step 2 of this file
    }
}

// step 2: the outcome of this lane's pixels, from LDS; the foreground's value of a fattened pixel from hist
LS_RC_FN void ls_st_decide(const lsim_sensor_stereo_t& st, int env, int lane, const LsStLds& l) {
    const int W = st.width, H = st.height, R = W * H, K = st.latency + st.frames, rad = st.edge_radius;
    const float y_hole = (fminf(fmaxf(st.drop_value, st.clip_lo), st.clip_hi) - st.offset) * st.gain;
    const float keep = 1.0f - st.edge_rel;
    const float* newest = st.hist + ((size_t)env * (size_t)K + (size_t)(K - 1)) * (size_t)st.hist_stride;
    uint32_t holes = 0u, fat = 0u;
    for (int r = lane; r < R; r += LS_ST_BLOCK) {
        const float Z = l.Z[r];
        int code = LS_ST_KEEP;
        float val = 0.0f;
        if (Z == Z) {                       // valid
            const int y = r / W, c = r - y * W;
            const float u = l.u[r];
            const int last = ls_st_imin(W - 1, c + st.window);
            // the windowed minimum of u, NaN (not valid) skipped by fminf and NaN when no column is valid.  No early exit and eight loads
            // in flight: with an exit tested per column every iteration waited for its own LDS round trip (304 -> 210 us)
            float m = ls_st_nan();
            const float* urow = l.u + y * W;
            for (int cc = c + 1; cc <= last; cc += 8) {     // a column past `last` reads `last` again, which changes no minimum
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = urow[ls_st_imin(cc + j, last)];
#pragma unroll
                for (int j = 0; j < 8; ++j) m = fminf(m, v[j]);
            }
            bool hole = l.code[r] != (uint8_t)0 || m <= u;
            int fg = -1;
            if (!hole) {
                const float thr = Z * keep;
                float best = 0.0f;
                for (int yy = ls_st_imax(y - rad, 0); yy <= ls_st_imin(y + rad, H - 1); ++yy)
                    for (int cc = ls_st_imax(c - rad, 0); cc <= ls_st_imin(c + rad, W - 1); ++cc) {
                        const float Zn = l.Z[yy * W + cc];
                        if (Zn < thr && (fg < 0 || Zn < best)) { fg = yy * W + cc; best = Zn; }
                    }
            }
            if (fg >= 0) {
                uint32_t x[4] = {(uint32_t)env, (uint32_t)st.tick, (uint32_t)LSIM_RNG_SENSOR_STEREO, (st.stream_id << 16) | (uint32_t)r};
                philox4x32_10(x, st.seed, st.rank);
                const float u0 = u32_to_u01(x[0]);
                if (u0 < st.p_edge_hole) hole = true;
                else if (u0 < st.p_edge_cum) { code = LS_ST_FATTEN; val = newest[fg]; fat += 1u; }
            }
            if (hole) { code = LS_ST_HOLE; val = y_hole; holes += 1u; }
        }
        l.code[r] = (uint8_t)code;
        l.val[r] = val;
    }
    if (holes) ls_st_add(l.cnt, holes);
    if (fat) ls_st_add(l.cnt + 1, fat);
}

// step 3: the rewritten pixels into the slots the capture wrote, k0 .. K - 1
LS_RC_FN void ls_st_store(const lsim_sensor_stereo_t& st, int env, int lane, int k0, const LsStLds& l) {
    const int R = st.width * st.height, K = st.latency + st.frames;
    const size_t hs = (size_t)st.hist_stride;
    float* h = st.hist + (size_t)env * (size_t)K * hs;
    for (int r = lane; r < R; r += LS_ST_BLOCK) {
        if (l.code[r] == (uint8_t)LS_ST_KEEP) continue;
        const float v = l.val[r];
        for (int k = k0; k < K; ++k) h[(size_t)k * hs + (size_t)r] = v;
    }
}

// ---- host side: the argument checks shared by the library and the CPU shim (no launch happens before they pass)
static inline int ls_st_sizes(int32_t width, int32_t height, size_t* lds_bytes) {
    if (!lds_bytes || width < 1 || height < 1) return LSIM_E_INVALID;
    const long long R = (long long)width * (long long)height;
    if (R > LSIM_STEREO_MAX_LDS_BYTES / 12) return LSIM_E_INVALID;       // before the plan is formed: no overflow
    const size_t b = ls_st_lds_bytes(R);
    if (b > (size_t)LSIM_STEREO_MAX_LDS_BYTES) return LSIM_E_INVALID;
    *lds_bytes = b;
    return LSIM_OK;
}
static inline int ls_st_validate(const lsim_sensor_stereo_t* st) {
    if (!st) return LSIM_E_INVALID;
    if (!ls_rc_aligned(st->depth, 4) || !ls_rc_aligned(st->hist, 16) || !ls_rc_aligned(st->episode_length, 8) || !ls_rc_aligned(st->state, 8)) return LSIM_E_INVALID;
    if ((st->inv_scale && !ls_rc_aligned(st->inv_scale, 4)) || (st->inst && !ls_rc_aligned(st->inst, 16))) return LSIM_E_INVALID;
    size_t lds;
    if (ls_st_sizes(st->width, st->height, &lds) != LSIM_OK) return LSIM_E_INVALID;
    const int R = st->width * st->height;
    if (st->depth_stride < (int64_t)R || (st->labels && st->label_stride < R)) return LSIM_E_INVALID;
    if (st->hist_stride < R || (st->hist_stride & 3) != 0) return LSIM_E_INVALID;
    if (st->latency < 0 || st->frames < 1 || st->latency > LSIM_SENSOR_MAX_HISTORY || st->frames > LSIM_SENSOR_MAX_HISTORY ||
        st->latency + st->frames > LSIM_SENSOR_MAX_HISTORY) return LSIM_E_INVALID;
    if (st->num_envs < 1 || st->env_stride < 1 || st->tick < 0 || st->stream_id >= 65536u || st->period < 1 || st->stagger < 0 || st->stagger > 1) return LSIM_E_INVALID;
    if (!ls_sensor_flags_ok(st->flags)) return LSIM_E_INVALID;
    if (st->window < 1 || st->window > LSIM_STEREO_MAX_WINDOW || st->edge_radius < 0 || st->edge_radius > 3) return LSIM_E_INVALID;
    if (!ls_rc_host_finite(st->fb) || !(st->fb >= 0.0f) || !ls_rc_host_finite(st->edge_rel) || !(st->edge_rel >= 0.0f) || !(st->edge_rel < 1.0f)) return LSIM_E_INVALID;
    if (!ls_rc_host_finite(st->p_edge_hole) || !(st->p_edge_hole >= 0.0f) || !ls_rc_host_finite(st->p_edge_cum) || !(st->p_edge_cum <= 1.0f) ||
        !(st->p_edge_cum >= st->p_edge_hole)) return LSIM_E_INVALID;
    if (!(st->max_disparity > 0.0f)) return LSIM_E_INVALID;
    if (!(st->t_lo >= 0.0f) || !(st->t_lo < st->t_hi)) return LSIM_E_INVALID;
    if (!ls_rc_host_finite(st->drop_value) || !ls_rc_host_finite(st->clip_lo) || !ls_rc_host_finite(st->clip_hi) || !(st->clip_lo <= st->clip_hi) ||
        !ls_rc_host_finite(st->offset) || !ls_rc_host_finite(st->gain)) return LSIM_E_INVALID;
    return LSIM_OK;
}
static inline int ls_st_env_slots(const lsim_sensor_stereo_t& st) { return ls_sensor_env_slots(st.num_envs, st.env_stride); }
static inline uint32_t ls_st_tick_mod(const lsim_sensor_stereo_t& st) { return ls_sensor_tick_mod(st.tick, st.period); }

#if defined(__HIPCC__) && !defined(LS_EMU)
__global__ __launch_bounds__(LS_ST_BLOCK) void lsim_k_sensor_stereo(const lsim_sensor_stereo_t st, uint32_t tick_mod) {
    extern __shared__ uint32_t ls_st_lds[];
    const int env = (int)blockIdx.x * st.env_stride, lane = (int)threadIdx.x;      // < num_envs: blockIdx.x <= (num_envs - 1) / env_stride
    bool fill;
    if (!ls_sensor_due(st.flags, st.episode_length, st.period, st.stagger, env, tick_mod, fill)) return;      // the whole block, before LDS and the barriers
    const LsStLds l = ls_st_carve(ls_st_lds, st.width * st.height);
    const float fbe = ls_st_fbe(st, env);
    if (lane < 2) l.cnt[lane] = 0u;
    ls_st_stage(st, env, lane, fbe, l);
    __syncthreads();
    ls_st_decide(st, env, lane, l);
    __syncthreads();
    ls_st_store(st, env, lane, ls_st_first_slot(st, env, fill), l);
    if (lane < 2 && l.cnt[lane] != 0u) ls_rc_count((long long*)st.state + lane, (long long)l.cnt[lane]);
}

extern "C" int lsim_sensor_stereo_sizes(int32_t width, int32_t height, size_t* lds_bytes) { return ls_st_sizes(width, height, lds_bytes); }

extern "C" int lsim_sensor_stereo(const lsim_sensor_stereo_t* st, void* stream) {
    const int rv = ls_st_validate(st);
    if (rv != LSIM_OK) return rv;
    size_t lds;
    (void)ls_st_sizes(st->width, st->height, &lds);
    static size_t configured[64];
    const int av = ls_allow_dynamic_lds((const void*)lsim_k_sensor_stereo, lds, configured);
    if (av != LSIM_OK) return av;
    hipLaunchKernelGGL(lsim_k_sensor_stereo, dim3((unsigned)ls_st_env_slots(*st)), dim3(LS_ST_BLOCK), lds, (hipStream_t)stream, *st, ls_st_tick_mod(*st));
    return hipGetLastError() == hipSuccess ? LSIM_OK : LSIM_E_HIP;
}
#endif
