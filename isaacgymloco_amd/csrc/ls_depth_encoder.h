// ls_depth_encoder.h -- the depth encoder (include/lsim.h, lsim_depth_encode): conv - ELU - conv - ELU - linear (- ELU) over the frame
// history a modelled range sensor keeps (ls_sensor_model.h), for the envs that are due on this tick only, one launch, forward only.
//
// Self-contained like its siblings (lsim.h, ls_sensor_model.h for the due rule, the C library): tests/emu/emu_depth_encoder.cpp compiles this
// file with g++ under LS_EMU and runs the same validation, plan, due rule and index arithmetic with plain fp32 loops for the sums.
//
// Shape of the launch (lsim_k_depth_encode): ONE workgroup of LS_DE_BLOCK = 256 lanes (four waves) per visited env.
//   0. ls_sensor_due first, as in lsim_k_sensor_capture: a block of an env that is not due ends before it touches LDS.  With period P and
//      stagger, P - 1 blocks in P are such empty blocks.
//   1. the env's image -- slots 0 .. frames - 1 of hist -- goes to LDS once, coalesced; the two tap tables are filled (ls_de_tap);
//   2. each convolution is an implicit GEMM on v_mfma_f32_16x16x4_f32: A = a 16 x 4 tile of the weights (16 output channels x 4 taps), read
//      straight from global memory where torch keeps them (row co of w[co][ci][ky][kx] IS the tap-major row of the GEMM), B = 4 taps x 16 output
//      positions gathered from the LDS image through the tap table (tap kk -> offset of (ci, ky, kx) in the input map) plus the position's own base
//      offset.  A wave owns LS_DE_PG position tiles of one channel tile at a time, so one weight value and one table entry feed LS_DE_PG MFMAs.
//      D[channel 4 q + r][position i] is four channels of one position per lane: bias, ELU, four stores to the next map in LDS;
//   3. the linear layer is a matrix-vector product per env (one column: no MFMA shape fits): a wave owns LS_DE_OG outputs at a time, its
//      lanes stride over the flattened a2 in LDS (16-byte vectors when w3 and the row length allow it, else single floats) against the
//      rows of w3 in global memory -- coalesced, L2-resident -- and a butterfly sums the 64 partial sums.
// LDS plan (LsDePlan; 4-byte words): [ X: the image, later a2 | A1 | taps of conv 1 | taps of conv 2 ].  conv 1 reads X and writes A1, conv 2
// reads A1 and writes a2 over the image, which is dead by then.  Activations never leave LDS; nothing but `latent` is written to memory.
// The weight pointers are cast to the global address space for the reason ls_policy.h gives (flat loads would count in lgkmcnt with the LDS reads).
#pragma once
#include "ls_sensor_model.h"

#define LS_DE_BLOCK 256
#define LS_DE_WAVES (LS_DE_BLOCK / 64)
#define LS_DE_PG 3          // position tiles per wave and pass of a convolution
#define LS_DE_OG 8          // outputs per wave and pass of the linear layer

struct LsDePlan {
    int h1, w1, h2, w2;     // output extents of the two convolutions
    int K1, K2, K3;         // dot-product lengths: frames*k1*k1, c1*k2*k2, c2*h2*w2
    int oA1, oT1, oT2;      // word offsets of A1 and the two tap tables (X is at 0)
    int words;              // LDS words in all
};

// the extents of `de` checked and the plan made; false: out of range or above the LDS budget
static inline bool ls_de_plan(const lsim_depth_encoder_t& de, LsDePlan& p) {
    if (de.height < 1 || de.width < 1 || de.frames < 1 || de.frames > LSIM_SENSOR_MAX_HISTORY) return false;
    if (de.c1 < 1 || de.c1 > LSIM_DEPTH_ENC_MAX_CHANNELS || de.c2 < 1 || de.c2 > LSIM_DEPTH_ENC_MAX_CHANNELS) return false;
    if (de.k1 < 1 || de.k1 > LSIM_DEPTH_ENC_MAX_KERNEL || de.k2 < 1 || de.k2 > LSIM_DEPTH_ENC_MAX_KERNEL) return false;
    if (de.s1 < 1 || de.s1 > LSIM_DEPTH_ENC_MAX_STRIDE || de.s2 < 1 || de.s2 > LSIM_DEPTH_ENC_MAX_STRIDE) return false;
    if (de.latent_dim < 1 || de.latent_dim > LSIM_DEPTH_ENC_MAX_LATENT) return false;
    if (de.k1 > de.height || de.k1 > de.width) return false;
    const long long budget = LSIM_DEPTH_ENC_MAX_LDS_BYTES / 4;
    const long long image = (long long)de.frames * de.height * de.width;        // <= 8 * 2^31 * 2^31: fits
    if ((long long)de.height * de.width > budget || image > budget) return false;
    p.h1 = (de.height - de.k1) / de.s1 + 1;
    p.w1 = (de.width - de.k1) / de.s1 + 1;
    if (de.k2 > p.h1 || de.k2 > p.w1) return false;
    p.h2 = (p.h1 - de.k2) / de.s2 + 1;
    p.w2 = (p.w1 - de.k2) / de.s2 + 1;
    const long long a1 = (long long)de.c1 * p.h1 * p.w1, a2 = (long long)de.c2 * p.h2 * p.w2;       // <= 64 * budget
    p.K1 = de.frames * de.k1 * de.k1;
    p.K2 = de.c1 * de.k2 * de.k2;
    const long long x = ((image > a2 ? image : a2) + 3) / 4 * 4, a1r = (a1 + 3) / 4 * 4;
    const long long words = x + a1r + p.K1 + p.K2;
    if (words > budget) return false;
    p.K3 = (int)a2;
    p.oA1 = (int)x;
    p.oT1 = (int)(x + a1r);
    p.oT2 = p.oT1 + p.K1;
    p.words = (int)words;
    return true;
}

// ---- index arithmetic shared by the kernel and the CPU shim
// tap kk = (ci * k + ky) * k + kx of a k x k kernel -> the offset of input element (ci, ky, kx) in a [C][hin][win] map
LS_RC_FN int ls_de_tap(int kk, int k, int hin, int win) {
    const int kx = kk % k, t = kk / k, ky = t % k, ci = t / k;
    return (ci * hin + ky) * win + kx;
}
// output position pos = y * wout + x of a convolution of stride s -> the offset of its window's first element in one [hin][win] plane
LS_RC_FN int ls_de_base(int pos, int wout, int s, int win) {
    const int y = pos / wout, x = pos - y * wout;
    return y * s * win + x * s;
}
// the first float of channel f of env's image in hist
LS_RC_FN size_t ls_de_slot(const lsim_depth_encoder_t& de, int env, int f) {
    return ((size_t)env * (size_t)de.hist_slots + (size_t)f) * (size_t)de.hist_stride;
}
LS_RC_FN float ls_de_elu(float v) { return v > 0.0f ? v : expm1f(v); }

// ---- host side: argument checks shared by the library and the CPU shim (no launch happens before they pass)
static inline int ls_de_validate(const lsim_depth_encoder_t* de, LsDePlan& p) {
    if (!de) return LSIM_E_INVALID;
    if (!ls_rc_aligned(de->hist, 16) || !ls_rc_aligned(de->latent, 16) || !ls_rc_aligned(de->episode_length, 8)) return LSIM_E_INVALID;
    if (!ls_rc_aligned(de->w1, 4) || !ls_rc_aligned(de->b1, 4) || !ls_rc_aligned(de->w2, 4) || !ls_rc_aligned(de->b2, 4) ||
        !ls_rc_aligned(de->w3, 4) || !ls_rc_aligned(de->b3, 4)) return LSIM_E_INVALID;
    if (de->num_envs < 1 || de->env_stride < 1) return LSIM_E_INVALID;
    if (!ls_de_plan(*de, p)) return LSIM_E_INVALID;
    if (de->hist_slots > LSIM_SENSOR_MAX_HISTORY || de->frames > de->hist_slots) return LSIM_E_INVALID;
    if ((long long)de->height * de->width > (long long)de->hist_stride || (de->hist_stride & 3) != 0) return LSIM_E_INVALID;
    if (de->final_act < 0 || de->final_act > 1) return LSIM_E_INVALID;
    if (de->latent_stride < de->latent_dim || (de->latent_stride & 3) != 0) return LSIM_E_INVALID;
    if (de->tick < 0 || de->period < 1 || de->stagger < 0 || de->stagger > 1) return LSIM_E_INVALID;
    if (!ls_sensor_flags_ok(de->flags)) return LSIM_E_INVALID;
    return LSIM_OK;
}
static inline int ls_de_sizes(const lsim_depth_encoder_t* de, size_t* lds_bytes) {
    LsDePlan p;
    if (!de || !lds_bytes || !ls_de_plan(*de, p)) return LSIM_E_INVALID;
    *lds_bytes = (size_t)p.words * 4u;
    return LSIM_OK;
}
static inline uint32_t ls_de_tick_mod(const lsim_depth_encoder_t& de) { return ls_sensor_tick_mod(de.tick, de.period); }
static inline int ls_de_env_slots(const lsim_depth_encoder_t& de) { return ls_sensor_env_slots(de.num_envs, de.env_stride); }

#if defined(__HIPCC__) && !defined(LS_EMU)
#define LS_DE_GLOBAL __attribute__((address_space(1)))
typedef const LS_DE_GLOBAL float* ls_de_gptr;
typedef float ls_de_v4f __attribute__((ext_vector_type(4)));
extern __shared__ float ls_de_lds[];

// one convolution: `in` [cin][hin][win] and `out` [cout][P] (P = hout * wout) in LDS, `tap` its table (K entries), w [cout][K] and b [cout] in
// global memory.  Work item = (channel tile, group of LS_DE_PG position tiles), dealt round-robin to the waves.
// Padding: a tap past K multiplies two zeros (x is zeroed as well as w: 0 * Inf would put a NaN where torch has none); a channel past cout
// or a position past P computes on clamped addresses into rows / columns of D that are not stored.
__device__ __forceinline__ void ls_de_conv(const float* in, float* out, const int* tap, ls_de_gptr w, ls_de_gptr b, int K, int cout, int P,
                                           int wout, int s, int win, int wave, int lane) {
    const int i = lane & 15, q = lane >> 4;
    const int ptiles = (P + 15) >> 4, pgroups = (ptiles + LS_DE_PG - 1) / LS_DE_PG, items = pgroups * ((cout + 15) >> 4);
    for (int item = wave; item < items; item += LS_DE_WAVES) {
        const int ct = item / pgroups, pg = item - ct * pgroups;
        int base[LS_DE_PG];
#pragma unroll
        for (int t = 0; t < LS_DE_PG; ++t) {
            const int pos = (pg * LS_DE_PG + t) * 16 + i;
            base[t] = ls_de_base(pos < P ? pos : 0, wout, s, win);
        }
        const int co = ct * 16 + i;
        ls_de_gptr wrow = w + (size_t)(co < cout ? co : cout - 1) * (size_t)K;
        ls_de_v4f acc[LS_DE_PG];
#pragma unroll
        for (int t = 0; t < LS_DE_PG; ++t) acc[t] = (ls_de_v4f){0.0f, 0.0f, 0.0f, 0.0f};
        // the weight and the table entry of step k0 + 4 are requested before the MFMAs of step k0
        int kc = q < K ? q : K - 1;
        float a = wrow[kc];
        int off = tap[kc];
#pragma unroll 2
        for (int k0 = 0; k0 < K; k0 += 4) {
            const bool ok = k0 + q < K;
            const int kn = k0 + 4 + q < K ? k0 + 4 + q : K - 1;
            const float a_next = wrow[kn];
            const int off_next = tap[kn];
            const float av = ok ? a : 0.0f;
#pragma unroll
            for (int t = 0; t < LS_DE_PG; ++t) {
                const float x = in[off + base[t]];
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, ok ? x : 0.0f, acc[t], 0, 0, 0);
            }
            a = a_next;
            off = off_next;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = ct * 16 + 4 * q + r;
            if (c < cout) {
                const float bias = b[c];
#pragma unroll
                for (int t = 0; t < LS_DE_PG; ++t) {
                    const int pos = (pg * LS_DE_PG + t) * 16 + i;
                    if (pos < P) out[c * P + pos] = ls_de_elu(acc[t][r] + bias);
                }
            }
        }
    }
}

// the linear layer of one env: a2 (K floats in LDS) against w3 [L][K]; VEC = 4: K % 4 == 0 and w3 16-byte aligned, else 1
template <int VEC>
__device__ __forceinline__ void ls_de_linear(const float* a2, ls_de_gptr w3, ls_de_gptr b3, int K, int L, int final_act, float* row, int wave, int lane) {
    for (int o0 = wave * LS_DE_OG; o0 < L; o0 += LS_DE_WAVES * LS_DE_OG) {
        float acc[LS_DE_OG];
        ls_de_gptr wr[LS_DE_OG];
#pragma unroll
        for (int g = 0; g < LS_DE_OG; ++g) {
            acc[g] = 0.0f;
            wr[g] = w3 + (size_t)(o0 + g < L ? o0 + g : L - 1) * (size_t)K;     // an output past L: a row that exists, a sum that is not stored
        }
        for (int j = lane * VEC; j < K; j += 64 * VEC) {
            if constexpr (VEC == 4) {
                const ls_de_v4f x = *(const ls_de_v4f*)(a2 + j);
#pragma unroll
                for (int g = 0; g < LS_DE_OG; ++g) {
                    const ls_de_v4f v = *(const LS_DE_GLOBAL ls_de_v4f*)(wr[g] + j);
                    acc[g] = fmaf(v.x, x.x, fmaf(v.y, x.y, fmaf(v.z, x.z, fmaf(v.w, x.w, acc[g]))));
                }
            } else {
                const float x = a2[j];
#pragma unroll
                for (int g = 0; g < LS_DE_OG; ++g) acc[g] = fmaf(wr[g][j], x, acc[g]);
            }
        }
        float mine = 0.0f;
#pragma unroll
        for (int g = 0; g < LS_DE_OG; ++g) {
            float v = acc[g];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
            if (lane == g) mine = v;
        }
        const int o = o0 + lane;
        if (lane < LS_DE_OG && o < L) {
            const float z = mine + b3[o];
            row[o] = final_act ? ls_de_elu(z) : z;
        }
    }
}

__global__ __launch_bounds__(LS_DE_BLOCK) void lsim_k_depth_encode(const lsim_depth_encoder_t de, const LsDePlan p, uint32_t tick_mod) {
    const int env = (int)blockIdx.x * de.env_stride;
    if (env >= de.num_envs) return;             // the whole block: env is blockIdx's
    bool fill;
    if (!ls_sensor_due(de.flags, de.episode_length, de.period, de.stagger, env, tick_mod, fill)) return;     // the whole block again, before LDS and the barriers
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* X = ls_de_lds;
    float* A1 = ls_de_lds + p.oA1;
    int* T1 = (int*)(ls_de_lds + p.oT1);
    int* T2 = (int*)(ls_de_lds + p.oT2);
    const int R = de.height * de.width;
    for (int f = 0; f < de.frames; ++f) {
        ls_de_gptr src = (ls_de_gptr)de.hist + ls_de_slot(de, env, f);
        for (int r = tid; r < R; r += LS_DE_BLOCK) X[f * R + r] = src[r];
    }
    for (int kk = tid; kk < p.K1; kk += LS_DE_BLOCK) T1[kk] = ls_de_tap(kk, de.k1, de.height, de.width);
    for (int kk = tid; kk < p.K2; kk += LS_DE_BLOCK) T2[kk] = ls_de_tap(kk, de.k2, p.h1, p.w1);
    __syncthreads();
    ls_de_conv(X, A1, T1, (ls_de_gptr)de.w1, (ls_de_gptr)de.b1, p.K1, de.c1, p.h1 * p.w1, p.w1, de.s1, de.width, wave, lane);
    __syncthreads();
    ls_de_conv(A1, X, T2, (ls_de_gptr)de.w2, (ls_de_gptr)de.b2, p.K2, de.c2, p.h2 * p.w2, p.w2, de.s2, p.w1, wave, lane);
    __syncthreads();
    float* row = de.latent + (size_t)env * (size_t)de.latent_stride;
    if ((p.K3 & 3) == 0 && ((uintptr_t)de.w3 & 15u) == 0u) ls_de_linear<4>(X, (ls_de_gptr)de.w3, (ls_de_gptr)de.b3, p.K3, de.latent_dim, de.final_act, row, wave, lane);
    else ls_de_linear<1>(X, (ls_de_gptr)de.w3, (ls_de_gptr)de.b3, p.K3, de.latent_dim, de.final_act, row, wave, lane);
}

extern "C" int lsim_depth_encode_sizes(const lsim_depth_encoder_t* de, size_t* lds_bytes) { return ls_de_sizes(de, lds_bytes); }

extern "C" int lsim_depth_encode(const lsim_depth_encoder_t* de, void* stream) {
    LsDePlan p;
    const int rv = ls_de_validate(de, p);
    if (rv != LSIM_OK) return rv;
    const size_t lds = (size_t)p.words * 4u;
    static size_t configured[64] = {0};
    if (ls_allow_dynamic_lds((const void*)lsim_k_depth_encode, lds, configured) != LSIM_OK) return LSIM_E_HIP;
    hipLaunchKernelGGL(lsim_k_depth_encode, dim3((unsigned)ls_de_env_slots(*de)), dim3(LS_DE_BLOCK), lds, (hipStream_t)stream, *de, p, ls_de_tick_mod(*de));
    return hipGetLastError() == hipSuccess ? LSIM_OK : LSIM_E_HIP;
}
#endif
