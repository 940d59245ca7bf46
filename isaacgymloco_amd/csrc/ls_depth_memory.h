// ls_depth_memory.h -- the depth memory (include/lsim.h, lsim_depth_memory_step, lsim_gru_sequence_forward / _backward): one GRU cell behind the
// depth encoder's latent row, stepped once per control step in the rollout and unrolled over a stored rollout chunk for its own training.
//
// Self-contained like its siblings (lsim.h, ls_sensor_model.h for the helpers, the C library): tests/emu/emu_depth_memory.cpp compiles this
// file with g++ under LS_EMU and runs the same validation, plan, tile split and index arithmetic with plain fp32 loops for the sums.
//
// Shape of all three launches: ONE workgroup of LS_GRU_BLOCK = 256 lanes (four waves) owns a TILE of LS_GRU_TILE = 16 consecutive envs -- the
// column extent of v_mfma_f32_16x16x4_f32 -- and no workgroup reads what another writes: no atomics, no exchange.  Every matrix product has the
// gate (or hidden) index on the rows of D and the env on its columns, D[unit 4 q + r][env i] for lane (i = lane & 15, q = lane >> 4), so a lane
// holds four consecutive units of ONE env, and a wave that owns hidden tile ht (16 units) forms the r, u and n rows of exactly those units in
// three accumulators: the gate math needs no lane movement.  Hidden tiles are dealt to the waves round-robin (ht = wave + 4 s, s < LS_GRU_SLOTS).
//   step      x = [z | p] and h_prev of the tile go to LDS; W_ih and W_hh are read once each, straight from global memory where torch keeps them
//             (L2-resident: every workgroup reads the same 3H rows); h' goes to h in place and to rows.
//   forward   W_hh goes to LDS once ([3H][H + 2]); the tile's h lives in two LDS buffers that swap every step, so ONE barrier per step; gi[t] of
//             a lane's own units is requested before the step's MFMAs.  Per step and wave: 3 H / 4 MFMAs per hidden tile, then the gate math.
//   backward  W_hh goes to LDS transposed ([H][3H + 2]); the total gradient dh stays in the registers of the lane that owns the unit; the gate
//             gradients [dr~ | du~ | dn~ r] of the tile go through one of two LDS buffers (one barrier per step) into the product with W_hh.
// Row pitches in LDS are (a multiple of 16) + 2 words: the A / B reads of a half-wave (i = 0..15, q = 0..1) then fall on 32 different banks.
// The weight pointers are cast to the global address space for the reason ls_policy.h gives (flat loads would count in lgkmcnt with the LDS reads).
#pragma once
#include "ls_sensor_model.h"

#define LS_GRU_BLOCK 256
#define LS_GRU_WAVES (LS_GRU_BLOCK / 64)
#define LS_GRU_TILE 16
#define LS_GRU_SLOTS (LSIM_GRU_MAX_HIDDEN / 16 / LS_GRU_WAVES)        // hidden tiles a wave owns at most

struct LsGruPlan {
    int H, I, HT;           // hidden, input (1 for the sequence launches), hidden tiles
    int ldx, ldh, ldg;      // LDS row pitches in words: x, h (and the rows of W_hh), the gate gradients (and the rows of W_hh transposed)
    int step_words, fwd_words, bwd_words;
};
static inline int ls_gru_pitch(int w) { return (w + 15) / 16 * 16 + 2; }
// the extents checked and the plan made; false: out of range or above the LDS budget
static inline bool ls_gru_plan(int hidden, int input, LsGruPlan& p) {
    if (hidden < 16 || (hidden & 15) != 0 || hidden > LSIM_GRU_MAX_HIDDEN) return false;
    if (input < 1 || input > LSIM_GRU_MAX_INPUT) return false;
    p.H = hidden; p.I = input; p.HT = hidden / 16;
    p.ldx = ls_gru_pitch(input); p.ldh = ls_gru_pitch(hidden); p.ldg = ls_gru_pitch(3 * hidden);
    p.step_words = LS_GRU_TILE * (p.ldx + p.ldh);
    p.fwd_words = (3 * hidden + 2 * LS_GRU_TILE) * p.ldh;
    p.bwd_words = (hidden + 2 * LS_GRU_TILE) * p.ldg;
    const int budget = LSIM_GRU_MAX_LDS_BYTES / 4;
    return p.step_words <= budget && p.fwd_words <= budget && p.bwd_words <= budget;
}
static inline int ls_gru_sizes(int hidden, int input, size_t* lds_step, size_t* lds_forward, size_t* lds_backward) {
    LsGruPlan p;
    if (!ls_gru_plan(hidden, input, p)) return LSIM_E_INVALID;
    if (lds_step) *lds_step = (size_t)p.step_words * 4u;
    if (lds_forward) *lds_forward = (size_t)p.fwd_words * 4u;
    if (lds_backward) *lds_backward = (size_t)p.bwd_words * 4u;
    return LSIM_OK;
}
static inline int ls_gru_tiles(int n) { return (n + LS_GRU_TILE - 1) / LS_GRU_TILE; }

// ---- index arithmetic and the cell's scalar math, shared by the kernels and the CPU shim
LS_RC_FN int ls_gru_unit(int ht, int q, int r) { return ht * 16 + 4 * q + r; }                      // the unit of D row 4 q + r of hidden tile ht
LS_RC_FN size_t ls_gru_at(int t, int n, int env, int width) { return ((size_t)t * (size_t)n + (size_t)env) * (size_t)width; }       // row (t, env) of a [T, n, width] array
LS_RC_FN bool ls_gru_fresh(uint32_t flags, const int64_t* episode_length, int env) { return ls_sensor_fresh(flags, episode_length, env); }
LS_RC_FN bool ls_gru_stepped(uint32_t flags, bool fresh) { return fresh || (flags & LSIM_SENSOR_RESETS_ONLY) == 0u; }
LS_RC_FN float ls_gru_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }
// pre-activations -> (r, u, n, h'); gh_n without r applied
LS_RC_FN float ls_gru_cell(float pre_r, float pre_u, float gi_n, float gh_n, float h_prev, float& r, float& u, float& n) {
    r = ls_gru_sigmoid(pre_r);
    u = ls_gru_sigmoid(pre_u);
    n = tanhf(gi_n + r * gh_n);
    return (1.0f - u) * n + u * h_prev;
}
// one unit's gate gradients from the total gradient dh: [0] dr~, [1] du~, [2] dn~, [3] dn~ * r; returns dh * u
LS_RC_FN float ls_gru_cell_bwd(float dh, float r, float u, float n, float gh_n, float h_prev, float* d) {
    const float dn = dh * (1.0f - u) * (1.0f - n * n);
    d[0] = dn * gh_n * r * (1.0f - r);
    d[1] = dh * (h_prev - n) * u * (1.0f - u);
    d[2] = dn;
    d[3] = dn * r;
    return dh * u;
}

// ---- host side: argument checks shared by the library and the CPU shim (no launch happens before they pass)
static inline int ls_dm_validate(const lsim_depth_memory_t* dm, LsGruPlan& p) {
    if (!dm) return LSIM_E_INVALID;
    if (!ls_rc_aligned(dm->z, 4) || !ls_rc_aligned(dm->h, 4) || !ls_rc_aligned(dm->episode_length, 8)) return LSIM_E_INVALID;
    if (!ls_rc_aligned(dm->weight_ih, 4) || !ls_rc_aligned(dm->weight_hh, 4) || !ls_rc_aligned(dm->bias_ih, 4) || !ls_rc_aligned(dm->bias_hh, 4)) return LSIM_E_INVALID;
    if (dm->num_envs < 1 || dm->latent_dim < 1 || dm->proprio_dim < 0) return LSIM_E_INVALID;
    if (dm->latent_dim > LSIM_GRU_MAX_INPUT || dm->proprio_dim > LSIM_GRU_MAX_INPUT) return LSIM_E_INVALID;           // before the sum
    if (!ls_gru_plan(dm->hidden, dm->latent_dim + dm->proprio_dim, p)) return LSIM_E_INVALID;
    if (dm->proprio_dim > 0 && (!ls_rc_aligned(dm->p, 4) || dm->p_ld < dm->proprio_dim)) return LSIM_E_INVALID;
    if (dm->z_ld < dm->latent_dim || dm->h_ld < dm->hidden) return LSIM_E_INVALID;
    if (dm->rows && (!ls_rc_aligned(dm->rows, 4) || dm->rows_ld < dm->latent_dim + dm->hidden)) return LSIM_E_INVALID;
    if (!ls_sensor_flags_ok(dm->flags)) return LSIM_E_INVALID;
    return LSIM_OK;
}
static inline int ls_gs_validate(const lsim_gru_sequence_t* gs, bool backward, LsGruPlan& p) {
    if (!gs) return LSIM_E_INVALID;
    if (!ls_rc_aligned(gs->h0, 16) || !ls_rc_aligned(gs->hs, 16) || !gs->reset || !ls_rc_aligned(gs->weight_hh, 4)) return LSIM_E_INVALID;
    if (backward) {
        if (!ls_rc_aligned(gs->save, 16) || !ls_rc_aligned(gs->dhs, 16) || !ls_rc_aligned(gs->dgi, 16) || !ls_rc_aligned(gs->dghn, 16)) return LSIM_E_INVALID;
        if (gs->dh0 && !ls_rc_aligned(gs->dh0, 16)) return LSIM_E_INVALID;
    } else {
        if (!ls_rc_aligned(gs->gi, 16) || !ls_rc_aligned(gs->bias_hh, 4)) return LSIM_E_INVALID;
        if (gs->save && !ls_rc_aligned(gs->save, 16)) return LSIM_E_INVALID;
    }
    if (gs->steps < 1 || gs->num_envs < 1) return LSIM_E_INVALID;
    if (!ls_gru_plan(gs->hidden, 1, p)) return LSIM_E_INVALID;
    return LSIM_OK;
}

#if defined(__HIPCC__) && !defined(LS_EMU)
#define LS_GRU_GLOBAL __attribute__((address_space(1)))
typedef const LS_GRU_GLOBAL float* ls_gru_gptr;
typedef float ls_gru_v4f __attribute__((ext_vector_type(4)));
extern __shared__ float ls_gru_lds[];

// three products that share their B operand: acc_g += W[g * H + row0 + (0..15)][0..K) . B[0..K)[env], g = 0, 1, 2.  W has row pitch ldw (global
// memory or LDS), B is the tile's [16][ldb] image in LDS; zero_b: the lane's env column is zero (a reset env).  A k past K multiplies two zeros.
template <typename WP>
__device__ __forceinline__ void ls_gru_mma3(WP w, int ldw, int H, int row0, int K, const float* bt, int ldb, bool zero_b, int i, int q,
                                            ls_gru_v4f& a0, ls_gru_v4f& a1, ls_gru_v4f& a2) {
    WP w0 = w + (size_t)(row0 + i) * (size_t)ldw, w1 = w0 + (size_t)H * (size_t)ldw, w2 = w1 + (size_t)H * (size_t)ldw;
    const float* brow = bt + i * ldb;
#pragma unroll 4
    for (int k0 = 0; k0 < K; k0 += 4) {
        const bool ok = k0 + q < K;
        const int k = ok ? k0 + q : K - 1;
        const float b = ok && !zero_b ? brow[k] : 0.0f;
        const float x0 = w0[k], x1 = w1[k], x2 = w2[k];
        a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ok ? x0 : 0.0f, b, a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ok ? x1 : 0.0f, b, a1, 0, 0, 0);
        a2 = __builtin_amdgcn_mfma_f32_16x16x4f32(ok ? x2 : 0.0f, b, a2, 0, 0, 0);
    }
}

__global__ __launch_bounds__(LS_GRU_BLOCK) void lsim_k_depth_memory_step(const lsim_depth_memory_t dm, const LsGruPlan p) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, q = lane >> 4;
    const int env0 = (int)blockIdx.x * LS_GRU_TILE, N = dm.num_envs, L = dm.latent_dim, H = p.H, I = p.I;
    if (dm.flags & LSIM_SENSOR_RESETS_ONLY) {       // a tile without a fresh env ends here, the whole block, before LDS
        const bool mine = tid < LS_GRU_TILE && env0 + tid < N && dm.episode_length[env0 + tid] == 0;
        if (!__syncthreads_or(mine ? 1 : 0)) return;
    }
    float* xt = ls_gru_lds;
    float* hb = ls_gru_lds + LS_GRU_TILE * p.ldx;
    for (int idx = tid; idx < LS_GRU_TILE * I; idx += LS_GRU_BLOCK) {
        const int e = idx / I, c = idx - e * I, env = env0 + e;
        float v = 0.0f;
        if (env < N) v = c < L ? dm.z[(size_t)env * (size_t)dm.z_ld + c] : dm.p[(size_t)env * (size_t)dm.p_ld + (c - L)];
        xt[e * p.ldx + c] = v;
    }
    for (int idx = tid; idx < LS_GRU_TILE * H; idx += LS_GRU_BLOCK) {
        const int e = idx / H, j = idx - e * H, env = env0 + e;
        float v = 0.0f;
        if (env < N && !ls_gru_fresh(dm.flags, dm.episode_length, env)) v = dm.h[(size_t)env * (size_t)dm.h_ld + j];
        hb[e * p.ldh + j] = v;
    }
    __syncthreads();
    const int env = env0 + i;
    const bool write = env < N && ls_gru_stepped(dm.flags, ls_gru_fresh(dm.flags, dm.episode_length, env));
    ls_gru_gptr bih = (ls_gru_gptr)dm.bias_ih, bhh = (ls_gru_gptr)dm.bias_hh;
    for (int ht = wave; ht < p.HT; ht += LS_GRU_WAVES) {
        const ls_gru_v4f zero = {0.0f, 0.0f, 0.0f, 0.0f};
        ls_gru_v4f ar = zero, au = zero, ain = zero, ahn = zero;
        ls_gru_mma3((ls_gru_gptr)dm.weight_ih, I, H, ht * 16, I, xt, p.ldx, false, i, q, ar, au, ain);
        ls_gru_mma3((ls_gru_gptr)dm.weight_hh, H, H, ht * 16, H, hb, p.ldh, false, i, q, ar, au, ahn);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = ls_gru_unit(ht, q, r);
            float gr, gu, gn;
            const float hn = ls_gru_cell(ar[r] + bih[j] + bhh[j], au[r] + bih[H + j] + bhh[H + j], ain[r] + bih[2 * H + j], ahn[r] + bhh[2 * H + j],
                                         hb[i * p.ldh + j], gr, gu, gn);
            if (write) {
                dm.h[(size_t)env * (size_t)dm.h_ld + j] = hn;
                if (dm.rows) dm.rows[(size_t)env * (size_t)dm.rows_ld + L + j] = hn;
            }
        }
    }
    if (dm.rows)
        for (int idx = tid; idx < LS_GRU_TILE * L; idx += LS_GRU_BLOCK) {
            const int e = idx / L, c = idx - e * L, ev = env0 + e;
            if (ev < N && ls_gru_stepped(dm.flags, ls_gru_fresh(dm.flags, dm.episode_length, ev))) dm.rows[(size_t)ev * (size_t)dm.rows_ld + c] = xt[e * p.ldx + c];
        }
}

__global__ __launch_bounds__(LS_GRU_BLOCK) void lsim_k_gru_sequence_forward(const lsim_gru_sequence_t gs, const LsGruPlan p) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, q = lane >> 4;
    const int env0 = (int)blockIdx.x * LS_GRU_TILE, n = gs.num_envs, H = p.H, T = gs.steps, ld = p.ldh;
    float* W = ls_gru_lds;
    float* hb = ls_gru_lds + 3 * H * ld;
    ls_gru_gptr whh = (ls_gru_gptr)gs.weight_hh, bhh = (ls_gru_gptr)gs.bias_hh;
    for (int idx = tid; idx < 3 * H * H; idx += LS_GRU_BLOCK) {
        const int m = idx / H;
        W[m * ld + (idx - m * H)] = whh[idx];
    }
    for (int idx = tid; idx < LS_GRU_TILE * H; idx += LS_GRU_BLOCK) {
        const int e = idx / H, j = idx - e * H;
        hb[e * ld + j] = env0 + e < n ? gs.h0[(size_t)(env0 + e) * (size_t)H + j] : 0.0f;
    }
    const int env = env0 + i, envc = env < n ? env : n - 1;        // a column past n computes on the last env's data and stores nothing
    const bool live = env < n;
    ls_gru_v4f br[LS_GRU_SLOTS], bu[LS_GRU_SLOTS], bn[LS_GRU_SLOTS];
#pragma unroll
    for (int s = 0; s < LS_GRU_SLOTS; ++s) {
        const int ht = wave + LS_GRU_WAVES * s, j0 = ls_gru_unit(ht < p.HT ? ht : 0, q, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) { br[s][r] = bhh[j0 + r]; bu[s][r] = bhh[H + j0 + r]; bn[s][r] = bhh[2 * H + j0 + r]; }
    }
    bool rs = gs.reset[envc] != 0;
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        const float* cur = hb + (t & 1) * LS_GRU_TILE * ld;
        float* nxt = hb + ((t + 1) & 1) * LS_GRU_TILE * ld;
        const bool rs_next = t + 1 < T ? gs.reset[(size_t)(t + 1) * (size_t)n + envc] != 0 : false;
#pragma unroll
        for (int s = 0; s < LS_GRU_SLOTS; ++s) {
            const int ht = wave + LS_GRU_WAVES * s;
            if (ht < p.HT) {
                const int j0 = ls_gru_unit(ht, q, 0);
                const ls_gru_v4f* g = (const ls_gru_v4f*)(gs.gi + ls_gru_at(t, n, envc, 3 * H) + j0);       // requested before the MFMAs
                const ls_gru_v4f gir = g[0], giu = g[H / 4], gin = g[2 * H / 4];
                const ls_gru_v4f zero = {0.0f, 0.0f, 0.0f, 0.0f};
                ls_gru_v4f ar = zero, au = zero, an = zero;
                ls_gru_mma3((const float*)W, ld, H, ht * 16, H, cur, ld, rs, i, q, ar, au, an);
                ls_gru_v4f vr, vu, vn, vg, vh;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float hp = rs ? 0.0f : cur[i * ld + j0 + r];
                    const float ghn = an[r] + bn[s][r];
                    float gr, gu, gn;
                    const float hn = ls_gru_cell(gir[r] + (ar[r] + br[s][r]), giu[r] + (au[r] + bu[s][r]), gin[r], ghn, hp, gr, gu, gn);
                    vr[r] = gr; vu[r] = gu; vn[r] = gn; vg[r] = ghn; vh[r] = hn;
                    nxt[i * ld + j0 + r] = hn;
                }
                if (live) {
                    *(ls_gru_v4f*)(gs.hs + ls_gru_at(t, n, env, H) + j0) = vh;
                    if (gs.save) {
                        ls_gru_v4f* sv = (ls_gru_v4f*)(gs.save + ls_gru_at(t, n, env, 4 * H) + j0);
                        sv[0] = vr; sv[H / 4] = vu; sv[2 * H / 4] = vn; sv[3 * H / 4] = vg;
                    }
                }
            }
        }
        rs = rs_next;
        __syncthreads();        // nxt is complete; cur may be overwritten in the step after next
    }
}

__global__ __launch_bounds__(LS_GRU_BLOCK) void lsim_k_gru_sequence_backward(const lsim_gru_sequence_t gs, const LsGruPlan p) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, q = lane >> 4;
    const int env0 = (int)blockIdx.x * LS_GRU_TILE, n = gs.num_envs, H = p.H, T = gs.steps, ld = p.ldg;
    float* WT = ls_gru_lds;                     // WT[k][m] = W_hh[m][k]
    float* db = ls_gru_lds + H * ld;
    ls_gru_gptr whh = (ls_gru_gptr)gs.weight_hh;
    for (int idx = tid; idx < 3 * H * H; idx += LS_GRU_BLOCK) {
        const int m = idx / H;
        WT[(idx - m * H) * ld + m] = whh[idx];
    }
    const int env = env0 + i, envc = env < n ? env : n - 1;
    const bool live = env < n;
    ls_gru_v4f dh[LS_GRU_SLOTS];
#pragma unroll
    for (int s = 0; s < LS_GRU_SLOTS; ++s) {
        const int ht = wave + LS_GRU_WAVES * s;
        dh[s] = (ls_gru_v4f){0.0f, 0.0f, 0.0f, 0.0f};
        if (ht < p.HT && live) dh[s] = *(const ls_gru_v4f*)(gs.dhs + ls_gru_at(T - 1, n, env, H) + ls_gru_unit(ht, q, 0));
    }
    __syncthreads();
    for (int t = T - 1; t >= 0; --t) {
        float* buf = db + (t & 1) * LS_GRU_TILE * ld;
        const bool rs = gs.reset[(size_t)t * (size_t)n + envc] != 0;
        ls_gru_v4f carry[LS_GRU_SLOTS], nextd[LS_GRU_SLOTS];
#pragma unroll
        for (int s = 0; s < LS_GRU_SLOTS; ++s) {
            const int ht = wave + LS_GRU_WAVES * s;
            carry[s] = nextd[s] = (ls_gru_v4f){0.0f, 0.0f, 0.0f, 0.0f};
            if (ht < p.HT) {
                const int j0 = ls_gru_unit(ht, q, 0);
                const ls_gru_v4f* sv = (const ls_gru_v4f*)(gs.save + ls_gru_at(t, n, envc, 4 * H) + j0);
                const ls_gru_v4f vr = sv[0], vu = sv[H / 4], vn = sv[2 * H / 4], vg = sv[3 * H / 4];
                ls_gru_v4f hp = {0.0f, 0.0f, 0.0f, 0.0f};
                if (!rs) hp = t > 0 ? *(const ls_gru_v4f*)(gs.hs + ls_gru_at(t - 1, n, envc, H) + j0) : *(const ls_gru_v4f*)(gs.h0 + (size_t)envc * (size_t)H + j0);
                if (t > 0 && live) nextd[s] = *(const ls_gru_v4f*)(gs.dhs + ls_gru_at(t - 1, n, env, H) + j0);        // requested before the product
                ls_gru_v4f dr, du, dn, dg;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float d[4];
                    carry[s][r] = ls_gru_cell_bwd(dh[s][r], vr[r], vu[r], vn[r], vg[r], hp[r], d);
                    dr[r] = d[0]; du[r] = d[1]; dn[r] = d[2]; dg[r] = d[3];
                    buf[i * ld + j0 + r] = d[0];
                    buf[i * ld + H + j0 + r] = d[1];
                    buf[i * ld + 2 * H + j0 + r] = d[3];
                }
                if (live) {
                    ls_gru_v4f* o = (ls_gru_v4f*)(gs.dgi + ls_gru_at(t, n, env, 3 * H) + j0);
                    o[0] = dr; o[H / 4] = du; o[2 * H / 4] = dn;
                    *(ls_gru_v4f*)(gs.dghn + ls_gru_at(t, n, env, H) + j0) = dg;
                }
            }
        }
        __syncthreads();        // the tile's gate gradients of step t are complete; the other buffer is free for step t - 1
#pragma unroll
        for (int s = 0; s < LS_GRU_SLOTS; ++s) {
            const int ht = wave + LS_GRU_WAVES * s;
            if (ht < p.HT) {
                const int j0 = ls_gru_unit(ht, q, 0);
                // two accumulators take alternate k-steps (the MFMA's dependent latency), added at the end: an order the extents fix
                ls_gru_v4f a0 = {0.0f, 0.0f, 0.0f, 0.0f}, a1 = {0.0f, 0.0f, 0.0f, 0.0f};
                const float* wrow = WT + (ht * 16 + i) * ld;
                const float* brow = buf + i * ld;
#pragma unroll 2
                for (int m0 = 0; m0 < 3 * H; m0 += 8) {           // 3 H is a multiple of 16
                    a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wrow[m0 + q], brow[m0 + q], a0, 0, 0, 0);
                    a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wrow[m0 + 4 + q], brow[m0 + 4 + q], a1, 0, 0, 0);
                }
                ls_gru_v4f v;
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = rs ? 0.0f : carry[s][r] + (a0[r] + a1[r]);
                if (t > 0) dh[s] = v + nextd[s];
                else if (gs.dh0 && live) *(ls_gru_v4f*)(gs.dh0 + (size_t)env * (size_t)H + j0) = v;
            }
        }
    }
}

extern "C" int lsim_depth_memory_sizes(int32_t hidden, int32_t input_dim, size_t* lds_step, size_t* lds_forward, size_t* lds_backward) {
    return ls_gru_sizes(hidden, input_dim, lds_step, lds_forward, lds_backward);
}

extern "C" int lsim_depth_memory_step(const lsim_depth_memory_t* dm, void* stream) {
    LsGruPlan p;
    const int rv = ls_dm_validate(dm, p);
    if (rv != LSIM_OK) return rv;
    static size_t configured[64] = {0};
    const size_t lds = (size_t)p.step_words * 4u;
    if (ls_allow_dynamic_lds((const void*)lsim_k_depth_memory_step, lds, configured) != LSIM_OK) return LSIM_E_HIP;
    hipLaunchKernelGGL(lsim_k_depth_memory_step, dim3((unsigned)ls_gru_tiles(dm->num_envs)), dim3(LS_GRU_BLOCK), lds, (hipStream_t)stream, *dm, p);
    return hipGetLastError() == hipSuccess ? LSIM_OK : LSIM_E_HIP;
}

extern "C" int lsim_gru_sequence_forward(const lsim_gru_sequence_t* gs, void* stream) {
    LsGruPlan p;
    const int rv = ls_gs_validate(gs, false, p);
    if (rv != LSIM_OK) return rv;
    static size_t configured[64] = {0};
    const size_t lds = (size_t)p.fwd_words * 4u;
    if (ls_allow_dynamic_lds((const void*)lsim_k_gru_sequence_forward, lds, configured) != LSIM_OK) return LSIM_E_HIP;
    hipLaunchKernelGGL(lsim_k_gru_sequence_forward, dim3((unsigned)ls_gru_tiles(gs->num_envs)), dim3(LS_GRU_BLOCK), lds, (hipStream_t)stream, *gs, p);
    return hipGetLastError() == hipSuccess ? LSIM_OK : LSIM_E_HIP;
}

extern "C" int lsim_gru_sequence_backward(const lsim_gru_sequence_t* gs, void* stream) {
    LsGruPlan p;
    const int rv = ls_gs_validate(gs, true, p);
    if (rv != LSIM_OK) return rv;
    static size_t configured[64] = {0};
    const size_t lds = (size_t)p.bwd_words * 4u;
    if (ls_allow_dynamic_lds((const void*)lsim_k_gru_sequence_backward, lds, configured) != LSIM_OK) return LSIM_E_HIP;
    hipLaunchKernelGGL(lsim_k_gru_sequence_backward, dim3((unsigned)ls_gru_tiles(gs->num_envs)), dim3(LS_GRU_BLOCK), lds, (hipStream_t)stream, *gs, p);
    return hipGetLastError() == hipSuccess ? LSIM_OK : LSIM_E_HIP;
}
#endif
