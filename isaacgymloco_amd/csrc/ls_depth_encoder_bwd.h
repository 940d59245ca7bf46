// ls_depth_encoder_bwd.h -- the depth encoder's backward pass (include/lsim.h, lsim_depth_encode_backward): the gradients of the six parameters
// of ls_depth_encoder.h's network from the gradient of its latent rows, for a batch of images.  The convolution activations are RECOMPUTED per
// sample in LDS with the forward's own routine (ls_de_conv) and never reach memory; what reaches the workspace is a2 and dz of every row (the
// operands of gw3 / gb3) and one partial sum of gw1 | gb1 | gw2 | gb2 per workgroup.
//
// Self-contained like ls_depth_encoder.h: tests/emu/emu_depth_encoder_backward.cpp compiles this file with g++ under LS_EMU and runs the same
// validation, plans, sample split, index arithmetic (ls_deb_dz, ls_deb_delu, ls_deb_da1, the tap and base tables, the partial layout) and the
// same order of the partial sums with plain fp32 loops where the kernels use MFMA tiles.
//
// Three launches, each on the caller's stream:
//   1. lsim_k_depth_encode_bwd: W = LsDebPlan.G persistent workgroups of LS_DE_BLOCK lanes; workgroup k loops over ITS samples (ls_deb_first /
//      ls_deb_count).  Per sample: image -> LDS, dz -> LDS and workspace, conv 1, conv 2 (ls_de_conv: the forward's implicit GEMMs; a2 gets a
//      region of its own because gw1 reads the image last), a2 -> workspace, da2 streamed over w3 (one column j per lane, the rows of w3
//      coalesced across lanes), d2 = da2 * ELU'(a2) over a2 in place; gb2 / gw2; da1 as a GATHER (ls_deb_da1: every a1 position sums the
//      (c, i, j) that reach it, in a fixed order -- no LDS atomics) and d1 = da1 * ELU'(a1) over a1 in place; gb1 / gw1.
//      A weight gradient is a GEMM per sample on v_mfma_f32_16x16x4_f32: D[channel][tap] += A[channel][4 positions] * B[4 positions][tap], A = d
//      in LDS, B gathered from the layer's input in LDS through the tap table (tap -> offset) and the base table (position -> offset).  A tile
//      (16 channels x 16 taps) is owned by the same wave and lanes for every sample, which add it to the workgroup's partial sum in the
//      workspace (the first sample stores): a read-modify-write by its one owner, in sample order.
//   2. lsim_k_depth_encode_bwd_fc: gw3 | gb3 = dz^T [a2 | 1] over the workspace rows, a wave per (16 columns of a2, up to 64 outputs), the batch
//      walked in order four rows per MFMA; column K3 of B is the constant 1, whose D column is gb3.
//   3. lsim_k_depth_encode_bwd_sum: the W partial sums added in the order of k into gw1, gb1, gw2, gb2.
// Nothing here depends on the arrival order of workgroups or waves: the same inputs, extents and W give the same bits.
#pragma once
#include "ls_depth_encoder.h"

#define LS_DEB_MAX_GRID 256                 // the kernel's own choice of W: one workgroup per CU of an MI355X (the LDS plan allows one per CU)
#define LS_DEB_PARTIAL_WORDS (8 << 20)      // ... but no more workgroups than keep all partial sums within 32 MB
#define LS_DEB_FC_OG 4                      // output tiles (16 outputs each) per wave of the gw3 launch

struct LsDebPlan {
    int G;                          // workgroups of launch 1
    int NP;                         // floats of one partial sum: gw1 | gb1 | gw2 | gb2
    int P1, P2;                     // positions of the two convolutions' outputs
    int oA1, oA2, oDZ, oT1, oT2, oB1, oB2;      // LDS word offsets (the image is at 0): a1, a2, dz, the tap tables, the base tables
    int oArgs;                      // ... and the launch's own arguments (LS_DEB_ARGS_WORDS, 16-byte aligned)
    int words;                      // LDS words in all
    long long wsDZ, wsPart;         // float offsets in the workspace (a2 rows are at 0)
    long long ws_bytes;
};

// the launch's arguments as the per-sample kernel keeps them in LDS (see ls_deb_arg)
struct LsDebArgs {
    lsim_depth_encoder_bwd_t db;
    LsDePlan p;
    LsDebPlan q;
};
#define LS_DEB_ARGS_WORDS ((int)((sizeof(LsDebArgs) + 15) / 16 * 4))

#if defined(__HIPCC__) && !defined(LS_EMU)
#define LS_DEB_HD __host__ __device__ static inline
#else
#define LS_DEB_HD static inline
#endif
// the forward's struct with db's extents and frame addressing (what ls_de_plan, ls_de_slot and ls_de_conv's callers read)
LS_DEB_HD lsim_depth_encoder_t ls_deb_forward(const lsim_depth_encoder_bwd_t& db) {
    lsim_depth_encoder_t de = {};
    de.hist = db.hist; de.w1 = db.w1; de.b1 = db.b1; de.w2 = db.w2; de.b2 = db.b2; de.w3 = db.w3; de.b3 = db.b3;
    de.hist_stride = db.hist_stride; de.hist_slots = db.hist_slots; de.num_envs = db.batch; de.env_stride = 1;
    de.height = db.height; de.width = db.width; de.frames = db.frames;
    de.c1 = db.c1; de.k1 = db.k1; de.s1 = db.s1; de.c2 = db.c2; de.k2 = db.k2; de.s2 = db.s2;
    de.latent_dim = db.latent_dim; de.final_act = db.final_act; de.latent_stride = db.latent_stride; de.period = 1;
    return de;
}

// batch, grid_limit and the extents checked, both plans made; false: out of range or above the LDS budget
static inline bool ls_deb_plan(const lsim_depth_encoder_bwd_t& db, lsim_depth_encoder_t& de, LsDePlan& p, LsDebPlan& q) {
    if (db.batch < 1 || db.grid_limit < 0) return false;
    de = ls_deb_forward(db);
    if (!ls_de_plan(de, p)) return false;               // every term below is within the forward's budget, so the sums fit
    q.P1 = p.h1 * p.w1;
    q.P2 = p.h2 * p.w2;
    const long long r4 = 3;
    const long long image = ((long long)de.frames * de.height * de.width + r4) / 4 * 4, a1 = ((long long)de.c1 * q.P1 + r4) / 4 * 4;
    const long long a2 = ((long long)p.K3 + r4) / 4 * 4, dz = ((long long)de.latent_dim + r4) / 4 * 4;
    const long long tables = ((long long)p.K1 + p.K2 + q.P1 + q.P2 + r4) / 4 * 4;
    const long long words = image + a1 + a2 + dz + tables + LS_DEB_ARGS_WORDS;
    if (words > LSIM_DEPTH_ENC_MAX_LDS_BYTES / 4) return false;
    q.oA1 = (int)image;
    q.oA2 = (int)(image + a1);
    q.oDZ = (int)(image + a1 + a2);
    q.oT1 = (int)(image + a1 + a2 + dz);
    q.oT2 = q.oT1 + p.K1;
    q.oB1 = q.oT2 + p.K2;
    q.oB2 = q.oB1 + q.P1;
    q.oArgs = (int)(words - LS_DEB_ARGS_WORDS);
    q.words = (int)words;
    q.NP = de.c1 * p.K1 + de.c1 + de.c2 * p.K2 + de.c2;             // <= 64 * 512 + 64 * 4096 + 128
    int cap = LS_DEB_PARTIAL_WORDS / q.NP;                          // >= 28
    if (cap > LS_DEB_MAX_GRID) cap = LS_DEB_MAX_GRID;
    if (db.grid_limit > 0 && db.grid_limit < cap) cap = db.grid_limit;
    q.G = db.batch < cap ? db.batch : cap;
    q.wsDZ = (long long)db.batch * p.K3;
    q.wsPart = (q.wsDZ + (long long)db.batch * de.latent_dim + r4) / 4 * 4;
    q.ws_bytes = 4 * (q.wsPart + (long long)cap * q.NP);            // `cap`, not G: the bytes grow with batch by the two rows only
    return true;
}

// ---- index arithmetic shared by the kernels and the CPU shim
// the samples of workgroup k of G: batch / G consecutive ones, the first batch % G workgroups one more
LS_RC_FN int ls_deb_first(int k, int batch, int G) { const int n = batch / G, r = batch % G; return k * n + (k < r ? k : r); }
LS_RC_FN int ls_deb_count(int k, int batch, int G) { return batch / G + (k < batch % G ? 1 : 0); }
// ELU' in terms of ELU's output
LS_RC_FN float ls_deb_delu(float a) { return a > 0.0f ? 1.0f : a + 1.0f; }
LS_RC_FN float ls_deb_dz(float g, float latent, int final_act) { return final_act ? g * ls_deb_delu(latent) : g; }
// word offsets of the four tensors in one partial sum
LS_RC_FN int ls_deb_part_gb1(int c1, int K1) { return c1 * K1; }
LS_RC_FN int ls_deb_part_gw2(int c1, int K1) { return c1 * K1 + c1; }
LS_RC_FN int ls_deb_part_gb2(int c1, int K1, int c2, int K2) { return c1 * K1 + c1 + c2 * K2; }
// da1 of a1's element (d, Y, X): the sum over the taps (i, j) of conv 2 whose window position (y, x) = ((Y - i) / s2, (X - j) / s2) exists, and over
// its output channels c, in the order i, j, c.  d2 [c2][h2][w2] (LDS), w2 [c2][c1][k2][k2] (WP: a global or a plain pointer)
template <class WP>
LS_RC_FN float ls_deb_da1(const float* d2, WP w2, int d, int Y, int X, int c1, int c2, int k2, int s2, int h2, int w2e) {
    float acc = 0.0f;
    for (int i = 0; i < k2 && i <= Y; ++i) {
        const int ty = Y - i, y = ty / s2;
        if (y * s2 != ty || y >= h2) continue;
        for (int j = 0; j < k2 && j <= X; ++j) {
            const int tx = X - j, x = tx / s2;
            if (x * s2 != tx || x >= w2e) continue;
            const float* dp = d2 + y * w2e + x;
            WP wp = w2 + ((size_t)d * k2 + i) * k2 + j;
            const size_t wstep = (size_t)c1 * k2 * k2;
            const int dstep = h2 * w2e;
            for (int c = 0; c < c2; ++c) acc = fmaf(wp[(size_t)c * wstep], dp[c * dstep], acc);
        }
    }
    return acc;
}

// ---- host side: argument checks shared by the library and the CPU shim (nothing is launched or written before they pass)
static inline int ls_deb_sizes(const lsim_depth_encoder_bwd_t* db, size_t* lds_bytes, size_t* workspace_bytes) {
    lsim_depth_encoder_t de;
    LsDePlan p;
    LsDebPlan q;
    if (!db || !lds_bytes || !workspace_bytes || !ls_deb_plan(*db, de, p, q)) return LSIM_E_INVALID;
    *lds_bytes = (size_t)q.words * 4u;
    *workspace_bytes = (size_t)q.ws_bytes;
    return LSIM_OK;
}
static inline int ls_deb_validate(const lsim_depth_encoder_bwd_t* db, lsim_depth_encoder_t& de, LsDePlan& p, LsDebPlan& q) {
    if (!db) return LSIM_E_INVALID;
    if (!ls_rc_aligned(db->hist, 16) || !ls_rc_aligned(db->workspace, 16)) return LSIM_E_INVALID;
    if (!ls_rc_aligned(db->w1, 4) || !ls_rc_aligned(db->b1, 4) || !ls_rc_aligned(db->w2, 4) || !ls_rc_aligned(db->b2, 4) ||
        !ls_rc_aligned(db->w3, 4) || !ls_rc_aligned(db->b3, 4) || !ls_rc_aligned(db->g, 4) || !ls_rc_aligned(db->latent, 4)) return LSIM_E_INVALID;
    if (!ls_rc_aligned(db->gw1, 4) || !ls_rc_aligned(db->gb1, 4) || !ls_rc_aligned(db->gw2, 4) || !ls_rc_aligned(db->gb2, 4) ||
        !ls_rc_aligned(db->gw3, 4) || !ls_rc_aligned(db->gb3, 4)) return LSIM_E_INVALID;
    if (!ls_deb_plan(*db, de, p, q)) return LSIM_E_INVALID;
    if (db->hist_slots > LSIM_SENSOR_MAX_HISTORY || db->frames > db->hist_slots) return LSIM_E_INVALID;
    if ((long long)db->height * db->width > (long long)db->hist_stride || (db->hist_stride & 3) != 0) return LSIM_E_INVALID;
    if (db->final_act < 0 || db->final_act > 1) return LSIM_E_INVALID;
    if (db->g_stride < db->latent_dim || db->latent_stride < db->latent_dim) return LSIM_E_INVALID;
    if (db->workspace_bytes < (uint64_t)q.ws_bytes) return LSIM_E_INVALID;
    return LSIM_OK;
}

#if defined(__HIPCC__) && !defined(LS_EMU)
typedef LS_DE_GLOBAL float* ls_de_gwptr;

// one layer's weight and bias gradient of one sample, added to the workgroup's partial sum (stored when `first`).  d [cout][P] (the gradient of
// the layer's pre-activation) and `in` (the layer's input) in LDS; tap [K], base [P] its tables; pw [cout][K], pb [cout] in the workspace.
// Work item = one 16 x 16 tile (channel tile, tap tile), dealt round-robin to the waves: the same wave and lane for every sample.
// Padding: a position past P multiplies two zeros; a channel past cout or a tap past K computes on clamped addresses into rows / columns of D
// that are not stored.
__device__ __forceinline__ void ls_deb_wgrad(const float* d, const float* in, const int* tap, const int* base, int K, int cout, int P,
                                             ls_de_gwptr pw, ls_de_gwptr pb, bool first, int wave, int lane) {
    const int i = lane & 15, q = lane >> 4;
    const int ktiles = (K + 15) >> 4, items = ktiles * ((cout + 15) >> 4);
    for (int item = wave; item < items; item += LS_DE_WAVES) {
        const int ct = item / ktiles, kt = item - ct * ktiles;
        const int c = ct * 16 + i, kk = kt * 16 + i;
        const float* drow = d + (c < cout ? c : cout - 1) * P;
        const float* col = in + tap[kk < K ? kk : K - 1];
        ls_de_v4f acc = (ls_de_v4f){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
        for (int p0 = 0; p0 < P; p0 += 4) {
            const int pos = p0 + q;
            const bool ok = pos < P;
            const int pc = ok ? pos : P - 1;
            const float a = drow[pc], x = col[base[pc]];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ok ? a : 0.0f, ok ? x : 0.0f, acc, 0, 0, 0);
        }
        if (kk < K) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int cc = ct * 16 + 4 * q + r;
                if (cc < cout) {
                    ls_de_gwptr dst = pw + (size_t)cc * (size_t)K + kk;
                    *dst = first ? acc[r] : *dst + acc[r];
                }
            }
        }
    }
    for (int c = wave; c < cout; c += LS_DE_WAVES) {
        float v = 0.0f;
        for (int pos = lane; pos < P; pos += 64) v += d[c * P + pos];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
        if (lane == 0) pb[c] = first ? v : pb[c] + v;
    }
}

// The launch's arguments live in LDS between the phases of a sample (LsDebArgs, written once): each phase reads the few it needs into scalar
// registers (ls_deb_arg: a broadcast LDS read made wave-uniform) behind the barrier that precedes it.  Kept as kernel arguments, the ~70 scalars
// of all phases and what the compiler derives from them stay live across the whole sample loop, more than the scalar register file holds.
__device__ __forceinline__ int ls_deb_arg(const int& v) { return __builtin_amdgcn_readfirstlane(v); }
template <class T>
__device__ __forceinline__ T* ls_deb_arg(T* const& v) {
    const uint64_t u = (uint64_t)(uintptr_t)v;
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(u >> 32));
    return (T*)(uintptr_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ long long ls_deb_arg(const long long& v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uint64_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (long long)(((uint64_t)hi << 32) | lo);
}

// ---- the phases of one sample b of workgroup k; S: the arguments in LDS, lds: the workgroup's dynamic LDS
__device__ __forceinline__ void ls_deb_load(const LsDebArgs* S, float* lds, int b, int tid) {
    const lsim_depth_encoder_bwd_t& db = S->db;
    const int frames = ls_deb_arg(db.frames), R = ls_deb_arg(db.height) * ls_deb_arg(db.width), L = ls_deb_arg(db.latent_dim);
    const size_t slot = (size_t)ls_deb_arg(db.hist_stride), slots = (size_t)ls_deb_arg(db.hist_slots);
    ls_de_gptr hist = (ls_de_gptr)ls_deb_arg(db.hist);
    for (int f = 0; f < frames; ++f) {
        ls_de_gptr src = hist + ((size_t)b * slots + (size_t)f) * slot;         // ls_de_slot
        for (int r = tid; r < R; r += LS_DE_BLOCK) lds[f * R + r] = src[r];
    }
    float* DZ = lds + ls_deb_arg(S->q.oDZ);
    ls_de_gptr g = (ls_de_gptr)ls_deb_arg(db.g) + (size_t)b * (size_t)ls_deb_arg(db.g_stride);
    ls_de_gptr lat = (ls_de_gptr)ls_deb_arg(db.latent) + (size_t)b * (size_t)ls_deb_arg(db.latent_stride);
    ls_de_gwptr wdz = (ls_de_gwptr)(float*)ls_deb_arg(db.workspace) + (size_t)ls_deb_arg(S->q.wsDZ) + (size_t)b * (size_t)L;
    const int final_act = ls_deb_arg(db.final_act);
    for (int o = tid; o < L; o += LS_DE_BLOCK) {
        const float v = ls_deb_dz(g[o], lat[o], final_act);
        DZ[o] = v;
        wdz[o] = v;
    }
}
__device__ __forceinline__ void ls_deb_conv1(const LsDebArgs* S, float* lds, int wave, int lane) {
    const lsim_depth_encoder_bwd_t& db = S->db;
    ls_de_conv(lds, lds + ls_deb_arg(S->q.oA1), (const int*)(lds + ls_deb_arg(S->q.oT1)), (ls_de_gptr)ls_deb_arg(db.w1), (ls_de_gptr)ls_deb_arg(db.b1),
               ls_deb_arg(S->p.K1), ls_deb_arg(db.c1), ls_deb_arg(S->q.P1), ls_deb_arg(S->p.w1), ls_deb_arg(db.s1), ls_deb_arg(db.width), wave, lane);
}
__device__ __forceinline__ void ls_deb_conv2(const LsDebArgs* S, float* lds, int wave, int lane) {
    const lsim_depth_encoder_bwd_t& db = S->db;
    ls_de_conv(lds + ls_deb_arg(S->q.oA1), lds + ls_deb_arg(S->q.oA2), (const int*)(lds + ls_deb_arg(S->q.oT2)), (ls_de_gptr)ls_deb_arg(db.w2),
               (ls_de_gptr)ls_deb_arg(db.b2), ls_deb_arg(S->p.K2), ls_deb_arg(db.c2), ls_deb_arg(S->q.P2), ls_deb_arg(S->p.w2), ls_deb_arg(db.s2),
               ls_deb_arg(S->p.w1), wave, lane);
}
// a2 to the workspace row; da2[j] = sum_o w3[o][j] dz[o], o ascending; d2 over a2 in place (element j is this lane's alone)
__device__ __forceinline__ void ls_deb_d2(const LsDebArgs* S, float* lds, int b, int tid) {
    const int K3 = ls_deb_arg(S->p.K3), L = ls_deb_arg(S->db.latent_dim);
    float* A2 = lds + ls_deb_arg(S->q.oA2);
    const float* DZ = lds + ls_deb_arg(S->q.oDZ);
    ls_de_gwptr row = (ls_de_gwptr)(float*)ls_deb_arg(S->db.workspace) + (size_t)b * (size_t)K3;
    ls_de_gptr w3 = (ls_de_gptr)ls_deb_arg(S->db.w3);
    for (int j = tid; j < K3; j += LS_DE_BLOCK) {
        const float a = A2[j];
        row[j] = a;
        ls_de_gptr wc = w3 + j;
        float acc = 0.0f;
#pragma unroll 8
        for (int o = 0; o < L; ++o) acc = fmaf(wc[(size_t)o * (size_t)K3], DZ[o], acc);
        A2[j] = acc * ls_deb_delu(a);
    }
}
__device__ __forceinline__ ls_de_gwptr ls_deb_partial(const LsDebArgs* S, int k) {
    return (ls_de_gwptr)(float*)ls_deb_arg(S->db.workspace) + (size_t)ls_deb_arg(S->q.wsPart) + (size_t)k * (size_t)ls_deb_arg(S->q.NP);
}
__device__ __forceinline__ void ls_deb_wgrad2(const LsDebArgs* S, float* lds, int k, bool first, int wave, int lane) {
    const int c1 = ls_deb_arg(S->db.c1), c2 = ls_deb_arg(S->db.c2), K1 = ls_deb_arg(S->p.K1), K2 = ls_deb_arg(S->p.K2);
    ls_de_gwptr part = ls_deb_partial(S, k);
    ls_deb_wgrad(lds + ls_deb_arg(S->q.oA2), lds + ls_deb_arg(S->q.oA1), (const int*)(lds + ls_deb_arg(S->q.oT2)), (const int*)(lds + ls_deb_arg(S->q.oB2)),
                 K2, c2, ls_deb_arg(S->q.P2), part + ls_deb_part_gw2(c1, K1), part + ls_deb_part_gb2(c1, K1, c2, K2), first, wave, lane);
}
// da1 as a gather, d1 = da1 * ELU'(a1) over a1 in place (element e is this lane's alone)
__device__ __forceinline__ void ls_deb_d1(const LsDebArgs* S, float* lds, int tid) {
    const int c1 = ls_deb_arg(S->db.c1), c2 = ls_deb_arg(S->db.c2), k2 = ls_deb_arg(S->db.k2), s2 = ls_deb_arg(S->db.s2);
    const int P1 = ls_deb_arg(S->q.P1), w1 = ls_deb_arg(S->p.w1), h2 = ls_deb_arg(S->p.h2), w2 = ls_deb_arg(S->p.w2);
    float* A1 = lds + ls_deb_arg(S->q.oA1);
    const float* D2 = lds + ls_deb_arg(S->q.oA2);
    ls_de_gptr W2 = (ls_de_gptr)ls_deb_arg(S->db.w2);
    for (int e = tid; e < c1 * P1; e += LS_DE_BLOCK) {
        const int d = e / P1, pos = e - d * P1, Y = pos / w1, X = pos - Y * w1;
        const float da = ls_deb_da1(D2, W2, d, Y, X, c1, c2, k2, s2, h2, w2);
        A1[e] = da * ls_deb_delu(A1[e]);
    }
}
__device__ __forceinline__ void ls_deb_wgrad1(const LsDebArgs* S, float* lds, int k, bool first, int wave, int lane) {
    const int c1 = ls_deb_arg(S->db.c1), K1 = ls_deb_arg(S->p.K1);
    ls_de_gwptr part = ls_deb_partial(S, k);
    ls_deb_wgrad(lds + ls_deb_arg(S->q.oA1), lds, (const int*)(lds + ls_deb_arg(S->q.oT1)), (const int*)(lds + ls_deb_arg(S->q.oB1)), K1, c1, ls_deb_arg(S->q.P1),
                 part, part + ls_deb_part_gb1(c1, K1), first, wave, lane);
}

__global__ __launch_bounds__(LS_DE_BLOCK) void lsim_k_depth_encode_bwd(const lsim_depth_encoder_bwd_t db, const LsDePlan p, const LsDebPlan q) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = (int)blockIdx.x;              // < q.G <= batch: every workgroup has a sample
    const int b0 = ls_deb_first(k, db.batch, q.G), nb = ls_deb_count(k, db.batch, q.G);
    float* lds = ls_de_lds;
    LsDebArgs* S = (LsDebArgs*)(lds + q.oArgs);
    if (tid == 0) {
        S->db = db;
        S->p = p;
        S->q = q;
    }
    int* T1 = (int*)(lds + q.oT1);
    int* T2 = (int*)(lds + q.oT2);
    int* B1 = (int*)(lds + q.oB1);
    int* B2 = (int*)(lds + q.oB2);
    for (int kk = tid; kk < p.K1; kk += LS_DE_BLOCK) T1[kk] = ls_de_tap(kk, db.k1, db.height, db.width);
    for (int kk = tid; kk < p.K2; kk += LS_DE_BLOCK) T2[kk] = ls_de_tap(kk, db.k2, p.h1, p.w1);
    for (int pos = tid; pos < q.P1; pos += LS_DE_BLOCK) B1[pos] = ls_de_base(pos, p.w1, db.s1, db.width);
    for (int pos = tid; pos < q.P2; pos += LS_DE_BLOCK) B2[pos] = ls_de_base(pos, p.w2, db.s2, p.w1);
    for (int s = 0; s < nb; ++s) {
        const int b = b0 + s;
        const bool first = s == 0;
        __syncthreads();                        // the arguments and the tables are written; the last sample's gw1 has read the image and d1
        ls_deb_load(S, lds, b, tid);
        __syncthreads();
        ls_deb_conv1(S, lds, wave, lane);
        __syncthreads();
        ls_deb_conv2(S, lds, wave, lane);
        __syncthreads();
        ls_deb_d2(S, lds, b, tid);
        __syncthreads();
        ls_deb_wgrad2(S, lds, k, first, wave, lane);
        __syncthreads();                        // gw2 has read a1
        ls_deb_d1(S, lds, tid);
        __syncthreads();
        ls_deb_wgrad1(S, lds, k, first, wave, lane);
    }
}

// gw3 [L][K3] | gb3 [L] from the workspace rows a2 [B][K3] and dz [B][L]: wave item = (column tile jt of K3 + 1 columns, group of LS_DEB_FC_OG
// output tiles); D[o][j] += dz[b][o] * (j < K3 ? a2[b][j] : 1), b ascending, four rows per MFMA
__global__ __launch_bounds__(LS_DE_BLOCK) void lsim_k_depth_encode_bwd_fc(const lsim_depth_encoder_bwd_t db, const LsDebPlan q, int K3, int jtiles, int items) {
    const int lane = (int)threadIdx.x & 63, item = (int)blockIdx.x * LS_DE_WAVES + ((int)threadIdx.x >> 6);
    if (item >= items) return;                  // the whole wave; no barrier follows
    const int i = lane & 15, r4 = lane >> 4, L = db.latent_dim, B = db.batch;
    const int og = item / jtiles, jt = item - og * jtiles;
    const int j = jt * 16 + i;
    ls_de_gptr a2 = (ls_de_gptr)(const float*)db.workspace;
    ls_de_gptr dz = a2 + (size_t)q.wsDZ;
    const int jc = j < K3 ? j : 0;
    int oc[LS_DEB_FC_OG];
    ls_de_v4f acc[LS_DEB_FC_OG];
#pragma unroll
    for (int t = 0; t < LS_DEB_FC_OG; ++t) {
        const int o = (og * LS_DEB_FC_OG + t) * 16 + i;
        oc[t] = o < L ? o : L - 1;
        acc[t] = (ls_de_v4f){0.0f, 0.0f, 0.0f, 0.0f};
    }
#pragma unroll 2
    for (int b0 = 0; b0 < B; b0 += 4) {
        const int b = b0 + r4;
        const bool ok = b < B;
        const size_t bc = (size_t)(ok ? b : B - 1);
        const float xv = a2[bc * (size_t)K3 + jc];
        const float x = ok ? (j < K3 ? xv : 1.0f) : 0.0f;
#pragma unroll
        for (int t = 0; t < LS_DEB_FC_OG; ++t) {
            const float a = dz[bc * (size_t)L + oc[t]];
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ok ? a : 0.0f, x, acc[t], 0, 0, 0);
        }
    }
    if (j > K3) return;
#pragma unroll
    for (int t = 0; t < LS_DEB_FC_OG; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = (og * LS_DEB_FC_OG + t) * 16 + 4 * r4 + r;
            if (o < L) {
                if (j < K3) db.gw3[(size_t)o * (size_t)K3 + j] = acc[t][r];
                else db.gb3[o] = acc[t][r];
            }
        }
}

// the G partial sums gw1 | gb1 | gw2 | gb2 added in the order of the workgroups
__global__ __launch_bounds__(LS_DE_BLOCK) void lsim_k_depth_encode_bwd_sum(const lsim_depth_encoder_bwd_t db, const LsDebPlan q, int K1, int K2) {
    const int idx = (int)(blockIdx.x * LS_DE_BLOCK + threadIdx.x);
    if (idx >= q.NP) return;
    ls_de_gptr part = (ls_de_gptr)(const float*)db.workspace + (size_t)q.wsPart + idx;
    float v = part[0];
    for (int k = 1; k < q.G; ++k) v += part[(size_t)k * (size_t)q.NP];
    const int ob1 = ls_deb_part_gb1(db.c1, K1), ow2 = ls_deb_part_gw2(db.c1, K1), ob2 = ls_deb_part_gb2(db.c1, K1, db.c2, K2);
    if (idx < ob1) db.gw1[idx] = v;
    else if (idx < ow2) db.gb1[idx - ob1] = v;
    else if (idx < ob2) db.gw2[idx - ow2] = v;
    else db.gb2[idx - ob2] = v;
}

extern "C" int lsim_depth_encode_backward_sizes(const lsim_depth_encoder_bwd_t* db, size_t* lds_bytes, size_t* workspace_bytes) {
    return ls_deb_sizes(db, lds_bytes, workspace_bytes);
}

extern "C" int lsim_depth_encode_backward(const lsim_depth_encoder_bwd_t* db, void* stream) {
    lsim_depth_encoder_t de;
    LsDePlan p;
    LsDebPlan q;
    const int rv = ls_deb_validate(db, de, p, q);
    if (rv != LSIM_OK) return rv;
    const size_t lds = (size_t)q.words * 4u;
    static size_t configured[64] = {0};
    if (ls_allow_dynamic_lds((const void*)lsim_k_depth_encode_bwd, lds, configured) != LSIM_OK) return LSIM_E_HIP;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(lsim_k_depth_encode_bwd, dim3((unsigned)q.G), dim3(LS_DE_BLOCK), lds, st, *db, p, q);
    const int jtiles = (p.K3 + 1 + 15) >> 4, otiles = (db->latent_dim + 15) >> 4;
    const int items = jtiles * ((otiles + LS_DEB_FC_OG - 1) / LS_DEB_FC_OG);
    hipLaunchKernelGGL(lsim_k_depth_encode_bwd_fc, dim3((unsigned)((items + LS_DE_WAVES - 1) / LS_DE_WAVES)), dim3(LS_DE_BLOCK), 0, st, *db, q, p.K3, jtiles, items);
    hipLaunchKernelGGL(lsim_k_depth_encode_bwd_sum, dim3((unsigned)((q.NP + LS_DE_BLOCK - 1) / LS_DE_BLOCK)), dim3(LS_DE_BLOCK), 0, st, *db, q, p.K1, p.K2);
    return hipGetLastError() == hipSuccess ? LSIM_OK : LSIM_E_HIP;
}
#endif
