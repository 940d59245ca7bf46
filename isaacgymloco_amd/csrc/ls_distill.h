// ls_distill.h -- the loss joint of vision distillation (include/lsim.h, lsim_distill_loss): the squared error between a minibatch's action
// means and the teacher's means of the same transitions, its gradient and its per-workgroup sums, one launch.  lsim.h states every rule;
// this file is that text in code.
//
// Self-contained (lsim.h and the C library): tests/emu/emu_distill.cpp compiles this file with g++ under LS_EMU and runs the same validation,
// the same chunking and the same per-item functions over plain arrays, lanes and waves looped in the order of the launch.
//
// Shape of the launch (lsim_k_distill_loss): a FIXED grid of LSIM_DISTILL_PARTIALS workgroups of LS_DL_BLOCK = 256 lanes, whatever `batch`.
//   Workgroup p owns the rows [p * chunk, min(batch, (p + 1) * chunk)), chunk = ceil(batch / LSIM_DISTILL_PARTIALS): contiguous, so that a
//   wave's loads of mu and its stores of g are contiguous too.  The rows of a chunk are cut into items -- one column of one row on the scalar
//   path, four consecutive columns (one 128-bit load of mu, one of target, one store of g) on the vector path -- and lane l takes the items
//   l, l + 256, ... of its workgroup's chunk in ascending order, adding d * d of each to ITS OWN fp32 sum.  A pass of the grid therefore
//   covers LSIM_DISTILL_PARTIALS * 256 items; a larger minibatch makes every lane loop.  index[row] is one dword load per item (the lanes of
//   a row read the same word: a broadcast); a row whose index lies outside 0 .. target_rows - 1 takes the branch that stores +0.0f and reads
//   neither mu's value into the sum nor target at all.
//   Then the sums meet in a fixed order: a butterfly over the wave's 64 lanes (__shfl_xor, 6 steps, every lane ends with the same value), the
//   four waves' values through 16 bytes of LDS and one barrier, lane 0 adds them in ascending wave order and stores partial[p].  No atomic,
//   no exchange between workgroups, no counter: every bit written is a function of the inputs and of these two constants alone, so two
//   launches agree bit for bit.  An idle workgroup (p * chunk >= batch) runs the same code over no items and stores 0.
//   Vector path: actions, mu_stride, target_stride and g_stride multiples of 4 and mu, target and g 16-byte aligned (every row then starts
//   on a 16-byte boundary); decided on the host, a template parameter of the kernel.  The columns from `actions` to a stride are never
//   loaded or stored on either path.
//   The minibatch of the default configuration (24 576 rows of 12 actions) moves 3.5 MB: the launch is bound by its launch cost, not by
//   bandwidth, and nothing here is tuned beyond coalescing.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "../../include/lsim.h"

#if defined(LS_EMU) || !defined(__HIPCC__)
#define LS_DL_FN static inline
#else
#define LS_DL_FN __device__ __forceinline__
#endif

#define LS_DL_BLOCK 256
#define LS_DL_WAVES (LS_DL_BLOCK / 64)

// rows per workgroup
LS_DL_FN long long ls_dl_chunk(const lsim_distill_loss_t& dl) {
    return ((long long)dl.batch + LSIM_DISTILL_PARTIALS - 1) / LSIM_DISTILL_PARTIALS;
}
// the row of target that minibatch row `row` is compared with, or -1: the row carries no loss
LS_DL_FN long long ls_dl_target_row(const lsim_distill_loss_t& dl, long long row) {
    const int32_t t = dl.index[row];
    return t >= 0 && t < dl.target_rows ? (long long)t : -1;
}
// scalar item: column `col` of `row` -> d * d (0 for a skipped row); g[row][col] is written
LS_DL_FN float ls_dl_item(const lsim_distill_loss_t& dl, long long row, int col) {
    float* g = dl.g + (size_t)row * (size_t)dl.g_stride + (size_t)col;
    const long long t = ls_dl_target_row(dl, row);
    if (t < 0) {
        *g = 0.0f;
        return 0.0f;
    }
    const float d = dl.mu[(size_t)row * (size_t)dl.mu_stride + (size_t)col] - dl.target[(size_t)t * (size_t)dl.target_stride + (size_t)col];
    *g = d * dl.scale;
    return d * d;
}
// vector item: columns 4 q .. 4 q + 3 of `row` -> the sum of their d * d in ascending column order; the four g are written
LS_DL_FN float ls_dl_item4(const lsim_distill_loss_t& dl, long long row, int q) {
    float* g = dl.g + (size_t)row * (size_t)dl.g_stride + (size_t)4 * (size_t)q;
    const long long t = ls_dl_target_row(dl, row);
#if defined(__HIPCC__) && !defined(LS_EMU)
    if (t < 0) {
        *(float4*)g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return 0.0f;
    }
    const float4 m = *(const float4*)(dl.mu + (size_t)row * (size_t)dl.mu_stride + (size_t)4 * (size_t)q);
    const float4 y = *(const float4*)(dl.target + (size_t)t * (size_t)dl.target_stride + (size_t)4 * (size_t)q);
    const float d0 = m.x - y.x, d1 = m.y - y.y, d2 = m.z - y.z, d3 = m.w - y.w;
    *(float4*)g = make_float4(d0 * dl.scale, d1 * dl.scale, d2 * dl.scale, d3 * dl.scale);
    return ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
#else
    if (t < 0) {
        for (int k = 0; k < 4; ++k) g[k] = 0.0f;
        return 0.0f;
    }
    const float* m = dl.mu + (size_t)row * (size_t)dl.mu_stride + (size_t)4 * (size_t)q;
    const float* y = dl.target + (size_t)t * (size_t)dl.target_stride + (size_t)4 * (size_t)q;
    float d[4];
    for (int k = 0; k < 4; ++k) {
        d[k] = m[k] - y[k];
        g[k] = d[k] * dl.scale;
    }
    return ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3];
#endif
}
// lane `lane` of workgroup `p`: its own sum over the items lane, lane + 256, ... of the workgroup's chunk
template <bool VEC>
LS_DL_FN float ls_dl_lane(const lsim_distill_loss_t& dl, int p, int lane) {
    const long long chunk = ls_dl_chunk(dl), first = (long long)p * chunk;
    long long rows = (long long)dl.batch - first;
    if (rows > chunk) rows = chunk;
    const int per_row = VEC ? dl.actions >> 2 : dl.actions;
    float acc = 0.0f;
    for (long long i = lane; i < rows * per_row; i += LS_DL_BLOCK) {       // rows <= 0 for an idle workgroup: no item
        const long long r = i / per_row;
        const int c = (int)(i - r * per_row);
        acc = acc + (VEC ? ls_dl_item4(dl, first + r, c) : ls_dl_item(dl, first + r, c));
    }
    return acc;
}

static inline bool ls_dl_aligned(const void* p, size_t a) { return p && ((uintptr_t)p & (a - 1)) == 0; }
static inline bool ls_dl_host_finite(float v) { return v == v && v <= 3.402823466e38f && v >= -3.402823466e38f; }
static inline int ls_dl_validate(const lsim_distill_loss_t* dl) {
    if (!dl) return LSIM_E_INVALID;
    if (!ls_dl_aligned(dl->mu, 4) || !ls_dl_aligned(dl->target, 4) || !ls_dl_aligned(dl->index, 4)) return LSIM_E_INVALID;
    if (!ls_dl_aligned(dl->g, 4) || !ls_dl_aligned(dl->partial, 4)) return LSIM_E_INVALID;
    if (dl->batch < 1 || dl->actions < 1 || dl->actions > LSIM_DISTILL_MAX_ACTIONS || dl->target_rows < 1) return LSIM_E_INVALID;
    if (dl->mu_stride < dl->actions || dl->target_stride < dl->actions || dl->g_stride < dl->actions) return LSIM_E_INVALID;
    if (!ls_dl_host_finite(dl->scale)) return LSIM_E_INVALID;
    return LSIM_OK;
}
// the 128-bit path: every row of the three float arrays starts on a 16-byte boundary and holds whole groups of four
static inline bool ls_dl_vector(const lsim_distill_loss_t& dl) {
    return ((dl.actions | dl.mu_stride | dl.target_stride | dl.g_stride) & 3) == 0 && ls_dl_aligned(dl.mu, 16) && ls_dl_aligned(dl.target, 16) &&
           ls_dl_aligned(dl.g, 16);
}

#if defined(__HIPCC__) && !defined(LS_EMU)
template <bool VEC>
__global__ __launch_bounds__(LS_DL_BLOCK) void lsim_k_distill_loss(const lsim_distill_loss_t dl) {
    __shared__ float part[LS_DL_WAVES];
    const int tid = (int)threadIdx.x;
    float acc = ls_dl_lane<VEC>(dl, (int)blockIdx.x, tid);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc = acc + __shfl_xor(acc, m, 64);
    if ((tid & 63) == 0) part[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        float sum = part[0];
#pragma unroll
        for (int w = 1; w < LS_DL_WAVES; ++w) sum = sum + part[w];
        dl.partial[blockIdx.x] = sum;
    }
}

extern "C" int lsim_distill_loss(const lsim_distill_loss_t* dl, void* stream) {
    const int rv = ls_dl_validate(dl);
    if (rv != LSIM_OK) return rv;
    if (ls_dl_vector(*dl))
        hipLaunchKernelGGL(lsim_k_distill_loss<true>, dim3(LSIM_DISTILL_PARTIALS), dim3(LS_DL_BLOCK), 0, (hipStream_t)stream, *dl);
    else
        hipLaunchKernelGGL(lsim_k_distill_loss<false>, dim3(LSIM_DISTILL_PARTIALS), dim3(LS_DL_BLOCK), 0, (hipStream_t)stream, *dl);
    return hipGetLastError() == hipSuccess ? LSIM_OK : LSIM_E_HIP;
}
#endif
