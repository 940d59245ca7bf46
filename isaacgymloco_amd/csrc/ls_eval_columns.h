// ls_eval_columns.h -- caller-supplied per-env columns into the evaluator's groups (include/lsim.h, lsim_eval_columns): per group and column the
// sum, the sum of squares and the non-finite count of values[env][column], under the guarantees of lsim_k_eval -- 2^-32 fixed-point int64 words,
// integer atomics only (any order of waves gives the same bits), one launch, no host synchronisation.
//
// Self-contained like ls_eval.h (which it includes for the evaluator's state layout, ls_eval_fix / ls_eval_finite, the block's slot hash and the
// LDS / global add helpers): tests/emu/emu_eval_columns.cpp compiles this file with g++ under LS_EMU and runs the same per-env / per-block code.
//
// Shape of the launch (lsim_k_eval_columns): blocks of LS_EVAL_BLOCK = 256 lanes, lane = env, no trace block.
//   1. ls_evc_env: the lane reads reset_buf[env], its latched group (READ ONLY: lsim_k_eval of the same env-step, earlier on the stream, owns the
//      state) and its row of `values`, and forms its 1 + 3 num_cols addends.
//   2. ls_eval_slot: the block's distinct groups get slots of an LDS table (the 256-entry open-addressing hash of ls_eval.h).
//   3. ls_evc_lane_add: LDS 64-bit integer adds into the slot's words (rows of LS_EVC_WORDS words whatever num_cols is).
//   4. ls_evc_flush_one: one global integer atomic per (block, slot, nonzero word).
#pragma once
#include "ls_eval.h"

#define LS_EVC_WORDS (1 + LSIM_EVAL_COL_WORDS * LSIM_EVAL_MAX_COLUMNS)      // the widest row: 19 words

struct LsEvcAdd {
    int group;                  // latched group, or -1: the env contributes nothing
    long long w[LS_EVC_WORDS];  // [samples | sum_0, sq_0, nonfinite_0 | sum_1, ...]
};

// the evaluator's latched groups inside lsim_eval.state (ls_eval_state is the one statement of that layout)
LS_EV_FN const int* ls_evc_group1(const lsim_eval_columns& c) {
    lsim_eval e = {};
    e.state = (void*)c.state;
    e.num_envs = (int32_t)c.num_envs;
    return ls_eval_state(e).group1;
}

// step 1 of the launch for one env: lsim.h states the semantics
LS_EV_FN void ls_evc_env(const lsim_eval_columns& c, const int* group1, int env, LsEvcAdd& out) {
    const int g1 = group1[env];
    out.group = -1;
    if (c.reset_buf[env] != 0 || g1 <= 0 || g1 - 1 >= c.num_groups) return;
    out.group = g1 - 1;
    out.w[0] = 1;
    const float* row = c.values + (size_t)env * (size_t)c.ld;
#pragma unroll
    for (int k = 0; k < LSIM_EVAL_MAX_COLUMNS; ++k) {
        long long sum = 0, sq = 0, bad = 0;
        if (k < c.num_cols) {
            const float v = row[k];
            if (ls_eval_finite(v)) {
                sum = ls_eval_fix(v);
                sq = ls_eval_fix(v * v);       // one fp32 multiply; an overflowing square is +inf and adds the clamp
            } else {
                bad = 1;
            }
        }
        out.w[1 + LSIM_EVAL_COL_WORDS * k] = sum;
        out.w[2 + LSIM_EVAL_COL_WORDS * k] = sq;
        out.w[3 + LSIM_EVAL_COL_WORDS * k] = bad;
    }
}

// ---- the block's table: keys[LS_EVAL_BLOCK] (group + 1, 0 = free), acc[LS_EVAL_BLOCK][LS_EVC_WORDS]
LS_EV_FN void ls_evc_lane_add(long long* acc, int slot, const LsEvcAdd& a) {
    long long* row = acc + slot * LS_EVC_WORDS;
#pragma unroll
    for (int k = 0; k < LS_EVC_WORDS; ++k)
        if (a.w[k] != 0) ls_eval_lds_add(row + k, a.w[k]);
}
// idx in [0, LS_EVAL_BLOCK * LS_EVC_WORDS): one word of one slot to the global table (rows of 1 + 3 num_cols words there)
LS_EV_FN void ls_evc_flush_one(const lsim_eval_columns& c, const int* keys, const long long* acc, int idx) {
    const int slot = idx / LS_EVC_WORDS, k = idx - slot * LS_EVC_WORDS;
    const int g1 = keys[slot], width = 1 + LSIM_EVAL_COL_WORDS * c.num_cols;
    const long long v = acc[idx];
    if (g1 == 0 || v == 0 || k >= width) return;
    ls_eval_glb_add(c.table + (size_t)(g1 - 1) * (size_t)width + k, v);
}

// ---- host side: argument checks shared by the library and the CPU shim (no launch happens before they pass)
static inline int ls_evc_sizes(int num_groups, int num_cols, size_t* table_bytes) {
    if (!table_bytes || num_groups < 1 || num_groups > LSIM_EVAL_MAX_GROUPS || num_cols < 1 || num_cols > LSIM_EVAL_MAX_COLUMNS) return LSIM_E_INVALID;
    *table_bytes = (size_t)num_groups * (size_t)(1 + LSIM_EVAL_COL_WORDS * num_cols) * sizeof(int64_t);
    return LSIM_OK;
}
static inline int ls_evc_validate(const lsim_eval_columns* c) {
    if (!c) return LSIM_E_INVALID;
    if (ls_eval_check_sizes(c->num_envs, c->num_groups, 0, 1) != LSIM_OK) return LSIM_E_INVALID;
    if (c->num_cols < 1 || c->num_cols > LSIM_EVAL_MAX_COLUMNS || c->ld < c->num_cols) return LSIM_E_INVALID;
    if (!ls_eval_aligned(c->state, 16) || !c->reset_buf || !ls_eval_aligned(c->values, 4) || !ls_eval_aligned(c->table, 8)) return LSIM_E_INVALID;
    return LSIM_OK;
}

#if defined(__HIPCC__) && !defined(LS_EMU)
__global__ __launch_bounds__(LS_EVAL_BLOCK) void lsim_k_eval_columns(const lsim_eval_columns c) {
    __shared__ int keys[LS_EVAL_BLOCK];
    __shared__ long long acc[LS_EVAL_BLOCK * LS_EVC_WORDS];
    const int lane = (int)threadIdx.x;
    keys[lane] = 0;
#pragma unroll
    for (int k = 0; k < LS_EVC_WORDS; ++k) acc[k * LS_EVAL_BLOCK + lane] = 0;
    __syncthreads();
    const long long env = (long long)blockIdx.x * LS_EVAL_BLOCK + lane;
    if (env < c.num_envs) {
        LsEvcAdd a;
        ls_evc_env(c, ls_evc_group1(c), (int)env, a);
        if (a.group >= 0) {
            const int slot = ls_eval_slot(keys, a.group);
            if (slot >= 0) ls_evc_lane_add(acc, slot, a);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < LS_EVC_WORDS; ++k) ls_evc_flush_one(c, keys, acc, k * LS_EVAL_BLOCK + lane);
}

extern "C" int lsim_eval_columns_sizes(int num_groups, int num_cols, size_t* table_bytes) { return ls_evc_sizes(num_groups, num_cols, table_bytes); }
extern "C" int lsim_eval_columns_clear(const lsim_eval_columns* c, void* stream) {
    const int rc = ls_evc_validate(c);
    if (rc != LSIM_OK) return rc;
    size_t tb;
    (void)ls_evc_sizes(c->num_groups, c->num_cols, &tb);
    return hipMemsetAsync(c->table, 0, tb, (hipStream_t)stream) == hipSuccess ? LSIM_OK : LSIM_E_HIP;
}
extern "C" int lsim_eval_columns_accumulate(const lsim_eval_columns* c, void* stream) {
    const int rc = ls_evc_validate(c);
    if (rc != LSIM_OK) return rc;
    const int blocks = (int)((c->num_envs + LS_EVAL_BLOCK - 1) / LS_EVAL_BLOCK);
    hipLaunchKernelGGL(lsim_k_eval_columns, dim3(blocks), dim3(LS_EVAL_BLOCK), 0, (hipStream_t)stream, *c);
    return hipGetLastError() == hipSuccess ? LSIM_OK : LSIM_E_HIP;
}
#endif
