// TEST INFRASTRUCTURE -- CPU shim of the evaluator launch (isaacgymloco_amd/csrc/ls_eval.h): the same per-env / per-block functions the HIP kernel
// lsim_k_eval calls, in the same order, with the lanes of a block looped and plain memory in place of LDS and atomics.  The entry points carry
// the signatures of include/lsim.h (the stream is ignored); the test-only emu_eval_accumulate_ordered runs the same loops with `order` (may be
// NULL), a permutation of the envs: the order in which the "lanes" run, to show that the table does not depend on it.
#define LS_EMU 1
#include <string.h>
#include <vector>
#include "../../isaacgymloco_amd/csrc/ls_eval.h"

extern "C" int emu_eval_sizes(int64_t num_envs, int num_groups, int num_trace_envs, int trace_capacity, size_t* state_bytes, size_t* table_bytes,
                              size_t* trace_bytes) {
    return ls_eval_sizes(num_envs, num_groups, num_trace_envs, trace_capacity, state_bytes, table_bytes, trace_bytes);
}

extern "C" int emu_eval_clear(const lsim_eval* e, void* /*stream*/) {
    const int rc = ls_eval_validate(e);
    if (rc != LSIM_OK) return rc;
    size_t sb, tb, rb;
    (void)ls_eval_sizes(e->num_envs, e->num_groups, e->num_trace_envs, e->trace_capacity, &sb, &tb, &rb);
    memset(e->state, 0, sb);
    memset(e->table, 0, tb);
    if (rb) memset(e->trace, 0, rb);
    return LSIM_OK;
}

extern "C" int emu_eval_accumulate_ordered(const lsim_eval* ep, const int32_t* order) {
    const int rc = ls_eval_validate(ep);
    if (rc != LSIM_OK) return rc;
    const lsim_eval& e = *ep;
    const LsEvalState st = ls_eval_state(e);
    std::vector<int> keys(LS_EVAL_BLOCK);
    std::vector<long long> acc((size_t)LS_EVAL_BLOCK * LSIM_EVAL_WORDS);
    const int blocks = (e.num_envs + LS_EVAL_BLOCK - 1) / LS_EVAL_BLOCK;
    for (int b = 0; b < blocks; ++b) {
        std::fill(keys.begin(), keys.end(), 0);
        std::fill(acc.begin(), acc.end(), 0LL);
        for (int lane = 0; lane < LS_EVAL_BLOCK; ++lane) {
            const int i = b * LS_EVAL_BLOCK + lane;
            if (i >= e.num_envs) continue;
            const int env = order ? order[i] : i;
            LsEvalAdd a;
            ls_eval_env(e, st, env, a);
            const int slot = ls_eval_slot(keys.data(), a.group);
            if (slot < 0) return LSIM_E_INVALID;
            ls_eval_lane_add(acc.data(), slot, a);
        }
        for (int idx = 0; idx < LS_EVAL_BLOCK * LSIM_EVAL_WORDS; ++idx) ls_eval_flush_one(e, keys.data(), acc.data(), idx);
    }
    const long long t = *st.counter;
    for (int idx = 0; idx < e.num_trace_envs * LSIM_EVAL_TRACE_DIM; ++idx) ls_eval_trace_one(e, t, idx);
    *st.counter = t + 1;
    return LSIM_OK;
}

extern "C" int emu_eval_accumulate(const lsim_eval* e, void* /*stream*/) { return emu_eval_accumulate_ordered(e, nullptr); }
