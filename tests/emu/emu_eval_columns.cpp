// TEST INFRASTRUCTURE -- CPU shim of the evaluator-columns launch (isaacgymloco_amd/csrc/ls_eval_columns.h): the same per-env / per-block functions
// the HIP kernel lsim_k_eval_columns calls, in the same order, with the lanes of a block looped and plain memory in place of LDS and atomics.  The
// entry points carry the signatures of include/lsim.h (the stream is ignored); the evaluator's own launch is tests/emu/emu_eval.cpp's.  The
// test-only emu_eval_columns_accumulate_ordered runs the loops with `order` (may be NULL), a permutation of the envs: the order in which the
// "lanes" run, to show that the table does not depend on it.
#define LS_EMU 1
#include <string.h>
#include <vector>
#include "../../isaacgymloco_amd/csrc/ls_eval_columns.h"

extern "C" int emu_eval_columns_sizes(int num_groups, int num_cols, size_t* table_bytes) { return ls_evc_sizes(num_groups, num_cols, table_bytes); }

extern "C" int emu_eval_columns_clear(const lsim_eval_columns* c, void* /*stream*/) {
    const int rc = ls_evc_validate(c);
    if (rc != LSIM_OK) return rc;
    size_t tb;
    (void)ls_evc_sizes(c->num_groups, c->num_cols, &tb);
    memset(c->table, 0, tb);
    return LSIM_OK;
}

extern "C" int emu_eval_columns_accumulate_ordered(const lsim_eval_columns* cp, const int32_t* order) {
    const int rc = ls_evc_validate(cp);
    if (rc != LSIM_OK) return rc;
    const lsim_eval_columns& c = *cp;
    const int* group1 = ls_evc_group1(c);
    std::vector<int> keys(LS_EVAL_BLOCK);
    std::vector<long long> acc((size_t)LS_EVAL_BLOCK * LS_EVC_WORDS);
    const long long blocks = (c.num_envs + LS_EVAL_BLOCK - 1) / LS_EVAL_BLOCK;
    for (long long b = 0; b < blocks; ++b) {
        std::fill(keys.begin(), keys.end(), 0);
        std::fill(acc.begin(), acc.end(), 0LL);
        for (int lane = 0; lane < LS_EVAL_BLOCK; ++lane) {
            const long long i = b * LS_EVAL_BLOCK + lane;
            if (i >= c.num_envs) continue;
            const int env = order ? order[i] : (int)i;
            LsEvcAdd a;
            ls_evc_env(c, group1, env, a);
            if (a.group < 0) continue;
            const int slot = ls_eval_slot(keys.data(), a.group);
            if (slot < 0) return LSIM_E_INVALID;
            ls_evc_lane_add(acc.data(), slot, a);
        }
        for (int idx = 0; idx < LS_EVAL_BLOCK * LS_EVC_WORDS; ++idx) ls_evc_flush_one(c, keys.data(), acc.data(), idx);
    }
    return LSIM_OK;
}

extern "C" int emu_eval_columns_accumulate(const lsim_eval_columns* c, void* /*stream*/) { return emu_eval_columns_accumulate_ordered(c, nullptr); }
