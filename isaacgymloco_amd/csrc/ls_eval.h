// ls_eval.h -- device-side policy evaluation (include/lsim.h, lsim_eval): per-group metric sums and the state trace ring, one launch per env-step.
//
// Self-contained on purpose (only lsim.h and the C library): the evaluator works on the raw pointers of an lsim_eval, so tests/emu/emu_eval.cpp
// compiles this file with g++ under LS_EMU and runs the same per-env / per-block code over plain arrays.
//
// Shape of the launch (lsim_k_eval, lsim_hip.hip): blocks of LS_EVAL_BLOCK = 256 lanes, lane = env; the last block of the grid is the trace block.
//   1. ls_eval_env: the lane reads its env's rows (16-byte loads for the 48- / 96- / 16-byte rows), updates the evaluator's per-env state and
//      forms its LSIM_EVAL_WORDS addends (int64, already fixed point) for the group it latched.
//   2. ls_eval_slot: the block's groups get slots of an LDS table through a 256-entry open-addressing hash (LDS compare-and-swap).  Envs of one
//      block are interleaved over robots and terrain columns, so a block touches many groups: a slot per DISTINCT group of the block (at most
//      256, so the table never fills), not a dense [num_groups] array (4096 groups x 18 words would not fit).
//   3. ls_eval_lane_add: LDS 64-bit integer adds / max into the slot's words.
//   4. ls_eval_flush_one: one global integer atomic per (block, group touched, nonzero word).  Integer sums: any order gives the same bits.
//   trace block: ls_eval_trace_one per (trace env, column), coalesced f32 stores; then lane 0 advances the device-side launch counter (nobody else
//   reads it in this launch).
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/lsim.h"

#if defined(LS_EMU) || !defined(__HIPCC__)
#define LS_EV_FN static inline
#else
#define LS_EV_FN __device__ __forceinline__
#endif
#if defined(__HIPCC__) && !defined(LS_EMU)
#define LS_EV_HD __host__ __device__ static inline
#else
#define LS_EV_HD static inline
#endif

#define LS_EVAL_BLOCK 256
#define LS_EVAL_STATE_HEADER 64     // bytes in front of the per-env arrays: [0] int64 launch counter

struct LsEvalF4 { float x, y, z, w; };

// the evaluator's per-env state inside lsim_eval.state: SoA, every array 16-byte aligned
struct LsEvalState {
    long long* counter;      // [1]  launches since lsim_eval_clear
    long long* ret;          // [N]  sum of fix(rew) of the running episode
    LsEvalF4* pos;           // [N]  start x, y, last pre-reset x, y
    int* group1;             // [N]  latched group + 1 (0: none yet)
    int* length;             // [N]  env-steps of the running episode
};
LS_EV_HD size_t ls_eval_up16(size_t n) { return (n + 15) & ~(size_t)15; }
LS_EV_HD size_t ls_eval_state_bytes(long long n) { return LS_EVAL_STATE_HEADER + ls_eval_up16(8 * (size_t)n) + 16 * (size_t)n + 2 * ls_eval_up16(4 * (size_t)n); }
LS_EV_FN LsEvalState ls_eval_state(const lsim_eval& e) {
    char* p = (char*)e.state;
    const size_t n = (size_t)e.num_envs;
    LsEvalState s;
    s.counter = (long long*)p; p += LS_EVAL_STATE_HEADER;
    s.ret = (long long*)p; p += ls_eval_up16(8 * n);
    s.pos = (LsEvalF4*)p; p += 16 * n;
    s.group1 = (int*)p; p += ls_eval_up16(4 * n);
    s.length = (int*)p;
    return s;
}

// one addend in 2^-32 fixed point, clamped to +-2^20 (the scaling by a power of two is exact in fp32, so the word is the fp32 value itself up to
// the rounding of magnitudes below 2^-9); a non-finite value is not converted (ls_eval_finite)
LS_EV_FN bool ls_eval_finite(float v) { return fabsf(v) <= 3.402823466e38f; }
LS_EV_FN long long ls_eval_fix(float v) { return (long long)llrintf(fminf(fmaxf(v, -1048576.0f), 1048576.0f) * 4294967296.0f); }

LS_EV_FN int ls_eval_clampi(long long v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : (int)v); }
LS_EV_FN int ls_eval_group(const lsim_eval& e, int env) {
    const int r = (e.group_by & LSIM_EVAL_BY_ROBOT) && e.robot_ids ? ls_eval_clampi(e.robot_ids[env], e.num_robots) : 0;
    const int nt = (e.group_by & LSIM_EVAL_BY_TYPE) ? e.num_types : 1, nl = (e.group_by & LSIM_EVAL_BY_LEVEL) ? e.num_levels : 1;
    const int t = ls_eval_clampi(e.terrain_types[env], nt), l = ls_eval_clampi(e.terrain_levels[env], nl);
    return ls_eval_clampi(((long long)r * nt + t) * nl + l, e.num_groups);
}

struct LsEvalAdd {
    int group;
    long long w[LSIM_EVAL_WORDS];
};

// `value` in fixed point into `word`, or one more non-finite addend
#define LS_EV_ADD(word, value) do { const float v_ = (value); if (ls_eval_finite(v_)) word = ls_eval_fix(v_); else nonfinite += 1; } while (0)

// step 1 of the launch for one env: lsim.h states the semantics
LS_EV_FN void ls_eval_env(const lsim_eval& e, const LsEvalState& st, int env, LsEvalAdd& out) {
    const bool reset = e.reset_buf[env] != 0, tout = e.time_out_buf[env] != 0;
    const float px = e.root_states[13 * env], py = e.root_states[13 * env + 1];
    int g1 = st.group1[env];
    LsEvalF4 pos = st.pos[env];
    long long ret = st.ret[env];
    int len = st.length[env];
    if (g1 == 0) {              // first launch after lsim_eval_clear
        g1 = ls_eval_group(e, env) + 1;
        pos.x = pos.z = px; pos.y = pos.w = py;
    }
    out.group = g1 - 1;
    long long nonfinite = 0, w_lin = 0, w_lin2 = 0, w_yaw = 0, w_yaw2 = 0, w_power = 0, w_tsq = 0, w_rate = 0, w_peak = 0, w_ret = 0, w_dist = 0, w_rew = 0;
    int sat = 0, feet = 0;
    LS_EV_ADD(w_rew, e.rew[env]);
    ret += w_rew;
    len += 1;
    if (!reset) {
        const LsEvalF4 cmd = ((const LsEvalF4*)e.commands)[env];
        const float dx = cmd.x - e.base_lin_vel[3 * env], dy = cmd.y - e.base_lin_vel[3 * env + 1];
        const float e2 = dx * dx + dy * dy;
        LS_EV_ADD(w_lin, sqrtf(e2));
        LS_EV_ADD(w_lin2, e2);
        const float yw = fabsf(cmd.z - e.base_ang_vel[3 * env + 2]);
        LS_EV_ADD(w_yaw, yw);
        LS_EV_ADD(w_yaw2, yw * yw);
        float power = 0.0f, tsq = 0.0f, rate = 0.0f, peak = 0.0f;
        bool peak_nan = false;
#pragma unroll
        for (int q = 0; q < 3; ++q) {       // 4 joints per 16-byte load
            const LsEvalF4 tau = ((const LsEvalF4*)e.torques)[3 * env + q], lim = ((const LsEvalF4*)e.torque_limits)[3 * env + q];
            const LsEvalF4 a = ((const LsEvalF4*)e.actions)[3 * env + q], al = ((const LsEvalF4*)e.last_actions)[3 * env + q];
            const LsEvalF4 d0 = ((const LsEvalF4*)e.dof_state)[6 * env + 2 * q], d1 = ((const LsEvalF4*)e.dof_state)[6 * env + 2 * q + 1];   // (pos, vel) pairs
#define LS_EV_JOINT(t_, l_, qd_, a_, al_) do { const float da_ = (a_) - (al_), r_ = fabsf(t_) / (l_); \
                power = power + fabsf((t_) * (qd_)); tsq = tsq + (t_) * (t_); rate = rate + da_ * da_; sat += fabsf(t_) >= 0.98f * (l_) ? 1 : 0; \
                peak_nan = peak_nan || r_ != r_; peak = fmaxf(peak, r_); } while (0)       /* fmaxf drops a NaN operand: peak_nan carries it */
            LS_EV_JOINT(tau.x, lim.x, d0.y, a.x, al.x);
            LS_EV_JOINT(tau.y, lim.y, d0.w, a.y, al.y);
            LS_EV_JOINT(tau.z, lim.z, d1.y, a.z, al.z);
            LS_EV_JOINT(tau.w, lim.w, d1.w, a.w, al.w);
#undef LS_EV_JOINT
        }
        LS_EV_ADD(w_power, power);
        LS_EV_ADD(w_tsq, tsq);
        LS_EV_ADD(w_rate, rate);
        if (peak_nan) nonfinite += 1; else LS_EV_ADD(w_peak, peak);
        const uint32_t cf = ((const uint32_t*)e.contact_filt)[env];
        feet = ((cf & 0xffu) != 0) + ((cf & 0xff00u) != 0) + ((cf & 0xff0000u) != 0) + ((cf & 0xff000000u) != 0);
        pos.z = px; pos.w = py;
    } else {
        w_ret = ret;
        const float ddx = pos.z - pos.x, ddy = pos.w - pos.y;
        LS_EV_ADD(w_dist, sqrtf(ddx * ddx + ddy * ddy));
    }
    out.w[LSIM_EVAL_W_SAMPLES] = reset ? 0 : 1;
    out.w[LSIM_EVAL_W_LIN_ERR] = w_lin;
    out.w[LSIM_EVAL_W_LIN_ERR_SQ] = w_lin2;
    out.w[LSIM_EVAL_W_YAW_ERR] = w_yaw;
    out.w[LSIM_EVAL_W_YAW_ERR_SQ] = w_yaw2;
    out.w[LSIM_EVAL_W_POWER] = w_power;
    out.w[LSIM_EVAL_W_TORQUE_SQ] = w_tsq;
    out.w[LSIM_EVAL_W_ACTION_RATE] = w_rate;
    out.w[LSIM_EVAL_W_FEET_CONTACT] = feet;
    out.w[LSIM_EVAL_W_TORQUE_SAT] = sat;
    out.w[LSIM_EVAL_W_PEAK_TORQUE_RATIO] = w_peak;
    out.w[LSIM_EVAL_W_EPISODES] = reset ? 1 : 0;
    out.w[LSIM_EVAL_W_TIME_OUTS] = reset && tout ? 1 : 0;
    out.w[LSIM_EVAL_W_FALLS] = reset && !tout ? 1 : 0;
    out.w[LSIM_EVAL_W_RETURN] = w_ret;
    out.w[LSIM_EVAL_W_LENGTH] = reset ? len : 0;
    out.w[LSIM_EVAL_W_DISTANCE] = w_dist;
    out.w[LSIM_EVAL_W_NONFINITE] = nonfinite;
    if (reset) {
        ret = 0; len = 0;
        g1 = ls_eval_group(e, env) + 1;
        pos.x = pos.z = px; pos.y = pos.w = py;
    }
    st.group1[env] = g1;
    st.pos[env] = pos;
    st.ret[env] = ret;
    st.length[env] = len;
}

// ---- the block's table: keys[LS_EVAL_BLOCK] (group + 1, 0 = free), acc[LS_EVAL_BLOCK][LSIM_EVAL_WORDS]
#if defined(LS_EMU) || !defined(__HIPCC__)
LS_EV_FN int ls_eval_cas(int* p, int expect, int v) { const int o = *p; if (o == expect) *p = v; return o; }
LS_EV_FN void ls_eval_lds_add(long long* p, long long v) { *p += v; }
LS_EV_FN void ls_eval_lds_max(long long* p, long long v) { if (v > *p) *p = v; }
LS_EV_FN void ls_eval_glb_add(int64_t* p, long long v) { *p += v; }
LS_EV_FN void ls_eval_glb_max(int64_t* p, long long v) { if (v > *p) *p = v; }
#else
LS_EV_FN int ls_eval_cas(int* p, int expect, int v) { return atomicCAS(p, expect, v); }
LS_EV_FN void ls_eval_lds_add(long long* p, long long v) { (void)atomicAdd((unsigned long long*)p, (unsigned long long)v); }
LS_EV_FN void ls_eval_lds_max(long long* p, long long v) { (void)atomicMax((unsigned long long*)p, (unsigned long long)v); }     // the words are >= 0
LS_EV_FN void ls_eval_glb_add(int64_t* p, long long v) { (void)atomicAdd((unsigned long long*)p, (unsigned long long)v); }
LS_EV_FN void ls_eval_glb_max(int64_t* p, long long v) { (void)atomicMax((unsigned long long*)p, (unsigned long long)v); }
#endif

// the slot of `group` in the block's table: at most LS_EVAL_BLOCK distinct groups per block, so the probe always ends
LS_EV_FN int ls_eval_slot(int* keys, int group) {
    int s = (int)(((unsigned)group * 2654435761u) >> 24) & (LS_EVAL_BLOCK - 1);
    for (int probe = 0; probe < LS_EVAL_BLOCK; ++probe) {
        const int o = ls_eval_cas(keys + s, 0, group + 1);
        if (o == 0 || o == group + 1) return s;
        s = (s + 1) & (LS_EVAL_BLOCK - 1);
    }
    return -1;      // unreachable
}
LS_EV_FN void ls_eval_lane_add(long long* acc, int slot, const LsEvalAdd& a) {
    long long* row = acc + slot * LSIM_EVAL_WORDS;
#pragma unroll
    for (int k = 0; k < LSIM_EVAL_WORDS; ++k) {
        if (a.w[k] == 0) continue;
        if (k == LSIM_EVAL_W_PEAK_TORQUE_RATIO) ls_eval_lds_max(row + k, a.w[k]); else ls_eval_lds_add(row + k, a.w[k]);
    }
}
// idx in [0, LS_EVAL_BLOCK * LSIM_EVAL_WORDS): one word of one slot to the global table
LS_EV_FN void ls_eval_flush_one(const lsim_eval& e, const int* keys, const long long* acc, int idx) {
    const int slot = idx / LSIM_EVAL_WORDS, k = idx - slot * LSIM_EVAL_WORDS;
    const int g1 = keys[slot];
    const long long v = acc[idx];
    if (g1 == 0 || v == 0) return;
    int64_t* dst = e.table + (size_t)(g1 - 1) * LSIM_EVAL_WORDS + k;
    if (k == LSIM_EVAL_W_PEAK_TORQUE_RATIO) ls_eval_glb_max(dst, v); else ls_eval_glb_add(dst, v);
}

// ---- trace ring: column c of trace env k at launch t
LS_EV_FN float ls_eval_trace_value(const lsim_eval& e, int env, int c) {
    if (c < LSIM_EVAL_TR_DOF_POS) return e.actions[12 * env + c] * e.action_scale[12 * env + c] + e.default_dof_pos[12 * env + c];
    if (c < LSIM_EVAL_TR_DOF_VEL) return e.dof_state[24 * env + 2 * (c - LSIM_EVAL_TR_DOF_POS)];
    if (c < LSIM_EVAL_TR_TORQUES) return e.dof_state[24 * env + 2 * (c - LSIM_EVAL_TR_DOF_VEL) + 1];
    if (c < LSIM_EVAL_TR_COMMANDS) return e.torques[12 * env + c - LSIM_EVAL_TR_TORQUES];
    if (c < LSIM_EVAL_TR_BASE_LIN_VEL) return e.commands[4 * env + c - LSIM_EVAL_TR_COMMANDS];
    if (c < LSIM_EVAL_TR_BASE_ANG_VEL) return e.base_lin_vel[3 * env + c - LSIM_EVAL_TR_BASE_LIN_VEL];
    if (c < LSIM_EVAL_TR_CONTACT_FORCES_Z) return e.base_ang_vel[3 * env + c - LSIM_EVAL_TR_BASE_ANG_VEL];
    if (c < LSIM_EVAL_TR_ROOT_POS) {
        const int f = c - LSIM_EVAL_TR_CONTACT_FORCES_Z;      // selects, not an indexed read of the by-value argument (that costs scratch)
        const int body = f == 0 ? e.feet_bodies[0] : (f == 1 ? e.feet_bodies[1] : (f == 2 ? e.feet_bodies[2] : e.feet_bodies[3]));
        return e.contact_forces[(LSIM_NUM_BODIES * env + body) * 3 + 2];
    }
    if (c < LSIM_EVAL_TR_REW) return e.root_states[13 * env + c - LSIM_EVAL_TR_ROOT_POS];      // position 0..2, quaternion 3..6
    if (c == LSIM_EVAL_TR_REW) return e.rew[env];
    return e.reset_buf[env] ? 1.0f : 0.0f;
}
LS_EV_FN void ls_eval_trace_one(const lsim_eval& e, long long t, int idx) {
    const int k = idx / LSIM_EVAL_TRACE_DIM, c = idx - k * LSIM_EVAL_TRACE_DIM;
    const size_t row = (size_t)(t % e.trace_capacity);
    e.trace[(row * (size_t)e.num_trace_envs + (size_t)k) * LSIM_EVAL_TRACE_DIM + c] = ls_eval_trace_value(e, e.trace_envs[k], c);
}

// ---- host side: argument checks shared by the library and the CPU shim (no launch happens before they pass)
static inline int ls_eval_check_sizes(long long num_envs, int num_groups, int num_trace_envs, int trace_capacity) {
    if (num_envs < 1 || num_envs > 0x7fffffff / 32) return LSIM_E_INVALID;
    if (num_groups < 1 || num_groups > LSIM_EVAL_MAX_GROUPS) return LSIM_E_INVALID;
    if (num_trace_envs < 0 || num_trace_envs > LSIM_EVAL_MAX_TRACE_ENVS || trace_capacity < 1) return LSIM_E_INVALID;
    return LSIM_OK;
}
static inline int ls_eval_sizes(long long num_envs, int num_groups, int num_trace_envs, int trace_capacity, size_t* state_bytes, size_t* table_bytes,
                                size_t* trace_bytes) {
    if (!state_bytes || !table_bytes || !trace_bytes) return LSIM_E_INVALID;
    if (ls_eval_check_sizes(num_envs, num_groups, num_trace_envs, trace_capacity) != LSIM_OK) return LSIM_E_INVALID;
    *state_bytes = ls_eval_state_bytes(num_envs);
    *table_bytes = (size_t)num_groups * LSIM_EVAL_WORDS * sizeof(int64_t);
    *trace_bytes = (size_t)trace_capacity * (size_t)num_trace_envs * LSIM_EVAL_TRACE_DIM * sizeof(float);
    return LSIM_OK;
}
static inline bool ls_eval_aligned(const void* p, size_t a) { return p && ((uintptr_t)p & (a - 1)) == 0; }
static inline int ls_eval_validate(const lsim_eval* e) {
    if (!e) return LSIM_E_INVALID;
    if (ls_eval_check_sizes(e->num_envs, e->num_groups, e->num_trace_envs, e->trace_capacity) != LSIM_OK) return LSIM_E_INVALID;
    if (e->num_robots < 1 || e->num_robots > LSIM_MAX_ROBOTS || e->num_types < 1 || e->num_types > LSIM_TERRAIN_TYPES_MAX ||
        e->num_levels < 1 || e->num_levels > LSIM_TERRAIN_LEVELS_MAX) return LSIM_E_INVALID;
    if (e->group_by & ~(LSIM_EVAL_BY_ROBOT | LSIM_EVAL_BY_TYPE | LSIM_EVAL_BY_LEVEL)) return LSIM_E_INVALID;
    const int groups = ((e->group_by & LSIM_EVAL_BY_ROBOT) ? e->num_robots : 1) * ((e->group_by & LSIM_EVAL_BY_TYPE) ? e->num_types : 1) *
                       ((e->group_by & LSIM_EVAL_BY_LEVEL) ? e->num_levels : 1);
    if (groups != e->num_groups) return LSIM_E_INVALID;
    const void* a16[] = {e->commands, e->dof_state, e->torques, e->actions, e->last_actions, e->torque_limits, e->default_dof_pos, e->action_scale, e->state};
    for (const void* p : a16) if (!ls_eval_aligned(p, 16)) return LSIM_E_INVALID;
    const void* a8[] = {e->terrain_types, e->terrain_levels, e->table};
    for (const void* p : a8) if (!ls_eval_aligned(p, 8)) return LSIM_E_INVALID;
    const void* a4[] = {e->rew, e->base_lin_vel, e->base_ang_vel, e->root_states, e->contact_filt, e->contact_forces};
    for (const void* p : a4) if (!ls_eval_aligned(p, 4)) return LSIM_E_INVALID;
    if (!e->reset_buf || !e->time_out_buf) return LSIM_E_INVALID;
    if (e->num_trace_envs > 0 && !ls_eval_aligned(e->trace, 4)) return LSIM_E_INVALID;
    for (int k = 0; k < e->num_trace_envs; ++k) if (e->trace_envs[k] < 0 || e->trace_envs[k] >= e->num_envs) return LSIM_E_INVALID;
    for (int k = 0; k < LSIM_NUM_LEGS; ++k) if (e->feet_bodies[k] < 0 || e->feet_bodies[k] >= LSIM_NUM_BODIES) return LSIM_E_INVALID;
    return LSIM_OK;
}

#if defined(__HIPCC__) && !defined(LS_EMU)
__global__ __launch_bounds__(LS_EVAL_BLOCK) void lsim_k_eval(const lsim_eval e) {
    __shared__ int keys[LS_EVAL_BLOCK];
    __shared__ long long acc[LS_EVAL_BLOCK * LSIM_EVAL_WORDS];
    const int lane = (int)threadIdx.x;
    const LsEvalState st = ls_eval_state(e);
    if (blockIdx.x + 1 == gridDim.x) {          // the trace block: also the only reader and the writer of the launch counter
        const long long t = *st.counter;
        for (int idx = lane; idx < e.num_trace_envs * LSIM_EVAL_TRACE_DIM; idx += LS_EVAL_BLOCK) ls_eval_trace_one(e, t, idx);
        __syncthreads();
        if (lane == 0) *st.counter = t + 1;
        return;
    }
    keys[lane] = 0;
#pragma unroll
    for (int k = 0; k < LSIM_EVAL_WORDS; ++k) acc[k * LS_EVAL_BLOCK + lane] = 0;
    __syncthreads();
    const int env = (int)blockIdx.x * LS_EVAL_BLOCK + lane;
    if (env < e.num_envs) {
        LsEvalAdd a;
        ls_eval_env(e, st, env, a);
        const int slot = ls_eval_slot(keys, a.group);
        if (slot >= 0) ls_eval_lane_add(acc, slot, a);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < LSIM_EVAL_WORDS; ++k) ls_eval_flush_one(e, keys, acc, k * LS_EVAL_BLOCK + lane);
}

extern "C" int lsim_eval_sizes(int64_t num_envs, int num_groups, int num_trace_envs, int trace_capacity, size_t* state_bytes, size_t* table_bytes,
                               size_t* trace_bytes) {
    return ls_eval_sizes(num_envs, num_groups, num_trace_envs, trace_capacity, state_bytes, table_bytes, trace_bytes);
}
extern "C" int lsim_eval_clear(const lsim_eval* e, void* stream) {
    const int rc = ls_eval_validate(e);
    if (rc != LSIM_OK) return rc;
    size_t sb, tb, rb;
    (void)ls_eval_sizes(e->num_envs, e->num_groups, e->num_trace_envs, e->trace_capacity, &sb, &tb, &rb);
    if (hipMemsetAsync(e->state, 0, sb, (hipStream_t)stream) != hipSuccess) return LSIM_E_HIP;
    if (hipMemsetAsync(e->table, 0, tb, (hipStream_t)stream) != hipSuccess) return LSIM_E_HIP;
    if (rb && hipMemsetAsync(e->trace, 0, rb, (hipStream_t)stream) != hipSuccess) return LSIM_E_HIP;
    return LSIM_OK;
}
extern "C" int lsim_eval_accumulate(const lsim_eval* e, void* stream) {
    const int rc = ls_eval_validate(e);
    if (rc != LSIM_OK) return rc;
    const int blocks = (e->num_envs + LS_EVAL_BLOCK - 1) / LS_EVAL_BLOCK + 1;
    hipLaunchKernelGGL(lsim_k_eval, dim3(blocks), dim3(LS_EVAL_BLOCK), 0, (hipStream_t)stream, *e);
    return hipGetLastError() == hipSuccess ? LSIM_OK : LSIM_E_HIP;
}
#endif
