// ls_sensor_model.h -- the sensor model (include/lsim.h, lsim_sensor_capture): the ray cast of ls_raycast.h / ls_raycast_bodies.h for the envs
// that are due on this tick only, followed per ray by noise, dropout, clipping, normalisation and the env's frame history, one launch.
//
// Self-contained like its two siblings (lsim.h, ls_raycast_bodies.h, the Philox of ls_math.h and the C library): tests/emu/emu_sensor_model.cpp
// compiles this file with g++ under LS_EMU and runs the same per-block and per-ray code over plain arrays.
//
// Shape of the launch (lsim_k_sensor_capture): lsim_k_raycast_bodies's -- blocks of 256 lanes over the rays of ONE env, lane = ray -- with
//   0. ls_sm_due first: tick, the flags and the env are the block's, episode_length[env] is one scalar load, so the test costs a few scalar
//      instructions and a block of an env that is not due ends before the forward kinematics, before it touches LDS and before any barrier.
//      With period P and stagger, P - 1 blocks in P are such empty blocks;
//   1. the prologue of lsim_k_raycast_bodies (ls_rcb_fk, ls_rcb_prim) unless the struct is of the terrain-only form, which skips it and LDS altogether;
//   2. ls_sm_raw_bodies / ls_sm_raw_terrain: ls_rcb_ray / ls_rc_ray up to their store, returning the value instead.  They are copies, not edits:
//      the two existing kernels inline the originals and their results must not move.  The casts themselves (ls_rcb_cast, ls_rc_cast) are shared;
//   3. ls_sm_store: the clean value to out, one Philox block per ray, the model, and the ray's own column of hist -- K slots hist_stride floats
//      apart, lane = consecutive r, so every slot is read and written by a wave as one coalesced 256-byte line, and no lane reads what another writes.
#pragma once
#include "ls_raycast_bodies.h"
#include "ls_math.h"

// is env due on this tick, and is its whole history filled?  tick_mod = tick % period (formed on the host: no 64-bit division on the device)
// The rule itself, on the fields it reads: lsim_k_sensor_capture and lsim_k_depth_encode (ls_depth_encoder.h) both decide with this function.
LS_RC_FN bool ls_sensor_due(uint32_t flags, const int64_t* episode_length, int period, int stagger, int env, uint32_t tick_mod, bool& fill) {
    fill = (flags & LSIM_SENSOR_FILL_ALL) != 0u || episode_length[env] == 0;
    if (fill) return true;
    if (flags & LSIM_SENSOR_RESETS_ONLY) return false;
    const uint32_t p = (uint32_t)period;
    return (tick_mod + (stagger ? (uint32_t)env % p : 0u)) % p == 0u;      // both terms < p <= 2^31: no wrap
}
LS_RC_FN bool ls_sm_due(const lsim_sensor_model_t& sm, int env, uint32_t tick_mod, bool& fill) {
    return ls_sensor_due(sm.flags, sm.episode_length, sm.period, sm.stagger, env, tick_mod, fill);
}

// ls_rc_ray without its store: the value lsim_raycast writes for ray r of env; hit = (t < far), label 1 / 0
LS_RC_FN float ls_sm_raw_terrain(const lsim_raycast_t& rc, int env, int r, bool& hit, int& label) {
    const float* rs = rc.root_states + (size_t)13 * (size_t)env;
    const float* mt = rc.mount + (size_t)7 * (size_t)env;
    const LsRcV3 mp = ls_rc_rot(rs[3], rs[4], rs[5], rs[6], ls_rc_v3(mt[0], mt[1], mt[2]));
    const LsRcV3 o = ls_rc_v3(rs[0] + mp.x, rs[1] + mp.y, rs[2] + mp.z);
    const LsRcV3 ds = ls_rc_rot(mt[3], mt[4], mt[5], mt[6], ls_rc_v3(rc.dirs[3 * r], rc.dirs[3 * r + 1], rc.dirs[3 * r + 2]));
    const LsRcV3 d = ls_rc_rot(rs[3], rs[4], rs[5], rs[6], ds);
    const float sc = rc.scale ? rc.scale[r] : 1.0f;
    long long* state = (long long*)rc.state;
    float t = rc.far;
    if (ls_rc_finite(o.x) && ls_rc_finite(o.y) && ls_rc_finite(o.z) && ls_rc_finite(d.x) && ls_rc_finite(d.y) && ls_rc_finite(d.z)) {
        LsRcCount cnt;
        cnt.cells = 0; cnt.tris = 0;
        t = ls_rc_cast(rc, o, d, cnt);
#if defined(LS_RAYCAST_COUNTERS)
        ls_rc_count(state + 2, cnt.cells);
        ls_rc_count(state + 3, cnt.tris);
#endif
    } else {
        ls_rc_count(state, 1);
    }
    hit = t < rc.far;
    label = hit ? 1 : 0;
    return t * sc;
}

// ls_rcb_ray without its stores: the value and the label lsim_raycast_bodies writes for ray r of env; hit = (t < far)
LS_RC_FN float ls_sm_raw_bodies(const lsim_raycast_bodies_t& rb, const LsRcbShared& sh, int env, int r, bool& hit, int& label) {
    const lsim_raycast_t& rc = rb.rc;
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
    const float sc = rc.scale ? rc.scale[r] : 1.0f;
    long long* state = (long long*)rc.state;
    float t = rc.far;
    label = 0;
    const bool joints_ok = (sh.bad[0] | sh.bad[1] | sh.bad[2] | sh.bad[3]) == 0;
    if (joints_ok && ls_rc_finite(o.x) && ls_rc_finite(o.y) && ls_rc_finite(o.z) && ls_rc_finite(d.x) && ls_rc_finite(d.y) && ls_rc_finite(d.z)) {
        LsRcCount cnt;
        cnt.cells = 0; cnt.tris = 0;
        int tested = 0;
        const float tb = ls_rcb_cast(sh, mp, d, rc.near, rc.far, label, tested);
        lsim_raycast_t walk = rc;               // the shared walk, bounded by the body hit
        walk.far = tb;
        t = ls_rc_cast(walk, o, d, cnt);
        if (t < tb) label = 1;
#if defined(LS_RAYCAST_COUNTERS)
        ls_rc_count(state + 1, tested);
        ls_rc_count(state + 2, cnt.cells);
        ls_rc_count(state + 3, cnt.tris);
#endif
    } else {
        ls_rc_count(state, 1);
    }
    hit = t < rc.far;
    return t * sc;
}

// step 3: the clean value and label, the model (lsim.h states every line of it) and the ray's column of the history
LS_RC_FN void ls_sm_store(const lsim_sensor_model_t& sm, int env, int r, float raw, bool hit, int label, bool fill) {
    const lsim_raycast_bodies_t& rb = sm.rb;
    rb.rc.out[(size_t)env * (size_t)rb.rc.out_stride + (size_t)r] = raw;
    if (rb.labels) rb.labels[(size_t)env * (size_t)rb.label_stride + (size_t)r] = (uint8_t)label;
    uint32_t c[4] = {(uint32_t)env, (uint32_t)sm.tick, (uint32_t)LSIM_RNG_SENSOR, (sm.stream_id << 16) | (uint32_t)r};
    philox4x32_10(c, sm.seed, sm.rank);
    const float u0 = u32_to_u01(c[0]), u1 = u32_to_u01(c[1]), u2 = u32_to_u01(c[2]), u3 = u32_to_u01(c[3]);
    const float g = 2.0f * ((u0 + u1 + u2) - 1.5f);
    float v = raw;
    if (hit) {
        v = raw + (sm.sigma0 + sm.sigma2 * raw * raw) * g;
        if (u3 < sm.p_drop) v = sm.drop_value;
    }
    v = fminf(fmaxf(v, sm.clip_lo), sm.clip_hi);
    const float y = (v - sm.offset) * sm.gain;
    const int K = sm.latency + sm.frames;
    const size_t hs = (size_t)sm.hist_stride;
    float* h = sm.hist + (size_t)env * (size_t)K * hs + (size_t)r;
    if (fill) {
        for (int k = 0; k < K; ++k) h[(size_t)k * hs] = y;
    } else {
        for (int k = 0; k + 1 < K; ++k) h[(size_t)k * hs] = h[(size_t)(k + 1) * hs];
        h[(size_t)(K - 1) * hs] = y;
    }
}

// ---- host side: argument checks shared by the library and the CPU shim (no launch happens before they pass)
static inline bool ls_sm_terrain_only(const lsim_sensor_model_t& sm) { return !sm.rb.robots && sm.rb.num_robots == 0; }
static inline int ls_sm_validate(const lsim_sensor_model_t* sm) {
    if (!sm) return LSIM_E_INVALID;
    if (ls_sm_terrain_only(*sm)) {
        const int rv = ls_rc_validate(&sm->rb.rc);
        if (rv != LSIM_OK) return rv;
        if (sm->rb.flags != 0u || (sm->rb.labels && sm->rb.label_stride < sm->rb.rc.num_rays)) return LSIM_E_INVALID;
    } else {
        const int rv = ls_rcb_validate(&sm->rb);
        if (rv != LSIM_OK) return rv;
    }
    if (!ls_rc_aligned(sm->episode_length, 8) || !ls_rc_aligned(sm->hist, 16)) return LSIM_E_INVALID;
    if (sm->tick < 0 || sm->stream_id >= 65536u || sm->period < 1 || sm->stagger < 0 || sm->stagger > 1) return LSIM_E_INVALID;
    if (sm->latency < 0 || sm->frames < 1 || sm->latency > LSIM_SENSOR_MAX_HISTORY || sm->frames > LSIM_SENSOR_MAX_HISTORY ||
        sm->latency + sm->frames > LSIM_SENSOR_MAX_HISTORY) return LSIM_E_INVALID;
    if (sm->hist_stride < sm->rb.rc.num_rays || (sm->hist_stride & 3) != 0) return LSIM_E_INVALID;
    if (!ls_rc_host_finite(sm->sigma0) || !(sm->sigma0 >= 0.0f) || !ls_rc_host_finite(sm->sigma2) || !(sm->sigma2 >= 0.0f)) return LSIM_E_INVALID;
    if (!(sm->p_drop >= 0.0f) || !(sm->p_drop <= 1.0f) || !ls_rc_host_finite(sm->drop_value)) return LSIM_E_INVALID;
    if (!ls_rc_host_finite(sm->clip_lo) || !ls_rc_host_finite(sm->clip_hi) || !(sm->clip_lo <= sm->clip_hi)) return LSIM_E_INVALID;
    if (!ls_rc_host_finite(sm->offset) || !ls_rc_host_finite(sm->gain)) return LSIM_E_INVALID;
    if ((sm->flags & ~(uint32_t)(LSIM_SENSOR_FILL_ALL | LSIM_SENSOR_RESETS_ONLY)) != 0u) return LSIM_E_INVALID;
    if ((sm->flags & LSIM_SENSOR_FILL_ALL) && (sm->flags & LSIM_SENSOR_RESETS_ONLY)) return LSIM_E_INVALID;
    return LSIM_OK;
}
static inline uint32_t ls_sm_tick_mod(const lsim_sensor_model_t& sm) { return (uint32_t)(sm.tick % (int64_t)sm.period); }

#if defined(__HIPCC__) && !defined(LS_EMU)
__global__ __launch_bounds__(LS_RC_BLOCK) void lsim_k_sensor_capture(const lsim_sensor_model_t sm, int blocks_per_env, uint32_t tick_mod) {
    __shared__ LsRcbShared sh;
    const lsim_raycast_bodies_t& rb = sm.rb;
    const int slot = (int)blockIdx.x / blocks_per_env, chunk = (int)blockIdx.x - slot * blocks_per_env;
    const int env = slot * rb.rc.env_stride, lane = (int)threadIdx.x, r = chunk * LS_RC_BLOCK + lane;
    if (env >= rb.rc.num_envs) return;          // the whole block: env is blockIdx's
    bool fill;
    if (!ls_sm_due(sm, env, tick_mod, fill)) return;     // the whole block again, before LDS and the barriers
    bool hit = false;
    int label = 0;
    float raw = 0.0f;
    if (rb.robots) {
        if (lane < LSIM_NUM_LEGS) ls_rcb_fk(rb, sh, env, lane);
        __syncthreads();
        if (lane < sh.nprims) ls_rcb_prim(rb, sh, env, lane);
        __syncthreads();
        if (r < rb.rc.num_rays) raw = ls_sm_raw_bodies(rb, sh, env, r, hit, label);
    } else if (r < rb.rc.num_rays) {
        raw = ls_sm_raw_terrain(rb.rc, env, r, hit, label);
    }
    if (r < rb.rc.num_rays) ls_sm_store(sm, env, r, raw, hit, label, fill);
}

extern "C" int lsim_sensor_capture(const lsim_sensor_model_t* sm, void* stream) {
    const int rv = ls_sm_validate(sm);
    if (rv != LSIM_OK) return rv;
    const int bpe = ls_rc_blocks_per_env(sm->rb.rc);
    const long long blocks = (long long)bpe * ls_rc_env_slots(sm->rb.rc);
    if (blocks > 0x7fffffffLL) return LSIM_E_INVALID;
    hipLaunchKernelGGL(lsim_k_sensor_capture, dim3((unsigned)blocks), dim3(LS_RC_BLOCK), 0, (hipStream_t)stream, *sm, bpe, ls_sm_tick_mod(*sm));
    return hipGetLastError() == hipSuccess ? LSIM_OK : LSIM_E_HIP;
}
#endif
