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
//   1. the prologue of lsim_k_raycast_bodies (ls_rcb_block: ls_rcb_fk, ls_rcb_prim and their barriers) unless the struct is of the terrain-only
//      form, which skips it and LDS altogether;
//   2. ls_sm_raw_bodies / ls_sm_raw_terrain: one line each, ls_rcb_value / ls_rc_value at the tables' direction and scale.  ls_rc_value is the
//      very function ls_rc_ray stores the result of, so the terrain-only identity model writes lsim_raycast's bits by construction of the
//      source; ls_rcb_value is shared with lsim_k_sensor_capture_inst, and ls_rcb_ray is its text once more (ls_raycast_bodies.h says why).
//      Compared on the device against the commit that still had a copy per launch: profiles/raycast_refactor_ab.json;
//   3. ls_sm_store: the clean value to out, one Philox block per ray, the model, and the ray's own column of hist -- K slots hist_stride floats
//      apart, lane = consecutive r, so every slot is read and written by a wave as one coalesced 256-byte line, and no lane reads what another
//      writes.  It is three shared pieces (ls_sm_clean, ls_sm_draw, ls_sm_history) around the model line; ls_si_store is the same three around its own.
#pragma once
#include "ls_raycast_bodies.h"
#include "ls_math.h"

// ---- the visit rule of the sensor chain, on the fields it reads: every launch that takes `flags` decides with these functions
// the legal values of flags: 0, LSIM_SENSOR_FILL_ALL or LSIM_SENSOR_RESETS_ONLY
static inline bool ls_sensor_flags_ok(uint32_t flags) {
    if ((flags & ~(uint32_t)(LSIM_SENSOR_FILL_ALL | LSIM_SENSOR_RESETS_ONLY)) != 0u) return false;
    return !((flags & LSIM_SENSOR_FILL_ALL) && (flags & LSIM_SENSOR_RESETS_ONLY));
}
// the env slots a launch visits (slot i is env i * env_stride), for the num_envs >= 1 and env_stride >= 1 every validator demands
static inline int ls_sensor_env_slots(int num_envs, int env_stride) { return (num_envs - 1) / env_stride + 1; }
// tick % period, formed on the host: no 64-bit division on the device
static inline uint32_t ls_sensor_tick_mod(int64_t tick, int period) { return (uint32_t)(tick % (int64_t)period); }
// does env start an episode (or does the call say that all do)?
LS_RC_FN bool ls_sensor_fresh(uint32_t flags, const int64_t* episode_length, int env) {
    return (flags & LSIM_SENSOR_FILL_ALL) != 0u || episode_length[env] == 0;
}
// is env due on this tick, and is its whole history filled?  tick_mod = ls_sensor_tick_mod(tick, period)
LS_RC_FN bool ls_sensor_due(uint32_t flags, const int64_t* episode_length, int period, int stagger, int env, uint32_t tick_mod, bool& fill) {
    fill = ls_sensor_fresh(flags, episode_length, env);
    if (fill) return true;
    if (flags & LSIM_SENSOR_RESETS_ONLY) return false;
    const uint32_t p = (uint32_t)period;
    return (tick_mod + (stagger ? (uint32_t)env % p : 0u)) % p == 0u;      // both terms < p <= 2^31: no wrap
}
// the rule on the sensor model's own fields, under the names the CPU shims call
LS_RC_FN bool ls_sm_due(const lsim_sensor_model_t& sm, int env, uint32_t tick_mod, bool& fill) {
    return ls_sensor_due(sm.flags, sm.episode_length, sm.period, sm.stagger, env, tick_mod, fill);
}

// step 2: the value and label lsim_raycast / lsim_raycast_bodies write for ray r of env -- the shared ray routines at the tables' direction and scale
LS_RC_FN float ls_sm_raw_terrain(const lsim_raycast_t& rc, int env, int r, bool& hit, int& label) {
    return ls_rc_value(rc, env, rc.dirs + 3 * r, rc.scale ? rc.scale + r : nullptr, hit, label);
}
LS_RC_FN float ls_sm_raw_bodies(const lsim_raycast_bodies_t& rb, const LsRcbShared& sh, int env, int r, bool& hit, int& label) {
    return ls_rcb_value(rb, sh, env, rb.rc.dirs + 3 * r, rb.rc.scale ? rb.rc.scale + r : nullptr, hit, label);
}

// step 3 comes in three pieces, which ls_si_store (ls_sensor_instrument.h) shares: the two stores differ in the model line between (b) and (c)
// and in the slot count Ke alone.
// (a) the clean value and label
LS_RC_FN void ls_sm_clean(const lsim_raycast_bodies_t& rb, int env, int r, float raw, int label) {
    rb.rc.out[(size_t)env * (size_t)rb.rc.out_stride + (size_t)r] = raw;
    if (rb.labels) rb.labels[(size_t)env * (size_t)rb.label_stride + (size_t)r] = (uint8_t)label;
}
// (b) the ray's Philox block: the bounded normal g of three uniforms, and the dropout uniform u3
LS_RC_FN float ls_sm_draw(const lsim_sensor_model_t& sm, int env, int r, float& u3) {
    uint32_t c[4] = {(uint32_t)env, (uint32_t)sm.tick, (uint32_t)LSIM_RNG_SENSOR, (sm.stream_id << 16) | (uint32_t)r};
    philox4x32_10(c, sm.seed, sm.rank);
    const float u0 = u32_to_u01(c[0]), u1 = u32_to_u01(c[1]), u2 = u32_to_u01(c[2]);
    u3 = u32_to_u01(c[3]);
    return 2.0f * ((u0 + u1 + u2) - 1.5f);
}
// (c) clip, normalise, and the ray's column of the history: shifted over its first Ke <= K slots, the slots from Ke - 1 on taking the new value
// (Ke = K is the plain shift of all K slots)
LS_RC_FN void ls_sm_history(const lsim_sensor_model_t& sm, int env, int r, float v, int Ke, bool fill) {
    v = fminf(fmaxf(v, sm.clip_lo), sm.clip_hi);
    const float y = (v - sm.offset) * sm.gain;
    const int K = sm.latency + sm.frames;
    const size_t hs = (size_t)sm.hist_stride;
    float* h = sm.hist + (size_t)env * (size_t)K * hs + (size_t)r;
    if (fill) {
        for (int k = 0; k < K; ++k) h[(size_t)k * hs] = y;
    } else {
        for (int k = 0; k + 1 < Ke; ++k) h[(size_t)k * hs] = h[(size_t)(k + 1) * hs];
        for (int k = Ke - 1; k < K; ++k) h[(size_t)k * hs] = y;
    }
}

// step 3: the clean value and label, the model (lsim.h states every line of it) and the ray's column of the history
LS_RC_FN void ls_sm_store(const lsim_sensor_model_t& sm, int env, int r, float raw, bool hit, int label, bool fill) {
    ls_sm_clean(sm.rb, env, r, raw, label);
    float u3;
    const float g = ls_sm_draw(sm, env, r, u3);
    float v = raw;
    if (hit) {
        v = raw + (sm.sigma0 + sm.sigma2 * raw * raw) * g;
        if (u3 < sm.p_drop) v = sm.drop_value;
    }
    ls_sm_history(sm, env, r, v, sm.latency + sm.frames, fill);
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
    if (!ls_sensor_flags_ok(sm->flags)) return LSIM_E_INVALID;
    return LSIM_OK;
}
static inline uint32_t ls_sm_tick_mod(const lsim_sensor_model_t& sm) { return ls_sensor_tick_mod(sm.tick, sm.period); }

#if defined(__HIPCC__) && !defined(LS_EMU)
__global__ __launch_bounds__(LS_RC_BLOCK) void lsim_k_sensor_capture(const lsim_sensor_model_t sm, int blocks_per_env, uint32_t tick_mod) {
    __shared__ LsRcbShared sh;
    const lsim_raycast_bodies_t& rb = sm.rb;
    int env, r;
    ls_rc_block(rb.rc, blocks_per_env, env, r);
    if (env >= rb.rc.num_envs) return;          // the whole block: env is blockIdx's
    bool fill;
    if (!ls_sm_due(sm, env, tick_mod, fill)) return;     // the whole block again, before LDS and the barriers
    bool hit = false;
    int label = 0;
    float raw = 0.0f;
    if (rb.robots) {
        ls_rcb_block(rb, sh, env, (int)threadIdx.x);
        if (r < rb.rc.num_rays) raw = ls_sm_raw_bodies(rb, sh, env, r, hit, label);
    } else if (r < rb.rc.num_rays) {
        raw = ls_sm_raw_terrain(rb.rc, env, r, hit, label);
    }
    if (r < rb.rc.num_rays) ls_sm_store(sm, env, r, raw, hit, label, fill);
}

extern "C" int lsim_sensor_capture(const lsim_sensor_model_t* sm, void* stream) {
    const int rv = ls_sm_validate(sm);
    if (rv != LSIM_OK) return rv;
    int bpe;
    unsigned blocks;
    if (!ls_rc_grid(sm->rb.rc, bpe, blocks)) return LSIM_E_INVALID;
    hipLaunchKernelGGL(lsim_k_sensor_capture, dim3(blocks), dim3(LS_RC_BLOCK), 0, (hipStream_t)stream, *sm, bpe, ls_sm_tick_mod(*sm));
    return hipGetLastError() == hipSuccess ? LSIM_OK : LSIM_E_HIP;
}
#endif
