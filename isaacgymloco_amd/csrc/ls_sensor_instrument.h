// ls_sensor_instrument.h -- per-episode error of a sensor's own constants (include/lsim.h, lsim_sensor_instrument and lsim_sensor_capture_inst):
// one launch that draws, for every env that starts an episode, its row {lat, noise_gain, depth_scale, depth_quad, tan_scale, 0, 0, 0}, and the
// capture that reads the rows: lsim_k_sensor_capture with the env's latency, noise level, depth-scale error and field of view in place of the
// shared ones.  lsim.h states every formula; this file is that text in code.
//
// Self-contained like ls_sensor_model.h (lsim.h, ls_sensor_model.h and what it includes, the C library): tests/emu/emu_sensor_instrument.cpp
// compiles this file with g++ under LS_EMU and runs the same per-env, per-block and per-ray code over plain arrays.
//
// Shape of the draw launch (lsim_k_sensor_instrument): lsim_k_sensor_mount_jitter's -- one lane per VISITED env, blocks of 256, a lane whose
// env is not fresh ends after one 8-byte load.  A fresh one runs 20 Philox rounds and a dozen fp32 operations and writes its 32-byte row as two
// 16-byte stores.  At N = 4096 that is 16 blocks and 128 KB at the most: the launch is its own launch overhead.
//
// Shape of the capture (lsim_k_sensor_capture_inst): lsim_k_sensor_capture's, through the same functions -- ls_rc_block and ls_sm_due first,
// ls_rcb_block (the prologue of lsim_k_raycast_bodies) unless terrain only, then per ray a cast and a store.  The two early returns stand in
// each kernel: folded into one function that returns "go on", they changed the branch layout of both kernels.  What differs:
//   0. a due block loads its env's row once, into one VGPR (lane k holds row[k & 7]); the values are read out of it as wave-uniform scalars
//      (v_readlane) where they are used -- tan_scale ahead of the cast, the others behind it: the cast leaves no SGPR to carry them across;
//   1. ls_si_ray: the ray's direction and scale in the sensor frame, widened or narrowed by tan_scale.  One correctly rounded square root and
//      one division per ray, skipped by the whole block when tan_scale == 1;
//   2. ls_si_raw_terrain / ls_si_raw_bodies: ls_rc_value / ls_rcb_value (ls_raycast.h, ls_raycast_bodies.h) on that direction and scale, the
//      ray routines lsim_k_sensor_capture calls on the tables' own.  Nothing of the ray is restated here;
//   3. ls_si_store: the three pieces of ls_sm_store (ls_sm_clean, ls_sm_draw, ls_sm_history) around this launch's model line -- the calibration
//      error and the noise gain on a hit -- with the history shifted over the env's own Ke = L + frames <= K slots; the slots from Ke - 1 on
//      all take the new value, so they never hold anything older.
// That the neutral row writes lsim_sensor_capture's bits now follows from the source, up to the model line (ls_si_calibrated says what that takes).
#pragma once
#include "ls_sensor_model.h"
#include "ls_math.h"

#define LS_SI_ROW 8         // floats per row of inst

// the block-uniform values of ls_si_store's model line: of the env's row {lat, noise_gain, depth_scale, depth_quad, tan_scale, 0, 0, 0} the
// first four (lat as `slots`, below), and the three constants of the model they combine with
struct LsSiRow { int slots; float noise_gain, depth_scale, depth_quad, sigma0, sigma2, p_drop; };
// slots: Ke = L + frames, the slots of the history that an env with latency `lat` shifts through; frames <= Ke <= K
LS_RC_FN int ls_si_slots(const lsim_sensor_model_t& sm, float lat) {
    const int l = (int)lat;
    return (l < 0 ? 0 : (l > sm.latency ? sm.latency : l)) + sm.frames;
}

// ---- the draw launch
LS_RC_FN bool ls_si_fresh(const lsim_sensor_instrument_t& si, int env) { return ls_sensor_fresh(si.flags, si.episode_length, env); }

LS_RC_FN void ls_si_store_row(float* p, float a, float b, float c, float d, float e) {
#if defined(__HIPCC__) && !defined(LS_EMU)
    ((float4*)p)[0] = make_float4(a, b, c, d);      // rows are 32-byte aligned: two 16-byte stores
    ((float4*)p)[1] = make_float4(e, 0.0f, 0.0f, 0.0f);
#else
    p[0] = a; p[1] = b; p[2] = c; p[3] = d;
    p[4] = e; p[5] = 0.0f; p[6] = 0.0f; p[7] = 0.0f;
#endif
}

// the row of one fresh env
LS_RC_FN void ls_si_env(const lsim_sensor_instrument_t& si, int env) {
    uint32_t c0[4] = {(uint32_t)env, (uint32_t)si.tick, (uint32_t)LSIM_RNG_SENSOR_INSTRUMENT, (si.stream_id << 16) | 0u};
    uint32_t c1[4] = {(uint32_t)env, (uint32_t)si.tick, (uint32_t)LSIM_RNG_SENSOR_INSTRUMENT, (si.stream_id << 16) | 1u};
    philox4x32_10(c0, si.seed, si.rank);
    philox4x32_10(c1, si.seed, si.rank);
    const float u0 = u32_to_u01(c0[0]), u1 = u32_to_u01(c0[1]), u2 = u32_to_u01(c0[2]), u3 = u32_to_u01(c0[3]), u4 = u32_to_u01(c1[0]);
    const int span = si.lat_hi - si.lat_lo;
    int j = (int)floorf(u0 * (float)(span + 1));
    j = j < span ? j : span;
    const float lat = (float)(si.lat_hi - j);
    const float noise_gain = si.gain_lo + u1 * (si.gain_hi - si.gain_lo);
    const float depth_scale = (2.0f * u2 - 1.0f) * si.scale_range;
    const float depth_quad = (2.0f * u3 - 1.0f) * si.quad_range;
    const float tan_scale = 1.0f + (2.0f * u4 - 1.0f) * si.fov_range;
    ls_si_store_row(si.inst + (size_t)LS_SI_ROW * (size_t)env, lat, noise_gain, depth_scale, depth_quad, tan_scale);
}

// ---- the capture
// step 1: direction and scale of ray r in the sensor frame under the env's tan_scale
LS_RC_FN LsRcV3 ls_si_ray(const lsim_raycast_t& rc, int r, float tan_scale, float& sc) {
    LsRcV3 s = ls_rc_v3(rc.dirs[3 * r], rc.dirs[3 * r + 1], rc.dirs[3 * r + 2]);
    sc = rc.scale ? rc.scale[r] : 1.0f;
    if (tan_scale != 1.0f && s.x > 0.0f) {
        const float y = s.y * tan_scale, z = s.z * tan_scale;
        const float q = ls_div_exact(1.0f, ls_sqrt_exact(s.x * s.x + y * y + z * z));
        s = ls_rc_v3(s.x * q, y * q, z * q);
        sc = sc * q;
    }
    return s;
}

// step 2: the shared ray routines at the direction s and the scale sc
LS_RC_FN float ls_si_raw_terrain(const lsim_raycast_t& rc, int env, LsRcV3 s, float sc, bool& hit, int& label) {
    const float v[3] = {s.x, s.y, s.z};
    return ls_rc_value(rc, env, v, &sc, hit, label);
}
LS_RC_FN float ls_si_raw_bodies(const lsim_raycast_bodies_t& rb, const LsRcbShared& sh, int env, LsRcV3 s, float sc, bool& hit, int& label) {
    const float v[3] = {s.x, s.y, s.z};
    return ls_rcb_value(rb, sh, env, v, &sc, hit, label);
}

// m of the header, rounded as a product of its own.  Left to itself the compiler may fuse it into the sum that follows (m + n g as
// fma(raw, 1 + c, n g)), which rounds n g, where lsim_k_sensor_capture, with only one product to fuse, forms fma(n, g, raw) and does not:
// under the neutral row the two launches would then differ in the last bit
LS_RC_FN float ls_si_calibrated(float raw, float depth_scale, float depth_quad) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return raw * (1.0f + (depth_scale + depth_quad * raw));
}

// step 3: ls_sm_store under the env's row -- its three pieces (ls_sensor_model.h) around this launch's own model line, over the env's Ke slots
LS_RC_FN void ls_si_store(const lsim_sensor_model_t& sm, const LsSiRow& row, int env, int r, float raw, bool hit, int label, bool fill) {
    ls_sm_clean(sm.rb, env, r, raw, label);
    float u3;
    const float g = ls_sm_draw(sm, env, r, u3);
    float v = raw;
    if (hit) {
        const float m = ls_si_calibrated(raw, row.depth_scale, row.depth_quad);
        v = m + (row.noise_gain * (row.sigma0 + row.sigma2 * raw * raw)) * g;
        if (u3 < row.p_drop) v = sm.drop_value;
    }
    ls_sm_history(sm, env, r, v, row.slots, fill);
}

// ---- host side: the argument checks shared by the library and the CPU shim (no launch happens before they pass)
static inline int ls_si_validate(const lsim_sensor_instrument_t* si) {
    if (!si) return LSIM_E_INVALID;
    if (!ls_rc_aligned(si->inst, 32) || !ls_rc_aligned(si->episode_length, 8)) return LSIM_E_INVALID;
    if (si->num_envs < 1 || si->env_stride < 1 || si->tick < 0 || si->stream_id >= 65536u) return LSIM_E_INVALID;
    if (si->lat_lo < 0 || si->lat_lo > si->lat_hi || si->lat_hi >= LSIM_SENSOR_MAX_HISTORY) return LSIM_E_INVALID;
    const float ranges[5] = {si->gain_lo, si->gain_hi, si->scale_range, si->quad_range, si->fov_range};
    for (int k = 0; k < 5; ++k)
        if (!ls_rc_host_finite(ranges[k]) || !(ranges[k] >= 0.0f)) return LSIM_E_INVALID;
    if (!(si->gain_lo <= si->gain_hi) || !(si->fov_range < 1.0f)) return LSIM_E_INVALID;
    if (!ls_sensor_flags_ok(si->flags)) return LSIM_E_INVALID;
    return LSIM_OK;
}
static inline int ls_si_env_slots(const lsim_sensor_instrument_t& si) { return ls_sensor_env_slots(si.num_envs, si.env_stride); }
static inline int ls_si_capture_validate(const lsim_sensor_model_t* sm, const float* inst) {
    const int rv = ls_sm_validate(sm);
    if (rv != LSIM_OK) return rv;
    return ls_rc_aligned(inst, 16) ? LSIM_OK : LSIM_E_INVALID;
}

#if defined(__HIPCC__) && !defined(LS_EMU)
__global__ __launch_bounds__(LS_RC_BLOCK) void lsim_k_sensor_instrument(const lsim_sensor_instrument_t si, int slots) {
    const long long lane = (long long)blockIdx.x * LS_RC_BLOCK + (long long)threadIdx.x;
    if (lane >= (long long)slots) return;
    const int slot = (int)lane;
    const int env = slot * si.env_stride;       // < num_envs: slot <= (num_envs - 1) / env_stride
    if (ls_si_fresh(si, env)) ls_si_env(si, env);
}

extern "C" int lsim_sensor_instrument(const lsim_sensor_instrument_t* si, void* stream) {
    const int rv = ls_si_validate(si);
    if (rv != LSIM_OK) return rv;
    const int slots = ls_si_env_slots(*si);
    hipLaunchKernelGGL(lsim_k_sensor_instrument, dim3((unsigned)(((long long)slots + LS_RC_BLOCK - 1) / LS_RC_BLOCK)), dim3(LS_RC_BLOCK), 0,
                       (hipStream_t)stream, *si, slots);
    return hipGetLastError() == hipSuccess ? LSIM_OK : LSIM_E_HIP;
}

__global__ __launch_bounds__(LS_RC_BLOCK) void lsim_k_sensor_capture_inst(const lsim_sensor_model_t sm, const float* __restrict__ inst, int blocks_per_env,
                                                                          uint32_t tick_mod) {
    __shared__ LsRcbShared sh;
    const lsim_raycast_bodies_t& rb = sm.rb;
    const int lane = (int)threadIdx.x;
    int env, r;
    ls_rc_block(rb.rc, blocks_per_env, env, r);
    if (env >= rb.rc.num_envs) return;          // the whole block: env is blockIdx's
    bool fill;
    if (!ls_sm_due(sm, env, tick_mod, fill)) return;     // the whole block again, before LDS and the barriers
    // The env's row, loaded once into ONE VGPR: lane k of every wave holds row[k & 7] (every lane is live here).  tan_scale is read out of it
    // at once; lat becomes the slot count Ke; and the reserved lanes 5..7 take sigma0, sigma2 and p_drop.  Behind the cast ls_si_store's seven
    // block-uniform values are read back with v_readlane.  lsim_k_sensor_capture already holds 99 of the 100 SGPRs across the cast (the struct
    // comes by value), so the row cannot ride in SGPRs without spills; parked in lanes, it costs one VGPR and frees three SGPRs.
    const int sub = lane & (LS_SI_ROW - 1);
    const int rowv = __float_as_int(inst[(size_t)LS_SI_ROW * (size_t)env + (size_t)sub]);
    const float tan_scale = __int_as_float(__builtin_amdgcn_readlane(rowv, 4));
    const int slots = ls_si_slots(sm, __int_as_float(__builtin_amdgcn_readlane(rowv, 0)));
    const int carried = sub == 0 ? slots : sub == 5 ? __float_as_int(sm.sigma0) : sub == 6 ? __float_as_int(sm.sigma2) : sub == 7 ? __float_as_int(sm.p_drop) : rowv;
    bool hit = false;
    int label = 0;
    float raw = 0.0f, sc = 1.0f;
    if (rb.robots) {
        ls_rcb_block(rb, sh, env, lane);
        if (r < rb.rc.num_rays) {
            const LsRcV3 s = ls_si_ray(rb.rc, r, tan_scale, sc);
            raw = ls_si_raw_bodies(rb, sh, env, s, sc, hit, label);
        }
    } else if (r < rb.rc.num_rays) {
        const LsRcV3 s = ls_si_ray(rb.rc, r, tan_scale, sc);
        raw = ls_si_raw_terrain(rb.rc, env, s, sc, hit, label);
    }
    if (r < rb.rc.num_rays) {
        const LsSiRow row = {__builtin_amdgcn_readlane(carried, 0), __int_as_float(__builtin_amdgcn_readlane(carried, 1)),
                             __int_as_float(__builtin_amdgcn_readlane(carried, 2)), __int_as_float(__builtin_amdgcn_readlane(carried, 3)),
                             __int_as_float(__builtin_amdgcn_readlane(carried, 5)), __int_as_float(__builtin_amdgcn_readlane(carried, 6)),
                             __int_as_float(__builtin_amdgcn_readlane(carried, 7))};
        ls_si_store(sm, row, env, r, raw, hit, label, fill);
    }
}

extern "C" int lsim_sensor_capture_inst(const lsim_sensor_model_t* sm, const float* inst, void* stream) {
    const int rv = ls_si_capture_validate(sm, inst);
    if (rv != LSIM_OK) return rv;
    int bpe;
    unsigned blocks;
    if (!ls_rc_grid(sm->rb.rc, bpe, blocks)) return LSIM_E_INVALID;
    hipLaunchKernelGGL(lsim_k_sensor_capture_inst, dim3(blocks), dim3(LS_RC_BLOCK), 0, (hipStream_t)stream, *sm, inst, bpe, ls_sm_tick_mod(*sm));
    return hipGetLastError() == hipSuccess ? LSIM_OK : LSIM_E_HIP;
}
#endif
