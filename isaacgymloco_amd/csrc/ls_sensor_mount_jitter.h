// ls_sensor_mount_jitter.h -- per-episode randomisation of a sensor's mount pose (include/lsim.h, lsim_sensor_mount_jitter): for every env
// that starts an episode, two Philox blocks -> six uniforms -> a position offset and a small rotation about the base axes, written over the
// env's row of the mount array the capture kernels already read.  lsim.h states every formula; this file is that text in code.
//
// Self-contained like ls_sensor_model.h (lsim.h, the helpers of ls_raycast.h / ls_raycast_bodies.h, the Philox of ls_math.h and the C library):
// tests/emu/emu_sensor_mount_jitter.cpp compiles this file with g++ under LS_EMU and runs the same per-env code over plain arrays.
//
// Shape of the launch (lsim_k_sensor_mount_jitter): one lane per VISITED env (lane i of the grid is env i * env_stride), blocks of 256.  A lane
// whose env is not fresh ends after one 8-byte load.  A fresh one reads its 28-byte row of `nominal`, runs 20 Philox rounds and ~60 fp32
// operations, and writes its 28-byte row of `mount` with seven plain dword stores: rows are 28 bytes apart, so neither the loads nor the
// stores can be wider than a dword without straddling rows.  At N = 4096 that is 16 blocks and 112 KB of traffic at the most: the launch is
// its own launch overhead, and nothing here is worth tuning.
#pragma once
#include "ls_sensor_model.h"
#include "ls_math.h"

LS_RC_FN bool ls_smj_fresh(const lsim_sensor_mount_jitter_t& mj, int env) { return ls_sensor_fresh(mj.flags, mj.episode_length, env); }

// the row of one fresh env
LS_RC_FN void ls_smj_env(const lsim_sensor_mount_jitter_t& mj, int env) {
    uint32_t c0[4] = {(uint32_t)env, (uint32_t)mj.tick, (uint32_t)LSIM_RNG_SENSOR_MOUNT, (mj.stream_id << 16) | 0u};
    uint32_t c1[4] = {(uint32_t)env, (uint32_t)mj.tick, (uint32_t)LSIM_RNG_SENSOR_MOUNT, (mj.stream_id << 16) | 1u};
    philox4x32_10(c0, mj.seed, mj.rank);
    philox4x32_10(c1, mj.seed, mj.rank);
    const float s0 = 2.0f * u32_to_u01(c0[0]) - 1.0f, s1 = 2.0f * u32_to_u01(c0[1]) - 1.0f, s2 = 2.0f * u32_to_u01(c0[2]) - 1.0f;
    const float s3 = 2.0f * u32_to_u01(c0[3]) - 1.0f, s4 = 2.0f * u32_to_u01(c1[0]) - 1.0f, s5 = 2.0f * u32_to_u01(c1[1]) - 1.0f;
    const float* n = mj.nominal + (size_t)7 * (size_t)env;
    float* m = mj.mount + (size_t)7 * (size_t)env;
    const float h0 = 0.5f * (s3 * mj.rot_range[0]), h1 = 0.5f * (s4 * mj.rot_range[1]), h2 = 0.5f * (s5 * mj.rot_range[2]);
    const float c = ls_div_exact(1.0f, ls_sqrt_exact(1.0f + (h0 * h0 + h1 * h1 + h2 * h2)));
    const LsRcbQ q = ls_rcb_qmul(ls_rcb_q(h0 * c, h1 * c, h2 * c, c), ls_rcb_q(n[3], n[4], n[5], n[6]));
    m[0] = n[0] + s0 * mj.pos_range[0];
    m[1] = n[1] + s1 * mj.pos_range[1];
    m[2] = n[2] + s2 * mj.pos_range[2];
    m[3] = q.x;
    m[4] = q.y;
    m[5] = q.z;
    m[6] = q.w;
}

// ---- host side: the argument check shared by the library and the CPU shim (no launch happens before it passes)
static inline int ls_smj_validate(const lsim_sensor_mount_jitter_t* mj) {
    if (!mj) return LSIM_E_INVALID;
    if (!ls_rc_aligned(mj->nominal, 4) || !ls_rc_aligned(mj->mount, 4) || !ls_rc_aligned(mj->episode_length, 8)) return LSIM_E_INVALID;
    if ((const void*)mj->mount == (const void*)mj->nominal) return LSIM_E_INVALID;
    if (mj->num_envs < 1 || mj->env_stride < 1 || mj->tick < 0 || mj->stream_id >= 65536u) return LSIM_E_INVALID;
    for (int k = 0; k < 3; ++k) {
        if (!ls_rc_host_finite(mj->pos_range[k]) || !(mj->pos_range[k] >= 0.0f)) return LSIM_E_INVALID;
        if (!ls_rc_host_finite(mj->rot_range[k]) || !(mj->rot_range[k] >= 0.0f)) return LSIM_E_INVALID;
    }
    if (!ls_sensor_flags_ok(mj->flags)) return LSIM_E_INVALID;
    return LSIM_OK;
}
static inline int ls_smj_env_slots(const lsim_sensor_mount_jitter_t& mj) { return ls_sensor_env_slots(mj.num_envs, mj.env_stride); }

#if defined(__HIPCC__) && !defined(LS_EMU)
__global__ __launch_bounds__(LS_RC_BLOCK) void lsim_k_sensor_mount_jitter(const lsim_sensor_mount_jitter_t mj, int slots) {
    const long long lane = (long long)blockIdx.x * LS_RC_BLOCK + (long long)threadIdx.x;
    if (lane >= (long long)slots) return;
    const int slot = (int)lane;
    const int env = slot * mj.env_stride;       // < num_envs: slot <= (num_envs - 1) / env_stride
    if (ls_smj_fresh(mj, env)) ls_smj_env(mj, env);
}

extern "C" int lsim_sensor_mount_jitter(const lsim_sensor_mount_jitter_t* mj, void* stream) {
    const int rv = ls_smj_validate(mj);
    if (rv != LSIM_OK) return rv;
    const int slots = ls_smj_env_slots(*mj);
    hipLaunchKernelGGL(lsim_k_sensor_mount_jitter, dim3((unsigned)(((long long)slots + LS_RC_BLOCK - 1) / LS_RC_BLOCK)), dim3(LS_RC_BLOCK), 0,
                       (hipStream_t)stream, *mj, slots);
    return hipGetLastError() == hipSuccess ? LSIM_OK : LSIM_E_HIP;
}
#endif
