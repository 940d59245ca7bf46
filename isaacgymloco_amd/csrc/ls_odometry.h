// ls_odometry.h -- the two per-step launches of a map policy (include/lsim.h): lsim_odometry_step, an estimated base pose that drifts with
// the distance travelled, and lsim_map_rows, the elevation map's scan as the rows an actor reads.  lsim.h states every formula; this file is
// that text in code.
//
// Self-contained like ls_elevation_map.h (lsim.h, the helpers of ls_raycast.h / ls_raycast_bodies.h, the visit rule of ls_sensor_model.h, the
// Philox of ls_math.h and the C library): tests/emu/emu_odometry.cpp and tests/emu/emu_map_rows.cpp compile this file with g++ under LS_EMU
// and run the same per-lane code over plain arrays.
//
// Shape of lsim_k_odometry_step: lsim_k_sensor_mount_jitter's -- one lane per VISITED env (lane i of the grid is env i * env_stride), blocks
// of 256.  Every lane reads its 52-byte row of root_states (dword loads: rows are 52 bytes apart) and its 48-byte row of odo (three 16-byte
// loads), runs ONE Philox block (10 rounds: block 1 for a fresh env, block 0 for the others), ~80 fp32 operations with three correctly rounded
// roots / quotients, and writes odo with three 16-byte vector stores and est with thirteen dword stores.  At N = 4096 that is 16 blocks and
// 660 KB of traffic: the launch is its own launch overhead.
//
// Shape of lsim_k_map_rows: one lane per (visited env, column), the columns of an env consecutive lanes, blocks of 256 over the flattened
// index -- a wave reads 64 consecutive floats of a scan row (or 64 consecutive bytes of a known row) and writes 64 consecutive floats of a
// rows row, all coalesced; pose[e][2] is one dword that the lanes of an env share (one cache line per env).  One integer division per lane
// finds the env.  Nothing is staged, nothing is reduced: 4 + 1 bytes read and 8 written per point.
#pragma once
#include "ls_sensor_model.h"
#include "ls_math.h"

// ------------------------------------------------------------------------------------------------ odometry
struct LsOdoRow { float v[12]; };         // {dx, dy, dz, h, scale, yaw_bias, z_bias, 0, prev_x, prev_y, 0, 0}

#if defined(LS_EMU) || !defined(__HIPCC__)
LS_RC_FN LsOdoRow ls_odo_load(const float* o) { LsOdoRow r; for (int k = 0; k < 12; ++k) r.v[k] = o[k]; return r; }
LS_RC_FN void ls_odo_store(float* o, const LsOdoRow& r) { for (int k = 0; k < 12; ++k) o[k] = r.v[k]; }
#else
// rows of odo are 48 bytes apart and the array is 16-byte aligned (ls_odo_validate): three 16-byte accesses per row
LS_RC_FN LsOdoRow ls_odo_load(const float* o) {
    LsOdoRow r;
    for (int k = 0; k < 3; ++k) {
        const float4 a = ((const float4*)o)[k];
        r.v[4 * k] = a.x; r.v[4 * k + 1] = a.y; r.v[4 * k + 2] = a.z; r.v[4 * k + 3] = a.w;
    }
    return r;
}
LS_RC_FN void ls_odo_store(float* o, const LsOdoRow& r) {
    for (int k = 0; k < 3; ++k) ((float4*)o)[k] = make_float4(r.v[4 * k], r.v[4 * k + 1], r.v[4 * k + 2], r.v[4 * k + 3]);
}
#endif

LS_RC_FN float ls_odo_nan() { const uint32_t u = 0x7FC00000u; float v; __builtin_memcpy(&v, &u, 4); return v; }

// one visited env
LS_RC_FN void ls_odo_env(const lsim_odometry_t& od, int env) {
    const float* rs = od.root_states + (size_t)13 * (size_t)env;
    float* est = od.est + (size_t)13 * (size_t)env;
    float* orow = od.odo + (size_t)12 * (size_t)env;
    float p[13];
    for (int k = 0; k < 13; ++k) p[k] = rs[k];
    bool finite = true;
    for (int k = 0; k < 7; ++k) finite = finite && ls_rc_finite(p[k]);
    const bool fresh = ls_sensor_fresh(od.flags, od.episode_length, env);
    // one block per lane: the episode's biases (block 1) for a fresh env, the step's noise (block 0) for the others; the fourth word is unused
    uint32_t c[4] = {(uint32_t)env, (uint32_t)od.tick, (uint32_t)LSIM_RNG_ODOMETRY, (od.stream_id << 16) | (fresh ? 1u : 0u)};
    philox4x32_10(c, od.seed, od.rank);
    const float sa = 2.0f * u32_to_u01(c[0]) - 1.0f, sb = 2.0f * u32_to_u01(c[1]) - 1.0f, sc = 2.0f * u32_to_u01(c[2]) - 1.0f;
    LsOdoRow o;
    if (fresh) {
        o.v[0] = o.v[1] = o.v[2] = o.v[3] = 0.0f;
        o.v[4] = sa * od.scale_range;               // s4
        o.v[5] = sb * od.yaw_range;                 // s5
        o.v[6] = sc * od.z_range;                   // s6
        o.v[8] = p[0];
        o.v[9] = p[1];
    } else {
        o = ls_odo_load(orow);
        if (finite) {
            const bool have = ls_rc_finite(o.v[8]) && ls_rc_finite(o.v[9]);
            const float Dx = have ? p[0] - o.v[8] : 0.0f, Dy = have ? p[1] - o.v[9] : 0.0f;
            const float L = ls_sqrt_exact(Dx * Dx + Dy * Dy);
            const float h = o.v[3] + 0.5f * L * (o.v[5] + od.yaw_noise * sa);              // s0
            const float cc = ls_div_exact(1.0f, ls_sqrt_exact(1.0f + h * h));
            const LsRcV3 r = ls_rc_rot(0.0f, 0.0f, h * cc, cc, ls_rc_v3(Dx, Dy, 0.0f));
            const float k = 1.0f + (o.v[4] + od.pos_noise * sb);                             // s1
            o.v[0] = o.v[0] + (k * r.x - Dx);
            o.v[1] = o.v[1] + (k * r.y - Dy);
            o.v[2] = o.v[2] + L * (o.v[6] + od.z_noise * sc);                                // s2
            o.v[3] = h;
            o.v[8] = p[0];
            o.v[9] = p[1];
        } else {
            o.v[0] = o.v[1] = o.v[2] = o.v[3] = 0.0f;
            o.v[8] = o.v[9] = ls_odo_nan();
        }
    }
    o.v[7] = o.v[10] = o.v[11] = 0.0f;
    ls_odo_store(orow, o);
    if (finite) {
        const float h = o.v[3];
        const float cc = ls_div_exact(1.0f, ls_sqrt_exact(1.0f + h * h));
        const LsRcbQ q = ls_rcb_qmul(ls_rcb_q(0.0f, 0.0f, h * cc, cc), ls_rcb_q(p[3], p[4], p[5], p[6]));
        est[0] = p[0] + o.v[0];
        est[1] = p[1] + o.v[1];
        est[2] = p[2] + o.v[2];
        est[3] = q.x;
        est[4] = q.y;
        est[5] = q.z;
        est[6] = q.w;
    } else {
        for (int k = 0; k < 7; ++k) est[k] = p[k];
    }
    for (int k = 7; k < 13; ++k) est[k] = p[k];
}

// ---- host side: the argument check shared by the library and the CPU shim (no launch happens before it passes)
static inline int ls_odo_validate(const lsim_odometry_t* od) {
    if (!od) return LSIM_E_INVALID;
    if (!ls_rc_aligned(od->root_states, 4) || !ls_rc_aligned(od->est, 4) || !ls_rc_aligned(od->odo, 16) || !ls_rc_aligned(od->episode_length, 8)) return LSIM_E_INVALID;
    if ((const void*)od->est == (const void*)od->root_states) return LSIM_E_INVALID;
    if (od->num_envs < 1 || od->env_stride < 1 || od->tick < 0 || od->stream_id >= 65536u) return LSIM_E_INVALID;
    const float ranges[6] = {od->scale_range, od->yaw_range, od->z_range, od->pos_noise, od->yaw_noise, od->z_noise};
    for (int k = 0; k < 6; ++k) if (!ls_rc_host_finite(ranges[k]) || !(ranges[k] >= 0.0f)) return LSIM_E_INVALID;
    if (!ls_sensor_flags_ok(od->flags)) return LSIM_E_INVALID;
    return LSIM_OK;
}
static inline int ls_odo_env_slots(const lsim_odometry_t& od) { return ls_sensor_env_slots(od.num_envs, od.env_stride); }

// ------------------------------------------------------------------------------------------------ map rows
// element i of the launch: env slot i / (channels * P), column i % (channels * P)
LS_RC_FN void ls_mr_element(const lsim_map_rows_t& mr, long long i) {
    const int P = mr.num_points, cols = mr.channels * P;
    const int slot = (int)(i / (long long)cols), col = (int)(i - (long long)slot * (long long)cols);
    const size_t env = (size_t)slot * (size_t)mr.env_stride;          // < num_envs: slot <= (num_envs - 1) / env_stride
    float v;
    if (col < P) {
        const float z = mr.pose[env * (size_t)13 + 2], s = mr.scan[env * (size_t)mr.scan_stride + (size_t)col];
        const float t = z - mr.z_offset - s;
        v = (ls_rc_finite(z) && ls_rc_finite(s)) ? (t < -1.0f ? -1.0f : (t > 1.0f ? 1.0f : t)) * mr.scale : 0.0f;
    } else {
        v = mr.known[env * (size_t)mr.known_stride + (size_t)(col - P)] ? 1.0f : 0.0f;
    }
    mr.rows[env * (size_t)mr.ld + (size_t)col] = v;
}

static inline int ls_mr_validate(const lsim_map_rows_t* mr) {
    if (!mr) return LSIM_E_INVALID;
    if (!ls_rc_aligned(mr->scan, 4) || !ls_rc_aligned(mr->pose, 4) || !ls_rc_aligned(mr->rows, 4)) return LSIM_E_INVALID;
    if (mr->num_points < 1 || mr->num_points > LSIM_ELEVATION_MAP_MAX_POINTS || mr->channels < 1 || mr->channels > 2) return LSIM_E_INVALID;
    if (mr->channels == 2 && (!mr->known || mr->known_stride < mr->num_points)) return LSIM_E_INVALID;
    if (mr->scan_stride < mr->num_points || mr->ld < mr->channels * mr->num_points) return LSIM_E_INVALID;
    if (!ls_rc_host_finite(mr->z_offset) || !ls_rc_host_finite(mr->scale)) return LSIM_E_INVALID;
    if (mr->num_envs < 1 || mr->env_stride < 1) return LSIM_E_INVALID;
    return LSIM_OK;
}
static inline long long ls_mr_elements(const lsim_map_rows_t& mr) {
    return (long long)ls_sensor_env_slots(mr.num_envs, mr.env_stride) * (long long)(mr.channels * mr.num_points);
}

#if defined(__HIPCC__) && !defined(LS_EMU)
__global__ __launch_bounds__(LS_RC_BLOCK) void lsim_k_odometry_step(const lsim_odometry_t od, int slots) {
    const long long lane = (long long)blockIdx.x * LS_RC_BLOCK + (long long)threadIdx.x;
    if (lane >= (long long)slots) return;
    ls_odo_env(od, (int)lane * od.env_stride);  // < num_envs: lane <= (num_envs - 1) / env_stride
}

extern "C" int lsim_odometry_step(const lsim_odometry_t* od, void* stream) {
    const int rv = ls_odo_validate(od);
    if (rv != LSIM_OK) return rv;
    const int slots = ls_odo_env_slots(*od);
    hipLaunchKernelGGL(lsim_k_odometry_step, dim3((unsigned)(((long long)slots + LS_RC_BLOCK - 1) / LS_RC_BLOCK)), dim3(LS_RC_BLOCK), 0,
                       (hipStream_t)stream, *od, slots);
    return hipGetLastError() == hipSuccess ? LSIM_OK : LSIM_E_HIP;
}

__global__ __launch_bounds__(LS_RC_BLOCK) void lsim_k_map_rows(const lsim_map_rows_t mr, long long elements) {
    const long long i = (long long)blockIdx.x * LS_RC_BLOCK + (long long)threadIdx.x;
    if (i >= elements) return;
    ls_mr_element(mr, i);
}

extern "C" int lsim_map_rows(const lsim_map_rows_t* mr, void* stream) {
    const int rv = ls_mr_validate(mr);
    if (rv != LSIM_OK) return rv;
    const long long elements = ls_mr_elements(*mr);         // < 2^31 * 512
    const long long blocks = (elements + LS_RC_BLOCK - 1) / LS_RC_BLOCK;
    if (blocks > 0x7FFFFFFFLL) return LSIM_E_INVALID;       // more than a grid holds: only above 10^9 envs
    hipLaunchKernelGGL(lsim_k_map_rows, dim3((unsigned)blocks), dim3(LS_RC_BLOCK), 0, (hipStream_t)stream, *mr, elements);
    return hipGetLastError() == hipSuccess ? LSIM_OK : LSIM_E_HIP;
}
#endif
