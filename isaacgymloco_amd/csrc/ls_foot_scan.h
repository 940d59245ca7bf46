// ls_foot_scan.h -- foot scans (include/lsim.h, lsim_foot_scan): heights at a small pattern of points around each of the four feet, from the
// true terrain or from an elevation map, as the rows an actor reads.  lsim.h states every formula; this file is that text in code.
//
// Self-contained like ls_odometry.h (lsim.h, the vector and quaternion helpers of ls_raycast.h / ls_raycast_bodies.h, the cell helpers of
// ls_elevation_map.h, ls_math.h and the C library): tests/emu/emu_foot_scan.cpp compiles this file with g++ under LS_EMU and runs the same
// per-lane functions, the lanes looped and the LDS struct a plain struct.
//
// Shape of the launch (lsim_k_foot_scan): ONE workgroup of 256 lanes per visited env, 80 bytes of static LDS.
//   0. the pose (7 floats at an address the whole block shares) and the robot index: block-uniform;
//   1. ls_fs_fk: lanes 0..3 walk one leg's chain each (hip -> thigh -> calf -> foot) and write the foot's base-relative position and the
//      leg's non-finite-joint flag into LDS.  The recursion is lsim_raycast_bodies' WRITTEN OUT AGAIN here: routing that kernel through a
//      function shared with another caller moved its code and cost it time, and its text is not touched;
//   2. one __syncthreads(), reached by every lane (nothing before it returns or branches around it);
//   3. lane i < 4 K is point j = i % K of foot l = i / K: two LDS broadcasts-per-foot reads, the pattern offset (8 bytes), the source's
//      dependent loads (three int16 for the terrain; stamp, cell and for a known cell height for the map) and one coalesced dword store per
//      output array (lane i writes column i).
// The FK runs once per env and leg, not once per point.  Plain vector stores only; the one atomic is the bad-env counter (lane 0).
#pragma once
#include "ls_raycast_bodies.h"
#include "ls_elevation_map.h"

#define LS_FS_BLOCK 256                 // >= 4 * LSIM_FOOT_SCAN_MAX_POINTS

struct LsFsShared {
    float foot[LSIM_NUM_LEGS][4];       // F_l: base-relative, world orientation; pad
    int bad[LSIM_NUM_LEGS];             // leg l met a non-finite joint position
};

struct LsFsPose {
    float px, py, pz, qx, qy, qz, qw;   // pose[e][0:7]
    bool ok;                            // every component finite and (q.z, q.w) != (0, 0)
};

LS_RC_FN LsFsPose ls_fs_pose(const lsim_foot_scan_t& fs, int env) {
    const float* ps = fs.pose + (size_t)13 * (size_t)env;
    LsFsPose s;
    s.px = ps[0]; s.py = ps[1]; s.pz = ps[2]; s.qx = ps[3]; s.qy = ps[4]; s.qz = ps[5]; s.qw = ps[6];
    s.ok = ls_rc_finite(s.px) && ls_rc_finite(s.py) && ls_rc_finite(s.pz) && ls_rc_finite(s.qx) && ls_rc_finite(s.qy) && ls_rc_finite(s.qz) &&
           ls_rc_finite(s.qw) && !(s.qz == 0.0f && s.qw == 0.0f);
    return s;
}

LS_RC_FN int ls_fs_robot(const lsim_foot_scan_t& fs, int env) {
    int k = 0;
    if (fs.env_robot) {
        k = (int)fs.env_robot[env];
#if defined(__HIPCC__) && !defined(LS_EMU)
        k = __builtin_amdgcn_readfirstlane(k);       // env is the block's: the same for every lane
#endif
    }
    return ls_rcb_clampi(k, 0, fs.num_robots - 1);
}

// step 1, lane = leg 0..3: lsim.h's recursion down the leg's four bodies, from Q_0 = q and P_0 = 0
LS_RC_FN void ls_fs_fk(const lsim_foot_scan_t& fs, const LsFsPose& s, LsFsShared& sh, int env, int leg) {
    const lsim_raycast_robot& rob = fs.robots[ls_fs_robot(fs, env)];
    const float* th = fs.dof_state + (size_t)2 * LSIM_NUM_DOF * (size_t)env;
    LsRcbQ Q = ls_rcb_q(s.qx, s.qy, s.qz, s.qw);
    LsRcV3 P = ls_rc_v3(0.0f, 0.0f, 0.0f);
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        const lsim_raycast_body& bd = rob.bodies[1 + 4 * leg + k];
        const LsRcV3 jp = ls_rcb_qrot(Q, ls_rc_v3(bd.joint_pos[0], bd.joint_pos[1], bd.joint_pos[2]));
        P = ls_rc_v3(P.x + jp.x, P.y + jp.y, P.z + jp.z);
        if (bd.dof >= 0) {
            const float a = th[2 * ls_rcb_clampi(bd.dof, 0, LSIM_NUM_DOF - 1)];
            const float sn = sinf(0.5f * a), cs = cosf(0.5f * a);
            Q = ls_rcb_qmul(Q, ls_rcb_q(bd.joint_axis[0] * sn, bd.joint_axis[1] * sn, bd.joint_axis[2] * sn, cs));
        }
    }
    int bad = 0;
    // every dof of the env counts, also one no body of the table names
#pragma unroll 1
    for (int j = 0; j < 3; ++j) if (!ls_rc_finite(th[2 * (3 * leg + j)])) bad = 1;
    float* o = sh.foot[leg];
    o[0] = P.x; o[1] = P.y; o[2] = P.z; o[3] = 0.0f;
    sh.bad[leg] = bad;
}

// the terrain source: the reference's sampler, ls_sample_height_min3 (ls_post.h) on this struct's fields (LS_FN like it: ls_f2i is a host
// function in the compiler's host pass)
LS_FN float ls_fs_terrain(const lsim_foot_scan_t& fs, float x, float y) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (fs.mesh_type == 0) return 0.0f;
    const float fx = ls_div_exact(x + fs.border_size, fs.horizontal_scale);
    const float fy = ls_div_exact(y + fs.border_size, fs.horizontal_scale);
    int px = ls_f2i(fx), py = ls_f2i(fy);
    px = px < 0 ? 0 : (px > fs.grid_rows - 2 ? fs.grid_rows - 2 : px);
    py = py < 0 ? 0 : (py > fs.grid_cols - 2 ? fs.grid_cols - 2 : py);
    const int16_t* g = fs.height_grid;          // the largest index is (grid_rows - 1) * grid_cols + grid_cols - 2 < grid_rows * grid_cols < 2^31
    const int16_t h1 = g[px * fs.grid_cols + py], h2 = g[(px + 1) * fs.grid_cols + py], h3 = g[px * fs.grid_cols + py + 1];
    int16_t h = h1 < h2 ? h1 : h2;
    h = h < h3 ? h : h3;
    return (float)h * fs.vertical_scale;
}

// the map source: lsim_elevation_map's lookup (ls_em_lookup) at a point that is given; false: unknown
LS_RC_FN bool ls_fs_map(const lsim_foot_scan_t& fs, int env, float x, float y, float rinv, float& h) {
    if (!ls_rc_finite(x) || !ls_rc_finite(y)) return false;
    const float fx = ls_em_cellf(x, rinv), fy = ls_em_cellf(y, rinv);
    if (!ls_em_in_range(fx) || !ls_em_in_range(fy)) return false;
    const int ix = (int)fx, iy = (int)fy;
    const size_t at = (size_t)env * (size_t)(fs.size * fs.size) + (size_t)ls_em_slot(ix, iy, fs.size);
    if (!(fs.stamp[at] >= 0 && fs.cell[at] == ls_em_pack(ix, iy))) return false;
    h = fs.height[at];
    return true;
}

// step 3, lane i < 4 K: point i % K of foot i / K
LS_RC_FN void ls_fs_point(const lsim_foot_scan_t& fs, const LsFsPose& s, const LsFsShared& sh, int env, int i, float rinv) {
    const int K = fs.num_points, K4 = 4 * K;
    float* rows = fs.rows + (size_t)env * (size_t)fs.ld;
    const bool ok = s.ok && (sh.bad[0] | sh.bad[1] | sh.bad[2] | sh.bad[3]) == 0;
    float v = 0.0f, h = 0.0f;
    bool kn = false;
    if (ok) {
        const int l = i / K, j = i - l * K;
        const float* F = sh.foot[l];
        const float n = ls_div_exact(1.0f, ls_sqrt_exact(s.qz * s.qz + s.qw * s.qw));
        const LsRcV3 o = ls_rc_rot(0.0f, 0.0f, s.qz * n, s.qw * n, ls_rc_v3(fs.pattern[2 * j], fs.pattern[2 * j + 1], 0.0f));
        const float wx = (s.px + F[0]) + o.x, wy = (s.py + F[1]) + o.y;
        if (fs.source == LSIM_FOOT_SCAN_TERRAIN) {
            h = ls_fs_terrain(fs, wx, wy);
            kn = true;
        } else {
            h = s.pz - fs.unknown_drop;
            kn = ls_fs_map(fs, env, wx, wy, rinv, h);
        }
        const float t = ((s.pz + F[2]) - fs.z_offset) - h;
        v = ls_rc_finite(t) ? (t < -1.0f ? -1.0f : (t > 1.0f ? 1.0f : t)) * fs.scale : 0.0f;
    }
    rows[i] = v;
    if (fs.channels == 2) rows[K4 + i] = kn ? 1.0f : 0.0f;
    if (fs.heights) fs.heights[(size_t)env * (size_t)fs.heights_stride + (size_t)i] = h;
    if (fs.known) fs.known[(size_t)env * (size_t)fs.known_stride + (size_t)i] = kn ? (uint8_t)1 : (uint8_t)0;
}

// ---- host side: the argument check shared by the library and the CPU shim (no launch happens before it passes)
static inline int ls_fs_validate(const lsim_foot_scan_t* fs) {
    if (!fs) return LSIM_E_INVALID;
    if (!ls_rc_aligned(fs->pose, 4) || !ls_rc_aligned(fs->dof_state, 4) || !ls_rc_aligned(fs->robots, 4) || !ls_rc_aligned(fs->robots_host, 4) ||
        !ls_rc_aligned(fs->pattern, 4) || !ls_rc_aligned(fs->rows, 4) || !ls_rc_aligned(fs->state, 8)) return LSIM_E_INVALID;
    if (fs->heights && !ls_rc_aligned(fs->heights, 4)) return LSIM_E_INVALID;
    if (fs->source != LSIM_FOOT_SCAN_TERRAIN && fs->source != LSIM_FOOT_SCAN_MAP) return LSIM_E_INVALID;
    if (fs->num_envs < 1 || fs->env_stride < 1) return LSIM_E_INVALID;
    if (fs->num_robots < 1 || fs->num_robots > LSIM_MAX_ROBOTS || (!fs->env_robot && fs->num_robots != 1)) return LSIM_E_INVALID;
    if (fs->num_points < 1 || fs->num_points > LSIM_FOOT_SCAN_MAX_POINTS || fs->channels < 1 || fs->channels > 2) return LSIM_E_INVALID;
    const int K4 = 4 * fs->num_points;
    if (fs->ld < fs->channels * K4 || (fs->heights && fs->heights_stride < K4) || (fs->known && fs->known_stride < K4)) return LSIM_E_INVALID;
    if (!ls_rc_host_finite(fs->z_offset) || !ls_rc_host_finite(fs->scale)) return LSIM_E_INVALID;
    if (fs->source == LSIM_FOOT_SCAN_TERRAIN) {
        if (fs->mesh_type != 0) {
            if (!ls_rc_aligned(fs->height_grid, 2) || fs->grid_rows < 2 || fs->grid_cols < 2 ||
                (long long)fs->grid_rows * (long long)fs->grid_cols > 0x7FFFFFFFLL) return LSIM_E_INVALID;
            if (!ls_rc_host_finite(fs->horizontal_scale) || !(fs->horizontal_scale > 0.0f) || !ls_rc_host_finite(fs->vertical_scale) ||
                !(fs->vertical_scale > 0.0f) || !ls_rc_host_finite(fs->border_size)) return LSIM_E_INVALID;
        }
    } else {
        if (!ls_rc_aligned(fs->height, 4) || !ls_rc_aligned(fs->stamp, 4) || !ls_rc_aligned(fs->cell, 4)) return LSIM_E_INVALID;
        if (fs->size != 16 && fs->size != 32 && fs->size != 64) return LSIM_E_INVALID;
        if (!ls_rc_host_finite(fs->res) || !(fs->res > 0.0f) || !ls_rc_host_finite(fs->unknown_drop)) return LSIM_E_INVALID;
    }
    for (int k = 0; k < fs->num_robots; ++k) {
        const lsim_raycast_robot& rob = fs->robots_host[k];
        for (int b = 0; b < LSIM_NUM_BODIES; ++b) {          // the tree ls_rcb_validate accepts
            const lsim_raycast_body& bd = rob.bodies[b];
            const int parent = b == 0 ? -1 : ((b - 1) % 4 == 0 ? 0 : b - 1);
            if (bd.parent != parent || bd.dof < -1 || bd.dof >= LSIM_NUM_DOF || (b == 0 && bd.dof != -1)) return LSIM_E_INVALID;
            if (!ls_rcb_host_finite3(bd.joint_pos, 3) || !ls_rcb_host_finite3(bd.joint_axis, 3)) return LSIM_E_INVALID;
        }
    }
    return LSIM_OK;
}
static inline int ls_fs_env_slots(const lsim_foot_scan_t& fs) { return ls_sensor_env_slots(fs.num_envs, fs.env_stride); }
static inline float ls_fs_rinv(const lsim_foot_scan_t& fs) { return fs.source == LSIM_FOOT_SCAN_MAP ? (float)(1.0 / (double)fs.res) : 0.0f; }

#if defined(__HIPCC__) && !defined(LS_EMU)
__global__ __launch_bounds__(LS_FS_BLOCK) void lsim_k_foot_scan(const lsim_foot_scan_t fs, float rinv) {
    __shared__ LsFsShared sh;
    const int env = (int)blockIdx.x * fs.env_stride, lane = (int)threadIdx.x;      // < num_envs: blockIdx.x <= (num_envs - 1) / env_stride
    const LsFsPose s = ls_fs_pose(fs, env);
    if (lane < LSIM_NUM_LEGS) ls_fs_fk(fs, s, sh, env, lane);
    __syncthreads();
    if (lane == 0 && !(s.ok && (sh.bad[0] | sh.bad[1] | sh.bad[2] | sh.bad[3]) == 0)) ls_rc_count((long long*)fs.state, 1);
    if (lane < 4 * fs.num_points) ls_fs_point(fs, s, sh, env, lane, rinv);
}

extern "C" int lsim_foot_scan(const lsim_foot_scan_t* fs, void* stream) {
    const int rv = ls_fs_validate(fs);
    if (rv != LSIM_OK) return rv;
    hipLaunchKernelGGL(lsim_k_foot_scan, dim3((unsigned)ls_fs_env_slots(*fs)), dim3(LS_FS_BLOCK), 0, (hipStream_t)stream, *fs, ls_fs_rinv(*fs));
    return hipGetLastError() == hipSuccess ? LSIM_OK : LSIM_E_HIP;
}
#endif
