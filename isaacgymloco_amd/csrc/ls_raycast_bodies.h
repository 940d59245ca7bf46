// ls_raycast_bodies.h -- range sensors that also see the env's own robot (include/lsim.h, lsim_raycast_bodies): the terrain walk of
// ls_raycast.h plus the articulated collision primitives of the robot, one launch for all envs and rays.
//
// Self-contained like ls_raycast.h (only lsim.h, ls_raycast.h and the C library): tests/emu/emu_raycast_bodies.cpp compiles this file with g++
// under LS_EMU and runs the same per-block and per-ray code over plain arrays.
//
// Shape of the launch (lsim_k_raycast_bodies): lsim_k_raycast's -- blocks of 256 lanes over the rays of ONE env, lane = ray -- with a prologue:
//   1. ls_rcb_fk: lanes 0..3 walk one leg's chain each (base -> hip -> thigh -> calf -> foot) from root_states and dof_state and write the 17
//      body poses, relative to the base position, into LDS (lane 0 writes the base's too);
//   2. ls_rcb_prim: one lane per primitive turns (body pose, primitive pose) into a base-relative centre, world-oriented axes, sizes and a
//      bounding radius in LDS (48 x 16 floats = 3 KB); a primitive of a masked body gets kind -1.
//   A __syncthreads() after each (2 reads what 1 wrote): ls_rcb_block, which lsim_k_sensor_capture and lsim_k_sensor_capture_inst call too.
//   Both steps are a few hundred instructions of ONE wave per block, against 256 rays.
//   3. ls_rcb_ray (this launch) and ls_rcb_value (the same ray for the two capture launches, which hand it the direction and scale to cast:
//      one function where there were two; why ls_rcb_ray is not its third caller stands above ls_rcb_ray): a rolled loop over the primitives.  The primitive index is wave-uniform, so every lane reads the same LDS address (a broadcast,
//      no bank conflict) and the switch on `kind` does not diverge.  A bounding-sphere test rejects most primitives before the exact one.  The
//      smallest body hit then becomes `far` of the terrain walk (ls_rc_cast, shared with lsim_raycast and not changed: the walk takes its bounds
//      from the struct it is given, and this kernel hands it a copy with the shorter `far`), so a ray that ends on a thigh walks no cell behind it.
// The body test runs in coordinates relative to the base position (lsim.h says why): o' = R(q) mount_pos, never p + ... - p.
#pragma once
#include "ls_raycast.h"

#define LS_RCB_PRIM_WORDS 16            // centre 3, axes 9 (row k = local axis k in world orientation), size 3, bounding radius
#define LS_RCB_BODY_WORDS 8             // position 3, quaternion 4, pad

struct LsRcbShared {
    float body[LSIM_NUM_BODIES][LS_RCB_BODY_WORDS];
    float prim[LSIM_RAYCAST_MAX_PRIMS][LS_RCB_PRIM_WORDS];
    int kind[LSIM_RAYCAST_MAX_PRIMS];   // kind | body << 8, or -1: not seen
    int bad[LSIM_NUM_LEGS];             // leg l met a non-finite joint position
    int nprims;
};

struct LsRcbQ { float x, y, z, w; };
LS_RC_FN LsRcbQ ls_rcb_q(float x, float y, float z, float w) { LsRcbQ q; q.x = x; q.y = y; q.z = z; q.w = w; return q; }
// a * b: R(a * b) = R(a) R(b)
LS_RC_FN LsRcbQ ls_rcb_qmul(LsRcbQ a, LsRcbQ b) {
    return ls_rcb_q(a.w * b.x + b.w * a.x + (a.y * b.z - a.z * b.y), a.w * b.y + b.w * a.y + (a.z * b.x - a.x * b.z),
                    a.w * b.z + b.w * a.z + (a.x * b.y - a.y * b.x), a.w * b.w - (a.x * b.x + a.y * b.y + a.z * b.z));
}
LS_RC_FN LsRcV3 ls_rcb_qrot(LsRcbQ q, LsRcV3 v) { return ls_rc_rot(q.x, q.y, q.z, q.w, v); }
LS_RC_FN int ls_rcb_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

LS_RC_FN int ls_rcb_robot(const lsim_raycast_bodies_t& rb, int env) {
    int k = 0;
    if (rb.env_robot) {
        k = (int)rb.env_robot[env];
#if defined(__HIPCC__) && !defined(LS_EMU)
        k = __builtin_amdgcn_readfirstlane(k);       // env is the block's: the same for every lane (as ls_env_robot)
#endif
    }
    return ls_rcb_clampi(k, 0, rb.num_robots - 1);
}

// step 1, lane = leg 0..3: the poses of the leg's four bodies (lane 0: the base's too), base-relative position and world orientation
LS_RC_FN void ls_rcb_fk(const lsim_raycast_bodies_t& rb, LsRcbShared& sh, int env, int leg) {
    const lsim_raycast_robot& rob = rb.robots[ls_rcb_robot(rb, env)];
    const float* rs = rb.rc.root_states + (size_t)13 * (size_t)env;
    const float* th = rb.dof_state + (size_t)2 * LSIM_NUM_DOF * (size_t)env;
    LsRcbQ Q = ls_rcb_q(rs[3], rs[4], rs[5], rs[6]);
    LsRcV3 P = ls_rc_v3(0.0f, 0.0f, 0.0f);
    if (leg == 0) {
        float* b0 = sh.body[0];
        b0[0] = 0.0f; b0[1] = 0.0f; b0[2] = 0.0f; b0[3] = Q.x; b0[4] = Q.y; b0[5] = Q.z; b0[6] = Q.w;
        int np = rob.num_prims;
        sh.nprims = ls_rcb_clampi(np, 0, LSIM_RAYCAST_MAX_PRIMS);
    }
    int bad = 0;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        const int b = 1 + 4 * leg + k;
        const lsim_raycast_body& bd = rob.bodies[b];
        const LsRcV3 jp = ls_rcb_qrot(Q, ls_rc_v3(bd.joint_pos[0], bd.joint_pos[1], bd.joint_pos[2]));
        P = ls_rc_v3(P.x + jp.x, P.y + jp.y, P.z + jp.z);
        if (bd.dof >= 0) {
            const float a = th[2 * ls_rcb_clampi(bd.dof, 0, LSIM_NUM_DOF - 1)];
            if (!ls_rc_finite(a)) bad = 1;
            const float s = sinf(0.5f * a), c = cosf(0.5f * a);
            Q = ls_rcb_qmul(Q, ls_rcb_q(bd.joint_axis[0] * s, bd.joint_axis[1] * s, bd.joint_axis[2] * s, c));
        }
        float* o = sh.body[b];
        o[0] = P.x; o[1] = P.y; o[2] = P.z; o[3] = Q.x; o[4] = Q.y; o[5] = Q.z; o[6] = Q.w;
    }
    // every dof of the env counts, also one no body of the table names
#pragma unroll 1
    for (int j = 0; j < 3; ++j) if (!ls_rc_finite(th[2 * (3 * leg + j)])) bad = 1;
    sh.bad[leg] = bad;
}

// step 2, lane = primitive i < sh.nprims
LS_RC_FN void ls_rcb_prim(const lsim_raycast_bodies_t& rb, LsRcbShared& sh, int env, int i) {
    const lsim_raycast_prim& pr = rb.robots[ls_rcb_robot(rb, env)].prims[i];
    const int body = ls_rcb_clampi(pr.body, 0, LSIM_NUM_BODIES - 1);
    const int kind = pr.kind;
    if (!((rb.body_mask >> body) & 1u) || kind < 0 || kind > LSIM_RAYCAST_PRIM_CYLINDER) { sh.kind[i] = -1; return; }
    const float* bp = sh.body[body];
    const LsRcbQ Qb = ls_rcb_q(bp[3], bp[4], bp[5], bp[6]);
    const LsRcV3 c = ls_rcb_qrot(Qb, ls_rc_v3(pr.pos[0], pr.pos[1], pr.pos[2]));
    const LsRcbQ Q = ls_rcb_qmul(Qb, ls_rcb_q(pr.quat[0], pr.quat[1], pr.quat[2], pr.quat[3]));
    float* o = sh.prim[i];
    o[0] = bp[0] + c.x; o[1] = bp[1] + c.y; o[2] = bp[2] + c.z;
    const LsRcV3 ax = ls_rcb_qrot(Q, ls_rc_v3(1.0f, 0.0f, 0.0f)), ay = ls_rcb_qrot(Q, ls_rc_v3(0.0f, 1.0f, 0.0f)), az = ls_rcb_qrot(Q, ls_rc_v3(0.0f, 0.0f, 1.0f));
    o[3] = ax.x; o[4] = ax.y; o[5] = ax.z; o[6] = ay.x; o[7] = ay.y; o[8] = ay.z; o[9] = az.x; o[10] = az.y; o[11] = az.z;
    const float s0 = pr.size[0], s1 = pr.size[1], s2 = pr.size[2];
    o[12] = s0; o[13] = s1; o[14] = s2;
    float br;
    if (kind == LSIM_RAYCAST_PRIM_SPHERE) br = s0;
    else if (kind == LSIM_RAYCAST_PRIM_BOX) br = sqrtf(s0 * s0 + s1 * s1 + s2 * s2);
    else if (kind == LSIM_RAYCAST_PRIM_CAPSULE) br = s0 + s1;
    else br = sqrtf(s0 * s0 + s1 * s1);
    o[15] = br * 1.001f + 1e-6f;        // the rejection must never cut a hit the exact test would find: far more than the rounding of the two sides
    sh.kind[i] = kind | (body << 8);
}

// [t0, t1]: the t with a t^2 + 2 b t + c <= 0 (a >= 0); empty: t0 > t1.  The smaller root without cancellation when b < 0, c > 0 (the sensor
// outside, looking at the shape: the case that is reported)
LS_RC_FN void ls_rcb_quad(float a, float b, float c, float& t0, float& t1) {
    t0 = LS_RC_BIG; t1 = -LS_RC_BIG;
    if (a < 1e-30f) {                   // no quadratic term (a ray along a cylinder's axis): inside for all t, or for none
        if (c <= 0.0f) { t0 = -LS_RC_BIG; t1 = LS_RC_BIG; }
        return;
    }
    const float disc = b * b - a * c;
    if (!(disc >= 0.0f)) return;
    const float sq = sqrtf(disc);
    if (b < 0.0f) { const float q = sq - b; t0 = c / q; t1 = q / a; }
    else { const float q = -b - sq; t0 = q / a; t1 = (q != 0.0f) ? c / q : 0.0f; }
}

// t_in of one primitive in its own frame (origin o, direction d in local axes), LS_RC_BIG when the line misses it
LS_RC_FN float ls_rcb_entry(int kind, LsRcV3 o, LsRcV3 d, float s0, float s1, float s2) {
    float t0, t1;
    if (kind == LSIM_RAYCAST_PRIM_BOX) {
        t0 = -LS_RC_BIG; t1 = LS_RC_BIG;
        const float oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z}, hh[3] = {s0, s1, s2};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (fabsf(dd[k]) >= 1e-30f) {
                const float inv = 1.0f / dd[k];
                const float ta = (-hh[k] - oo[k]) * inv, tb = (hh[k] - oo[k]) * inv;
                t0 = fmaxf(t0, fminf(ta, tb)); t1 = fminf(t1, fmaxf(ta, tb));
            } else if (fabsf(oo[k]) > hh[k]) {
                return LS_RC_BIG;
            }
        }
        return t0 <= t1 ? t0 : LS_RC_BIG;
    }
    if (kind == LSIM_RAYCAST_PRIM_SPHERE) {
        ls_rcb_quad(ls_rc_dot(d, d), ls_rc_dot(o, d), ls_rc_dot(o, o) - s0 * s0, t0, t1);
        return t0 <= t1 ? t0 : LS_RC_BIG;
    }
    // the flat-capped cylinder: (infinite cylinder) and (slab |z| <= h)
    ls_rcb_quad(d.x * d.x + d.y * d.y, o.x * d.x + o.y * d.y, o.x * o.x + o.y * o.y - s0 * s0, t0, t1);
    if (fabsf(d.z) >= 1e-30f) {
        const float inv = 1.0f / d.z;
        const float ta = (-s1 - o.z) * inv, tb = (s1 - o.z) * inv;
        t0 = fmaxf(t0, fminf(ta, tb)); t1 = fminf(t1, fmaxf(ta, tb));
    } else if (fabsf(o.z) > s1) {
        t1 = -LS_RC_BIG;
    }
    float tin = t0 <= t1 ? t0 : LS_RC_BIG;
    if (kind == LSIM_RAYCAST_PRIM_CAPSULE) {
        // the capsule is the union of that cylinder and the two end spheres; the union is convex, so its interval starts at the smallest t_in
        const float dd = ls_rc_dot(d, d), r2 = s0 * s0;
#pragma unroll 1
        for (int e = 0; e < 2; ++e) {
            const LsRcV3 oe = ls_rc_v3(o.x, o.y, o.z + (e == 0 ? s1 : -s1));
            ls_rcb_quad(dd, ls_rc_dot(oe, d), ls_rc_dot(oe, oe) - r2, t0, t1);
            if (t0 <= t1) tin = fminf(tin, t0);
        }
    }
    return tin;
}

// the smallest contributed t_in over the seen primitives (or `far`), in base-relative coordinates; label = 2 + body of the winner, 0 if none
LS_RC_FN float ls_rcb_cast(const LsRcbShared& sh, LsRcV3 o, LsRcV3 d, float near, float far, int& label, int& tested) {
    float best = far;
    label = 0;
    const float dd = ls_rc_dot(d, d);
    const int n = sh.nprims;
#pragma unroll 1
    for (int i = 0; i < n; ++i) {
        const int kb = sh.kind[i];
        if (kb < 0) continue;
        const float* p = sh.prim[i];
        const LsRcV3 v = ls_rc_v3(o.x - p[0], o.y - p[1], o.z - p[2]);
        const float vd = ls_rc_dot(v, d), br = p[15];
        // the line's squared distance to the centre, times |d|^2, against the bounding radius
        if (ls_rc_dot(v, v) * dd - vd * vd > br * br * dd) continue;
        tested += 1;
        const LsRcV3 ol = ls_rc_v3(v.x * p[3] + v.y * p[4] + v.z * p[5], v.x * p[6] + v.y * p[7] + v.z * p[8], v.x * p[9] + v.y * p[10] + v.z * p[11]);
        const LsRcV3 dl = ls_rc_v3(d.x * p[3] + d.y * p[4] + d.z * p[5], d.x * p[6] + d.y * p[7] + d.z * p[8], d.x * p[9] + d.y * p[10] + d.z * p[11]);
        const float t = ls_rcb_entry(kb & 0xFF, ol, dl, p[12], p[13], p[14]);
        if (t >= near && t <= far && (t < best || label == 0)) { best = t; label = 2 + (kb >> 8); }
    }
    return best;
}

// The body ray of the two captures: the scaled range and the label of one ray of env -- pose (yaw frame if asked), bodies, terrain up to the
// body hit, scale; hit = (t < far).  `s` and `sc` as ls_rc_value's: where the ray's sensor-frame direction and its scale (NULL: 1) are read.
// lsim_k_sensor_capture, lsim_k_sensor_capture_inst and their CPU shims call it; ls_rcb_ray below does NOT (its comment says why), so a change
// to the pose convention, the non-finite rule, the counters or the tie rule is made here and there.
LS_RC_FN float ls_rcb_value(const lsim_raycast_bodies_t& rb, const LsRcbShared& sh, int env, const float* s, const float* sc, bool& hit, int& label) {
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
    const LsRcV3 ds = ls_rc_rot(mt[3], mt[4], mt[5], mt[6], ls_rc_v3(s[0], s[1], s[2]));
    const LsRcV3 d = ls_rc_rot(qx, qy, qz, qw, ds);
    const float scale = sc ? *sc : 1.0f;
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
        if (t < tb) label = 1;                  // a tie: the body keeps the label; no body and t == far: a miss, label 0
#if defined(LS_RAYCAST_COUNTERS)
        ls_rc_count(state + 1, tested);
        ls_rc_count(state + 2, cnt.cells);
        ls_rc_count(state + 3, cnt.tris);
#endif
    } else {
        ls_rc_count(state, 1);
    }
    hit = t < rc.far;
    return t * scale;
}

// ray r of env: pose, bodies, terrain up to the body hit, scale, store.  The text of ls_rcb_value at the tables' direction and scale, kept as
// text: through the function (the label then reaches ls_rcb_cast by two references instead of one) the compiler turns the tie rule's select
// into a branch and moves a block of the primitive loop, 5 instructions more, and lsim_raycast_bodies measured 0.13 - 0.49 % over the
// parent's slowest run on three of four workloads, in two sessions; with the label in a local of ls_rcb_value this kernel came out
// instruction-identical and lsim_sensor_capture 0.6 - 1.0 % slower on flat ground instead (profiles/raycast_refactor_ab.json).
// The bit-for-bit tests capture(identity) == lsim_raycast_bodies pin the two texts to each other.
LS_RC_FN void ls_rcb_ray(const lsim_raycast_bodies_t& rb, const LsRcbShared& sh, int env, int r) {
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
    int label = 0;
    const bool joints_ok = (sh.bad[0] | sh.bad[1] | sh.bad[2] | sh.bad[3]) == 0;
    if (joints_ok && ls_rc_finite(o.x) && ls_rc_finite(o.y) && ls_rc_finite(o.z) && ls_rc_finite(d.x) && ls_rc_finite(d.y) && ls_rc_finite(d.z)) {
        LsRcCount cnt;
        cnt.cells = 0; cnt.tris = 0;
        int tested = 0;
        const float tb = ls_rcb_cast(sh, mp, d, rc.near, rc.far, label, tested);
        lsim_raycast_t walk = rc;               // the shared walk, bounded by the body hit
        walk.far = tb;
        t = ls_rc_cast(walk, o, d, cnt);
        if (t < tb) label = 1;                  // a tie: the body keeps the label; no body and t == far: a miss, label 0
#if defined(LS_RAYCAST_COUNTERS)
        ls_rc_count(state + 1, tested);
        ls_rc_count(state + 2, cnt.cells);
        ls_rc_count(state + 3, cnt.tris);
#endif
    } else {
        ls_rc_count(state, 1);
    }
    rc.out[(size_t)env * (size_t)rc.out_stride + (size_t)r] = t * sc;
    if (rb.labels) rb.labels[(size_t)env * (size_t)rb.label_stride + (size_t)r] = (uint8_t)label;
}

// ---- host side: argument checks shared by the library and the CPU shim (no launch happens before they pass)
static inline bool ls_rcb_host_finite3(const float* v, int n) {
    for (int k = 0; k < n; ++k) if (!ls_rc_host_finite(v[k])) return false;
    return true;
}
static inline int ls_rcb_validate(const lsim_raycast_bodies_t* rb) {
    if (!rb) return LSIM_E_INVALID;
    const int rv = ls_rc_validate(&rb->rc);
    if (rv != LSIM_OK) return rv;
    if (!ls_rc_aligned(rb->dof_state, 4) || !ls_rc_aligned(rb->robots, 4) || !ls_rc_aligned(rb->robots_host, 4)) return LSIM_E_INVALID;
    if (rb->num_robots < 1 || rb->num_robots > LSIM_MAX_ROBOTS || (!rb->env_robot && rb->num_robots != 1)) return LSIM_E_INVALID;
    if (rb->labels && rb->label_stride < rb->rc.num_rays) return LSIM_E_INVALID;
    if (rb->flags & ~(uint32_t)LSIM_RAYCAST_FRAME_YAW) return LSIM_E_INVALID;
    for (int k = 0; k < rb->num_robots; ++k) {
        const lsim_raycast_robot& rob = rb->robots_host[k];
        if (rob.num_prims < 0 || rob.num_prims > LSIM_RAYCAST_MAX_PRIMS) return LSIM_E_INVALID;
        for (int b = 0; b < LSIM_NUM_BODIES; ++b) {
            const lsim_raycast_body& bd = rob.bodies[b];
            const int parent = b == 0 ? -1 : ((b - 1) % 4 == 0 ? 0 : b - 1);
            if (bd.parent != parent || bd.dof < -1 || bd.dof >= LSIM_NUM_DOF || (b == 0 && bd.dof != -1)) return LSIM_E_INVALID;
            if (!ls_rcb_host_finite3(bd.joint_pos, 3) || !ls_rcb_host_finite3(bd.joint_axis, 3)) return LSIM_E_INVALID;
        }
        for (int i = 0; i < rob.num_prims; ++i) {
            const lsim_raycast_prim& pr = rob.prims[i];
            if (pr.kind < LSIM_RAYCAST_PRIM_SPHERE || pr.kind > LSIM_RAYCAST_PRIM_CYLINDER || pr.body < 0 || pr.body >= LSIM_NUM_BODIES) return LSIM_E_INVALID;
            if (!ls_rcb_host_finite3(pr.pos, 3) || !ls_rcb_host_finite3(pr.quat, 4)) return LSIM_E_INVALID;
            const int used = pr.kind == LSIM_RAYCAST_PRIM_SPHERE ? 1 : (pr.kind == LSIM_RAYCAST_PRIM_BOX ? 3 : 2);
            for (int s = 0; s < used; ++s) if (!ls_rc_host_finite(pr.size[s]) || !(pr.size[s] > 0.0f)) return LSIM_E_INVALID;
        }
    }
    return LSIM_OK;
}

#if defined(__HIPCC__) && !defined(LS_EMU)
// steps 1 and 2 with their barriers: every lane of the block enters (the three kernels that see the robot return whole blocks only, before this)
__device__ __forceinline__ void ls_rcb_block(const lsim_raycast_bodies_t& rb, LsRcbShared& sh, int env, int lane) {
    if (lane < LSIM_NUM_LEGS) ls_rcb_fk(rb, sh, env, lane);
    __syncthreads();
    if (lane < sh.nprims) ls_rcb_prim(rb, sh, env, lane);
    __syncthreads();
}

__global__ __launch_bounds__(LS_RC_BLOCK) void lsim_k_raycast_bodies(const lsim_raycast_bodies_t rb, int blocks_per_env) {
    __shared__ LsRcbShared sh;
    int env, r;
    ls_rc_block(rb.rc, blocks_per_env, env, r);
    if (env >= rb.rc.num_envs) return;          // the whole block: env is blockIdx's
    ls_rcb_block(rb, sh, env, (int)threadIdx.x);
    if (r < rb.rc.num_rays) ls_rcb_ray(rb, sh, env, r);
}

extern "C" int lsim_raycast_bodies_sizes(size_t* state_bytes, size_t* robot_bytes) {
    if (!state_bytes || !robot_bytes) return LSIM_E_INVALID;
    *state_bytes = LSIM_RAYCAST_STATE_WORDS * sizeof(int64_t);
    *robot_bytes = sizeof(lsim_raycast_robot);
    return LSIM_OK;
}
extern "C" int lsim_raycast_bodies(const lsim_raycast_bodies_t* rb, void* stream) {
    const int rv = ls_rcb_validate(rb);
    if (rv != LSIM_OK) return rv;
    int bpe;
    unsigned blocks;
    if (!ls_rc_grid(rb->rc, bpe, blocks)) return LSIM_E_INVALID;
    hipLaunchKernelGGL(lsim_k_raycast_bodies, dim3(blocks), dim3(LS_RC_BLOCK), 0, (hipStream_t)stream, *rb, bpe);
    return hipGetLastError() == hipSuccess ? LSIM_OK : LSIM_E_HIP;
}
#endif
