"""TEST INFRASTRUCTURE -- float64 reference of the body-aware range sensor (include/lsim.h, lsim_raycast_bodies), written from the header alone.

Forward kinematics from the same float32 inputs (root_states, dof_state, the lsim_raycast_robot table), every primitive posed, and for every
ray the analytic interval [t_in, t_out] of each of the four kinds (sphere and cylinder: roots of the quadratic; box and the cylinder's caps:
slabs; capsule: the convex union of a cylinder and two spheres, so the smallest t_in of the three), all in float64 and in the base-relative
frame the header prescribes; then the minimum with the terrain brute force of tests/raycast_reference.py.  It shares no code with the kernel: no
bounding test, no LDS layout, no shortened terrain walk.

Acceptance (`check`) is the rule of tests/raycast_reference.py, unchanged, with its constants EPS_POS, EPS_ANG, C_TOL, ATOL, MAX_UNSTABLE: the
value under test must lie in the envelope of nine float64 evaluations (the ray, and origin / direction moved by +-EPS_POS / +-EPS_ANG along two
transverse axes -- the robot stays where it is), each widened by tol_k = ATOL + C * 2^-23 * (max|coordinate| + t_k) / |n_k . d_k|.  For a sample
that ends on a body, max|coordinate| is taken in the base-relative frame the body test runs in (the origin R(q) mount_pos and the hit point,
under a metre) and n_k is the primitive's outward normal at the entry point; for one that ends on the terrain both are raycast_reference's.
Why C = 16 also covers a body hit: the base-relative centre of a primitive is a sum of at most five rotated offsets (four joints and the
primitive's own), each a rotation by a quaternion that is itself the product of at most four fp32 quaternions (sinf / cosf of half the joint
angle: 1-2 u each): about 5 x (3 roundings of the sum + 4 u of the rotation) = 35 u at the magnitude of ONE offset (0.25 m), i.e. under 9 u of
a 1 m coordinate; the world-to-primitive rotation of o' and d adds 3 u; the quadratic (a, b, c: three dot products, b^2 - a c, the root without
cancellation) or the slab quotient adds about 8 u on the t term.  Roughly 12 u on the coordinate term and 8 u on t, in units of u = 2^-24: 6 and 4
times 2^-23 -- below the 16 that the terrain's own count was rounded up to, so the constant stays.
A label is compared wherever the nine evaluations agree on it; a ray on which they do not agree is unstable (it lies within the steps of a
silhouette, or of the curve where a shape meets the ground) and counts against the same MAX_UNSTABLE.
"""
import numpy as np

import raycast_reference as REF

SPHERE, BOX, CAPSULE, CYLINDER = 0, 1, 2, 3
FRAME_YAW = 1


def qmul(a, b):
    """a * b with R(a * b) = R(a) R(b), xyzw"""
    av, aw, bv, bw = a[..., :3], a[..., 3:4], b[..., :3], b[..., 3:4]
    return np.concatenate((aw * bv + bw * av + np.cross(av, bv), aw * bw - (av * bv).sum(-1, keepdims=True)), axis=-1)


def robot_dict(table):
    """plain float64 arrays of an lsim_raycast_robot (ctypes)"""
    bodies = [dict(joint_pos=np.array(list(b.joint_pos), np.float64), axis=np.array(list(b.joint_axis), np.float64), parent=int(b.parent), dof=int(b.dof))
              for b in table.bodies]
    prims = [dict(kind=int(p.kind), body=int(p.body), pos=np.array(list(p.pos), np.float64), quat=np.array(list(p.quat), np.float64),
                  size=np.array(list(p.size), np.float64)) for p in list(table.prims)[:table.num_prims]]
    return {"bodies": bodies, "prims": prims}


def fk(robot, quat, theta):
    """(P [17, 3] relative to the base position, Q [17, 4]) of one env: quat [4] the base's, theta [12]"""
    P, Q = np.zeros((17, 3)), np.zeros((17, 4))
    Q[0] = quat
    for b in range(1, 17):
        bd = robot["bodies"][b]
        a = bd["parent"]
        P[b] = P[a] + REF.quat_rotate(Q[a], bd["joint_pos"])
        th = theta[bd["dof"]] if bd["dof"] >= 0 else 0.0
        Q[b] = qmul(Q[a], np.concatenate((bd["axis"] * np.sin(0.5 * th), [np.cos(0.5 * th)])))
    return P, Q


def _quad(a, b, c):
    """[t0, t1] with a t^2 + 2 b t + c <= 0; empty: (inf, -inf)"""
    t0, t1 = np.full(a.shape, np.inf), np.full(a.shape, -np.inf)
    disc = b * b - a * c
    ok = (a > 1e-300) & (disc >= 0)
    sq = np.sqrt(np.where(ok, disc, 0.0))
    sa = np.where(ok, a, 1.0)
    t0, t1 = np.where(ok, (-b - sq) / sa, t0), np.where(ok, (-b + sq) / sa, t1)
    flat = ~(a > 1e-300) & (c <= 0)
    return np.where(flat, -np.inf, t0), np.where(flat, np.inf, t1)


def _slab(o, d, h):
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = (-h - o) / d, (h - o) / d
    lo, hi = np.minimum(ta, tb), np.maximum(ta, tb)
    par = np.abs(d) < 1e-300
    inside = np.abs(o) <= h
    return np.where(par, np.where(inside, -np.inf, np.inf), lo), np.where(par, np.where(inside, np.inf, -np.inf), hi)


def _sphere(o, d, r):
    t0, t1 = _quad((d * d).sum(-1), (o * d).sum(-1), (o * o).sum(-1) - r * r)
    hit = t0 <= t1
    tt = np.where(hit & np.isfinite(t0), t0, 0.0)
    n = (o + tt[..., None] * d) / r
    return np.where(hit, t0, np.inf), n


def _cylinder(o, d, r, h):
    s0, s1 = _quad(d[..., 0] ** 2 + d[..., 1] ** 2, o[..., 0] * d[..., 0] + o[..., 1] * d[..., 1], o[..., 0] ** 2 + o[..., 1] ** 2 - r * r)
    z0, z1 = _slab(o[..., 2], d[..., 2], h)
    t0, t1 = np.maximum(s0, z0), np.minimum(s1, z1)
    hit = t0 <= t1
    tt = np.where(hit & np.isfinite(t0), t0, 0.0)
    pt = o + tt[..., None] * d
    side = s0 >= z0
    n = np.where(side[..., None], np.stack((pt[..., 0] / r, pt[..., 1] / r, 0.0 * tt), -1), np.stack((0.0 * tt, 0.0 * tt, np.sign(pt[..., 2])), -1))
    return np.where(hit, t0, np.inf), n


def entry(kind, o, d, size):
    """(t_in [..], outward unit normal at the entry point [.., 3]) of one primitive in its own frame; t_in = inf: the line misses it"""
    if kind == SPHERE:
        return _sphere(o, d, size[0])
    if kind == BOX:
        lo, hi = zip(*(_slab(o[..., k], d[..., k], size[k]) for k in range(3)))
        lo, hi = np.stack(lo, -1), np.stack(hi, -1)
        t0, t1 = lo.max(-1), hi.min(-1)
        k = lo.argmax(-1)
        n = -np.sign(np.take_along_axis(d, k[..., None], -1)) * np.eye(3)[k]
        return np.where(t0 <= t1, t0, np.inf), n
    if kind == CYLINDER:
        return _cylinder(o, d, size[0], size[1])
    t, n = _cylinder(o, d, size[0], size[1])
    for s in (1.0, -1.0):
        ts, ns = _sphere(o - np.array([0.0, 0.0, s * size[1]]), d, size[0])
        better = ts < t
        t, n = np.where(better, ts, t), np.where(better[..., None], ns, n)
    return t, n


def sensor_quat(q, flags):
    if flags & FRAME_YAW:
        qy = np.array([0.0, 0.0, q[2], q[3]])
        return qy / np.sqrt(q[2] ** 2 + q[3] ** 2)
    return q


def rays(root_states, mount, dirs, flags=0):
    """(o world, o' base-relative, d) [N, R, 3] float64 from the float32 inputs"""
    rs, mt, dr = (np.asarray(x, np.float32).astype(np.float64) for x in (root_states, mount, dirs))
    N, R = rs.shape[0], dr.shape[0]
    o, orel, d = np.zeros((N, R, 3)), np.zeros((N, R, 3)), np.zeros((N, R, 3))
    for e in range(N):
        q = sensor_quat(rs[e, 3:7], flags)
        orel[e] = REF.quat_rotate(q, mt[e, 0:3])
        o[e] = rs[e, 0:3] + orel[e]
        d[e] = REF.quat_rotate(q, REF.quat_rotate(mt[e, 3:7], dr))
    return o, orel, d


def posed_prims(robot, quat, theta, body_mask):
    """[(kind, body, centre [3] base-relative, axes [3, 3] rows = local axes in world orientation, size)] of the seen primitives, table order"""
    P, Q = fk(robot, quat, theta)
    out = []
    for p in robot["prims"]:
        b = p["body"]
        if not (body_mask >> b) & 1:
            continue
        c = P[b] + REF.quat_rotate(Q[b], p["pos"])
        qq = qmul(Q[b], p["quat"])
        axes = np.stack([REF.quat_rotate(qq, e) for e in np.eye(3)])
        out.append((p["kind"], b, c, axes, p["size"]))
    return out


def cast_bodies(prims, orel, d, near, far):
    """one env: (t [R] (far: none), |n . d| [R] (nan: none), label [R] (0: none), coordinate magnitude [R]) over posed_prims"""
    R = d.shape[0]
    t, nd, label = np.full(R, far), np.full(R, np.nan), np.zeros(R, np.int64)
    for kind, body, c, axes, size in prims:
        ol, dl = (orel - c) @ axes.T, d @ axes.T
        ti, n = entry(kind, ol, dl, size)
        ok = (ti >= near) & (ti <= far) & ((ti < t) | (label == 0))
        t, label = np.where(ok, ti, t), np.where(ok, 2 + body, label)
        nd = np.where(ok, np.abs((n * dl).sum(-1)), nd)
    coord = np.maximum(np.abs(orel).max(-1), np.abs(orel + t[:, None] * d).max(-1))
    return t, nd, label, coord


def evaluate(scene, robots, env_robot, root_states, dof_pos, o, orel, d, near, far, body_mask):
    """(t, tol, tol of a one-plane move, label) [N, R] for given rays (the nine samples differ in o, orel, d only)"""
    near, far = float(np.float32(near)), float(np.float32(far))
    N, R = d.shape[:2]
    rs = np.asarray(root_states, np.float32).astype(np.float64)
    th = np.asarray(dof_pos, np.float32).astype(np.float64)
    tt, ndt = REF.cast(scene, o.reshape(-1, 3), d.reshape(-1, 3), near, far)
    tt, ndt = tt.reshape(N, R), ndt.reshape(N, R)
    coord_t = np.maximum(np.abs(o).max(-1), np.abs(o + tt[..., None] * d).max(-1))
    t, nd, coord, label = tt.copy(), ndt.copy(), coord_t, np.where(np.isnan(ndt), 0, 1)
    for e in range(N):
        prims = posed_prims(robots[int(env_robot[e])], rs[e, 3:7], th[e], body_mask)
        tb, ndb, lb, cb = cast_bodies(prims, orel[e], d[e], near, far)
        win = (lb > 0) & (tb <= tt[e])
        t[e], nd[e], coord[e], label[e] = np.where(win, tb, t[e]), np.where(win, ndb, nd[e]), np.where(win, cb, coord[e]), np.where(win, lb, label[e])
    miss = np.isnan(nd)
    snd = np.where(miss, 1.0, np.maximum(nd, 1e-300))
    tol = np.where(miss, REF.ATOL, REF.ATOL + REF.C_TOL * 2.0 ** -23 * (coord + t) / snd)
    move = np.where(miss, 0.0, 2.0 * (REF.EPS_POS + REF.EPS_ANG * t) / snd)
    return t, tol, move, label


def envelope(scene, robots, env_robot, root_states, dof_pos, mount, dirs, near, far, body_mask=0x1FFFF, flags=0):
    """lo, hi [N, R] (in t, before scaling), stable [N, R], label of the centre sample [N, R], labels agree [N, R]"""
    o, orel, d = rays(root_states, mount, dirs, flags)
    N, R = d.shape[:2]
    b1, b2 = (b.reshape(N, R, 3) for b in REF._transverse(d.reshape(-1, 3)))
    samples = [(0.0, d)]
    for b in (b1, b2):
        for sgn in (1.0, -1.0):
            samples.append((sgn * REF.EPS_POS * b, d))
            dd = d + sgn * REF.EPS_ANG * b
            samples.append((0.0, dd / np.linalg.norm(dd, axis=-1, keepdims=True)))
    lo, hi = np.full((N, R), np.inf), np.full((N, R), -np.inf)
    tmin, tmax = lo.copy(), hi.copy()
    tol0 = label0 = agree = None
    for shift, dd in samples:
        t, tol, move, label = evaluate(scene, robots, env_robot, root_states, dof_pos, o + shift, orel + shift, dd, near, far, body_mask)
        if tol0 is None:
            tol0, label0, agree = tol + move, label, np.ones((N, R), bool)
        agree &= label == label0
        lo, hi = np.minimum(lo, t - tol), np.maximum(hi, t + tol)
        tmin, tmax = np.minimum(tmin, t), np.maximum(tmax, t)
    return lo, hi, ((tmax - tmin) <= tol0) & agree, label0, agree


def check(scene, robots, env_robot, root_states, dof_pos, mount, dirs, near, far, got, got_labels=None, scale=None, body_mask=0x1FFFF, flags=0, label=""):
    """assert the cap on unstable rays on the reference alone, then every value of `got` [N, R] against its interval and every label of
    `got_labels` where the nine evaluations agree; returns (unstable share, share of rays that end on a body)"""
    lo, hi, stable, lab, agree = envelope(scene, robots, env_robot, root_states, dof_pos, mount, dirs, near, far, body_mask, flags)
    N, R = lo.shape
    share = 1.0 - stable.mean()
    print(f"raycast bodies {label}: {N * R} rays, unstable share {share:.4%}, on a body {np.mean(lab >= 2):.2%}, terrain {np.mean(lab == 1):.2%}")
    assert share <= REF.MAX_UNSTABLE, (label, share)
    sc = np.ones(R) if scale is None else np.asarray(scale, np.float32).astype(np.float64)
    g = np.asarray(got, np.float64)
    assert np.isfinite(g).all(), label
    lo_s, hi_s = lo * sc[None, :] - REF.ATOL, hi * sc[None, :] + REF.ATOL
    bad = ~((g >= lo_s) & (g <= hi_s))
    if bad.any():
        k = np.argwhere(bad)[:5]
        raise AssertionError(f"{label}: {bad.sum()} of {g.size} rays outside the envelope; first: " +
                             "; ".join(f"env {e} ray {r}: got {g[e, r]:.7f}, interval [{lo_s[e, r]:.7f}, {hi_s[e, r]:.7f}], label {lab[e, r]}" for e, r in k))
    if got_labels is not None:
        gl = np.asarray(got_labels).astype(np.int64)
        wrong = agree & (gl != lab)
        assert not wrong.any(), (label, int(wrong.sum()), [(int(e), int(r), int(gl[e, r]), int(lab[e, r])) for e, r in np.argwhere(wrong)[:5]])
    return share, float(np.mean(lab >= 2))
