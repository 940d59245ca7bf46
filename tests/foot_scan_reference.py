"""TEST INFRASTRUCTURE -- float64 reference of the foot-scan launch (include/lsim.h, lsim_foot_scan), written from the header's comment alone.
It shares no code with the kernel: its own forward kinematics, its own rotation, its own cell arithmetic, no LDS, no lanes.

A scene is a dict of the launch's inputs as numpy arrays and numbers (tests/foot_scan_scenes.py builds them; tests/foot_scan_emu_binding.py
turns one into a struct).  `reference(scene)` evaluates every point in float64 from the same fp32 inputs and returns what the launch must
write, plus for every point whether it is AMBIGUOUS: its float64 position w lies within
    delta = 64 * 2^-24 * max(1, |p.x|, |p.y|)   metres
of a cell boundary of the source's grid, on either axis.  That is the rounding of the kernel's fp32 chain at that magnitude: w is a sum of
four rotated link offsets, the pattern offset and p -- about a dozen roundings of a coordinate no larger than max(1, |p|) + 1, each at most
2^-24 relative, plus sinf / cosf of half a joint angle (1-2 ulp each, four links deep) -- rounded up to 64 ulp.  On an ambiguous point the
kernel may pick the neighbouring cell, so its height and known are not compared; everywhere else they are exact, and a row value may differ
by scale * delta (the same chain's error in p.z + F.z; h is a stored value and has none).  `check` applies that rule and the cap on the
ambiguous share, MAX_AMBIGUOUS = 1 % of a scene's points."""
import numpy as np

F = np.float32
TERRAIN, MAP = 0, 1
MAX_AMBIGUOUS = 0.01


def rotate(q, v):
    """R(q) v for q xyzw, by the rotation matrix"""
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return R @ np.asarray(v, np.float64)


def qmul(a, b):
    """a * b with R(a * b) = R(a) R(b), xyzw"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def bodies_of(table):
    """[(joint_pos, joint_axis, parent, dof)] of an lsim_raycast_robot (ctypes), in float64"""
    return [(np.array(list(b.joint_pos), np.float64), np.array(list(b.joint_axis), np.float64), int(b.parent), int(b.dof)) for b in table.bodies]


def feet(bodies, q, th):
    """F [4, 3]: P of bodies 4, 8, 12, 16 by the header's recursion, relative to the base position"""
    P, Q = {0: np.zeros(3)}, {0: np.asarray(q, np.float64)}
    for b in range(1, 17):
        jp, ax, parent, dof = bodies[b]
        P[b] = P[parent] + rotate(Q[parent], jp)
        a = float(th[dof]) if dof >= 0 else 0.0
        Q[b] = qmul(Q[parent], np.concatenate((ax * np.sin(0.5 * a), [np.cos(0.5 * a)])))
    return np.stack([P[4 + 4 * l] for l in range(4)])


def reference(sc):
    """dict: heights [N, 4K] f32, known [N, 4K] u8, rows [N, channels * 4K] f32, visited [N], bad [N], ambiguous [N, 4K], delta [N],
    centres [N, 4, 3] f64, w [N, 4K, 2] f64, category [N, 4K] (map source: 0 known, 1 never written, 2 a slot left over, 3 outside / not finite;
    terrain source: 0 inside the grid, 3 clipped)"""
    pose, th_all, pat = np.asarray(sc["pose"], F), np.asarray(sc["dof_pos"], F), np.asarray(sc["pattern"], F).astype(np.float64)
    N, K = pose.shape[0], pat.shape[0]
    K4 = 4 * K
    out = dict(heights=np.zeros((N, K4), F), known=np.zeros((N, K4), np.uint8), rows=np.zeros((N, sc["channels"] * K4), F),
               visited=np.arange(N) % sc["env_stride"] == 0, bad=np.zeros(N, bool), ambiguous=np.zeros((N, K4), bool), delta=np.zeros(N),
               centres=np.full((N, 4, 3), np.nan), w=np.full((N, K4, 2), np.nan), category=np.full((N, K4), -1))
    tabs = [bodies_of(t) for t in sc["tables"]]
    for e in range(N):
        if not out["visited"][e]:
            continue
        p, q, th = pose[e, 0:3].astype(np.float64), pose[e, 3:7].astype(np.float64), th_all[e]
        if not (np.isfinite(pose[e, :7]).all() and np.isfinite(th).all()) or (q[2] == 0.0 and q[3] == 0.0):
            out["bad"][e] = True
            continue
        k = 0 if sc.get("env_robot") is None else min(max(int(sc["env_robot"][e]), 0), len(tabs) - 1)
        Fl = feet(tabs[k], q, th)
        out["centres"][e] = p + Fl
        n = 1.0 / np.sqrt(q[2] * q[2] + q[3] * q[3])
        c, s = (q[3] * n) ** 2 - (q[2] * n) ** 2, 2.0 * (q[2] * n) * (q[3] * n)          # R(qy) is the plane rotation (c, -s; s, c)
        o = np.stack((c * pat[:, 0] - s * pat[:, 1], s * pat[:, 0] + c * pat[:, 1]), -1)  # [K, 2]
        w = (p[None, None, :2] + Fl[:, None, :2] + o[None, :, :]).reshape(K4, 2)
        out["w"][e] = w
        fz = np.repeat(p[2] + Fl[:, 2], K)
        delta = 64.0 * 2.0 ** -24 * max(1.0, abs(p[0]), abs(p[1]))
        out["delta"][e] = delta
        if sc["source"] == TERRAIN:
            known = np.ones(K4, np.uint8)
            if sc["mesh_type"] == 0:
                h, cat = np.zeros(K4, F), np.zeros(K4, int)
            else:
                g, hs = np.asarray(sc["height_grid"]), float(F(sc["hs"]))
                fx = (w + float(F(sc["border"]))) / hs
                out["ambiguous"][e] = (np.abs(fx - np.round(fx)) * hs < delta).any(-1)
                t = np.trunc(fx).astype(np.int64)
                px, py = np.clip(t[:, 0], 0, g.shape[0] - 2), np.clip(t[:, 1], 0, g.shape[1] - 2)
                cat = np.where((fx[:, 0] < 0) | (fx[:, 0] >= g.shape[0] - 1) | (fx[:, 1] < 0) | (fx[:, 1] >= g.shape[1] - 1), 3, 0)
                m = np.minimum(np.minimum(g[px, py], g[px + 1, py]), g[px, py + 1])
                h = m.astype(F) * F(sc["vs"])
        else:
            G, res = int(sc["G"]), float(F(sc["res"]))
            rinv = float(F(1.0 / res))
            fx = w * rinv
            out["ambiguous"][e] = (np.abs(fx - np.round(fx)) / rinv < delta).any(-1)
            cellf = np.floor(fx)
            inside = np.isfinite(w).all(-1) & (cellf > -32768).all(-1) & (cellf < 32768).all(-1)
            ci = np.where(inside[:, None], cellf, 0).astype(np.int64)
            slot = (ci[:, 0] & (G - 1)) * G + (ci[:, 1] & (G - 1))
            word = ((ci[:, 0] + 32768) << 16) | (ci[:, 1] + 32768)
            st, cw = np.asarray(sc["stamp"])[e].reshape(-1)[slot], np.asarray(sc["cell"])[e].reshape(-1)[slot].astype(np.int64)
            kn = inside & (st >= 0) & (cw == word)
            cat = np.where(~inside, 3, np.where(kn, 0, np.where(st < 0, 1, 2)))
            h = np.where(kn, np.asarray(sc["height"], F)[e].reshape(-1)[slot], F(pose[e, 2] - F(sc["unknown_drop"]))).astype(F)
            known = kn.astype(np.uint8)
        out["category"][e] = cat
        with np.errstate(invalid="ignore", over="ignore"):
            t = (fz.astype(F) - F(sc["z_offset"])) - h              # fz is exact in fp32 on the exact scenes; elsewhere scale * delta covers its rounding
            v = np.minimum(np.maximum(t, F(-1.0)), F(1.0)) * F(sc["scale"])
        out["heights"][e], out["known"][e] = h, known
        out["rows"][e, :K4] = np.where(np.isfinite(t), v, F(0.0))
        if sc["channels"] == 2:
            out["rows"][e, K4:] = known.astype(F)
    return out


def bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def check(sc, ref, got, exact, label="", cap=MAX_AMBIGUOUS):
    """`got`: dict rows [N, ld], heights [N, >= 4K], known [N, >= 4K], state (int), `before`: the same arrays before the launch.  exact: every
    point bit for bit; otherwise the ambiguous points are left out (at most `cap` of them) and rows get scale * delta.  `cap` None: no cap
    -- a live env of a few hundred points, where 1 % is three points and says nothing.  Returns the share"""
    K4, C = ref["heights"].shape[1], sc["channels"]
    vis, before = ref["visited"], got["before"]
    for name, width in (("rows", C * K4), ("heights", K4), ("known", K4)):
        a, b = got[name], before[name]
        assert np.array_equal(a[~vis], b[~vis]), f"{label}: {name} of an env that is not visited was written"
        assert np.array_equal(a[:, width:], b[:, width:]), f"{label}: {name} beyond column {width} was written"
    assert np.isfinite(got["rows"][vis][:, :C * K4]).all(), f"{label}: a non-finite row value"
    assert int(got["state"]) == int(before["state"]) + int((ref["bad"] & vis).sum()), f"{label}: state[0]"
    use = vis[:, None] & (np.ones_like(ref["ambiguous"]) if exact else ~ref["ambiguous"])
    share = float(ref["ambiguous"][vis].mean()) if vis.any() else 0.0
    if exact:
        assert not ref["ambiguous"].any(), f"{label}: an exact scene has a point within delta of a cell boundary"
        np.testing.assert_array_equal(bits(got["rows"][:, :C * K4])[vis], bits(ref["rows"])[vis], err_msg=label)
    else:
        assert cap is None or share <= cap, f"{label}: {share:.3%} of the points are ambiguous"
        tol = (abs(float(sc["scale"])) * ref["delta"])[:, None]
        err = np.abs(got["rows"][:, :K4].astype(np.float64) - ref["rows"][:, :K4].astype(np.float64))
        assert (err <= tol)[use].all(), f"{label}: row values off by up to {err[use].max():.3g}, allowed {tol.max():.3g}"
        if C == 2:
            assert np.array_equal(got["rows"][:, K4:2 * K4][use], ref["rows"][:, K4:][use]), f"{label}: the known block"
    assert np.array_equal(bits(got["heights"][:, :K4])[use], bits(ref["heights"])[use]), f"{label}: heights"
    assert np.array_equal(got["known"][:, :K4][use], ref["known"][use]), f"{label}: known"
    return share
