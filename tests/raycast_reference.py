"""TEST INFRASTRUCTURE -- float64 brute-force reference of the range sensor (include/lsim.h, lsim_raycast), written from the header alone.

It unpacks the mesh words into EVERY triangle and intersects every ray with every triangle (ray-plane intersection and barycentric
coordinates in float64, inclusive edges, both faces, the header's near / far / scale rules).  It shares no code with the kernel and does no
grid walk, never looks at bit 20 or the dz byte: a traversal bug (a skipped cell, a wrong 3 x 3 neighbourhood, a bad dz skip) shows as a wrong depth.

Acceptance (`check`), per ray and for EVERY ray:
  the reference evaluates the ray and eight neighbours -- origin moved by +-EPS_POS and direction tilted by +-EPS_ANG along the two axes
  transverse to the ray.  The value under test must lie in [min_k (t_k - tol_k), max_k (t_k + tol_k)] over the nine, where
      tol_k = ATOL + C * 2^-23 * (max|coordinate| + t_k) / |n_k . d_k|        (n_k: unit normal of the face sample k hits; a miss: ATOL)
  is the conditioning of a ray-plane intersection.  A ray is "stable" when its nine values agree to the centre's tol plus what moving the ray
  over ONE plane explains, 2 * (EPS_POS + EPS_ANG * t) / |n . d| (a sideways step s moves the hit by s * tan(incidence) <= s / |n . d|): near the
  world origin tol is a few micrometres, less than the step EPS_POS itself, so without that term every oblique ray on flat ground would count
  as unstable.  For a stable ray the check is a plain closeness test; an unstable one sees a depth discontinuity or a sharp crease within the steps.
  At most MAX_UNSTABLE of a scene's rays may be unstable, asserted on the reference alone before the value under test is looked at.

The constants, fixed before anything was run:
  EPS_POS = 4 * 1.5e-5 m: the fp32 spacing of a world coordinate at the far corner of the default 1100 x 1900 grid (190 m: 2^-16 = 1.5e-5 m),
            times 4: the origin is a sum of three such coordinates' worth of roundings (base position, rotated mount, their sum) and a vertex of
            two ((a + dx) * hs, - border), and the inclusive-edge slack of the header admits rays up to 3.3e-5 m outside an edge.
  EPS_ANG = 4 * 2^-23 rad: the fp32 spacing of a unit-vector component (2^-24 .. 2^-23), times 4: d is the product of two rotations of dirs[r],
            about ten roundings of that size per component.
  C = 16:   the intersection is t = -(n . s) / (n . d), n = e1 x e2, s = o - a, e = vertex differences, in fp32 with unit roundoff u = 2^-24.
            Relative to the plane's offset the roundings are: vertex coordinates (a + dx) * hs - border, 2 u each at magnitude max|coordinate|;
            the origin p + R(q) m, 1.5 u at that magnitude; s, 1 u; every component of n, 2 products and a difference, about 4 u in direction;
            n . s and n . d, 3 products and 2 sums each, 3 u each; the quotient (not correctly rounded in the simulator's build), 2 u.
            Sum of the counts on the coordinate term 3.5, on the t term 13, in units of u = 2^-23 / 2: 1.75 and 6.5 times 2^-23; the worst case over the
            three components of a vector adds a factor sqrt(3) to the first and the tilt of d (above) adds about 5 to the second: 3 and 11.5,
            rounded up to the next power of two.
  ATOL = 2e-6 m: the rounding of t * scale and of far * scale at 10 m (2^-24 * 10 = 6e-7), with room for the float32 output itself.
"""
import numpy as np

EPS_POS = 4 * 1.5e-5
EPS_ANG = 4 * 2.0 ** -23
C_TOL = 16.0
ATOL = 2e-6
MAX_UNSTABLE = 0.03
DZ_UNIT = 4


# ---- scenes: dict(mesh_type, words [rows, cols] int32 or None, hs, vs, border)
def plane_scene():
    return {"mesh_type": 0, "words": None, "hs": 0.1, "vs": 0.005, "border": 0.0}


def pack_words(hf, hs, vs, mesh_type=2, slope_threshold=0.75):
    """the packed vertex words of include/lsim.h (LSIM_BUF_TERRAIN_MESH) from an int16 height grid: the slope_treshold displacement of the
    reference's trimesh conversion for mesh_type 2, bit 20 and the dz byte.  A numpy restatement, compared with the library's in the tests."""
    hf = np.asarray(hf, np.int16)
    R, Cn = hf.shape
    H = hf.astype(np.float64)
    dx = np.zeros((R, Cn), np.int64)
    dy = np.zeros((R, Cn), np.int64)
    if mesh_type == 2 and slope_threshold > 0:
        thr = np.float32(np.float32(slope_threshold) * np.float32(hs)) / np.float32(vs)
        mx = np.zeros((R, Cn), np.int64); my = np.zeros((R, Cn), np.int64); mc = np.zeros((R, Cn), np.int64)
        mx[:-1, :] += (H[1:, :] - H[:-1, :] > thr)
        mx[1:, :] -= (H[:-1, :] - H[1:, :] > thr)
        my[:, :-1] += (H[:, 1:] - H[:, :-1] > thr)
        my[:, 1:] -= (H[:, :-1] - H[:, 1:] > thr)
        mc[:-1, :-1] += (H[1:, 1:] - H[:-1, :-1] > thr)
        mc[1:, 1:] -= (H[:-1, :-1] - H[1:, 1:] > thr)
        dx = mx + np.where(mx == 0, mc, 0)
        dy = my + np.where(my == 0, mc, 0)
    moved = (dx != 0) | (dy != 0)
    flags = (dx + 1) | ((dy + 1) << 2)
    words = (hf.astype(np.int64) & 0xFFFF) | (flags << 16)
    if mesh_type == 2 and slope_threshold > 0:
        words |= block_any(moved).astype(np.int64) << 20
    top = block_max(hf.astype(np.int64))
    dz = np.minimum((top - hf + DZ_UNIT - 1) // DZ_UNIT, 255)
    words |= dz << 24
    return (words & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def _block(a, fn, fill):
    """fn over the 4 x 4 block rows i-1..i+2, cols j-1..j+2 (clipped to the grid) of every (i, j)"""
    R, Cn = a.shape
    p = np.full((R + 3, Cn + 3), fill, a.dtype)
    p[1:R + 1, 1:Cn + 1] = a
    out = p[0:R, 0:Cn].copy()
    for di in range(4):
        for dj in range(4):
            out = fn(out, p[di:di + R, dj:dj + Cn])
    return out


def block_any(m):
    return _block(m, np.logical_or, False)


def block_max(h):
    return _block(h, np.maximum, np.iinfo(np.int64).min)


def force_slow_paths(words, which):
    """the same geometry with dz = 255 everywhere ("dz") or bit 20 set everywhere ("bit20"): legal words that disable one shortcut"""
    w = words.view(np.uint32).astype(np.int64)
    if which == "dz":
        w = (w & 0x00FFFFFF) | (255 << 24)
    else:
        w = w | (1 << 20)
    return (w & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def grid_scene(hf, hs=0.1, vs=0.005, border=0.0, mesh_type=2, slope_threshold=0.75):
    return {"mesh_type": mesh_type, "words": pack_words(hf, hs, vs, mesh_type, slope_threshold), "hs": hs, "vs": vs, "border": border}


def vertices(scene):
    """[rows, cols, 3] float64 vertex positions of the header's formula, from the float32 constants the launch is given"""
    w = scene["words"].view(np.uint32).astype(np.int64)
    hs, vs, border = (float(np.float32(scene[k])) for k in ("hs", "vs", "border"))
    rows, cols = w.shape
    a, b = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    dx, dy = ((w >> 16) & 3) - 1, ((w >> 18) & 3) - 1
    h = ((w & 0xFFFF) ^ 0x8000) - 0x8000          # int16 sign extension
    return np.stack(((a + dx) * hs - border, (b + dy) * hs - border, h * vs), axis=-1).astype(np.float64)


def triangles(scene):
    """(A, E1, E2) [T, 3]: every existing triangle of the mesh"""
    P = vertices(scene)
    p00, p10, p01, p11 = P[:-1, :-1], P[1:, :-1], P[:-1, 1:], P[1:, 1:]
    A = np.concatenate((p00.reshape(-1, 3), p00.reshape(-1, 3)))
    B = np.concatenate((p11.reshape(-1, 3), p10.reshape(-1, 3)))
    Cc = np.concatenate((p01.reshape(-1, 3), p11.reshape(-1, 3)))
    E1, E2 = B - A, Cc - A
    n = np.cross(E1, E2)
    keep = (n * n).sum(1) >= 1e-16
    return A[keep], E1[keep], E2[keep]


# ---- rays
def quat_rotate(q, v):
    """R(q) v of the header, q xyzw [..., 4], v [..., 3]"""
    u, w = q[..., :3], q[..., 3:4]
    t = 2.0 * np.cross(u, v)
    return v + w * t + np.cross(u, t)


def rays(root_states, mount, dirs):
    """(o, d) [N, R, 3] float64 from the float32 inputs: the header's sensor pose"""
    rs, mt, dr = (np.asarray(x, np.float32).astype(np.float64) for x in (root_states, mount, dirs))
    p, q = rs[:, None, 0:3], rs[:, None, 3:7]
    o = p + quat_rotate(q, mt[:, None, 0:3])
    d = quat_rotate(q, quat_rotate(mt[:, None, 3:7], dr[None, :, :]))
    return np.broadcast_to(o, d.shape).copy(), d


def cast(scene, o, d, near, far, chunk=1024):
    """brute force: (t [M], |n . d| of the hit face [M] (nan: miss)) for rays o, d [M, 3]"""
    o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    M = o.shape[0]
    near, far = float(np.float32(near)), float(np.float32(far))
    t_out, nd_out = np.full(M, far), np.full(M, np.nan)
    if scene["mesh_type"] == 0 or scene["words"] is None:
        with np.errstate(divide="ignore", invalid="ignore"):
            t = -o[:, 2] / d[:, 2]
        ok = (np.abs(d[:, 2]) >= 1e-30) & (t >= near) & (t <= far)
        t_out[ok] = t[ok]
        nd_out[ok] = np.abs(d[ok, 2])
        return t_out, nd_out
    A, E1, E2 = triangles(scene)
    Nn = np.cross(E1, E2)
    nn = (Nn * Nn).sum(1)
    G1, G2 = np.cross(E2, Nn) / nn[:, None], np.cross(Nn, E1) / nn[:, None]      # dual basis: u = (P - a) . g1, v = (P - a) . g2
    Nu = Nn / np.sqrt(nn)[:, None]
    na, ag1, ag2 = (Nu * A).sum(1), (A * G1).sum(1), (A * G2).sum(1)
    SLACK = 1e-9        # inclusive edges in float64
    for c0 in range(0, M, chunk):
        oc, dc = o[c0:c0 + chunk], d[c0:c0 + chunk]
        nd = dc @ Nu.T
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (na[None, :] - oc @ Nu.T) / nd
            u = oc @ G1.T + t * (dc @ G1.T) - ag1[None, :]
            v = oc @ G2.T + t * (dc @ G2.T) - ag2[None, :]
            ok = (np.abs(nd) > 1e-14) & (u >= -SLACK) & (v >= -SLACK) & (u + v <= 1 + SLACK) & (t >= near) & (t <= far)
        t = np.where(ok, t, np.inf)
        k = t.argmin(1)
        rows = np.arange(t.shape[0])
        hit = np.isfinite(t[rows, k])
        t_out[c0:c0 + chunk][hit] = t[rows, k][hit]
        nd_out[c0:c0 + chunk][hit] = np.abs(nd[rows, k][hit])
    return t_out, nd_out


def _transverse(d):
    """two unit vectors orthogonal to d [M, 3] and to each other"""
    ref = np.where((np.abs(d[:, 0:1]) > 0.9), np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]))
    b1 = np.cross(d, ref)
    b1 /= np.linalg.norm(b1, axis=1, keepdims=True)
    b2 = np.cross(d, b1)
    b2 /= np.linalg.norm(b2, axis=1, keepdims=True)
    return b1, b2


def envelope(scene, o, d, near, far):
    """lo, hi, stable [M]: the acceptance interval of every ray (in t, before scaling) and which rays are stable"""
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    b1, b2 = _transverse(d)
    samples = [(o, d)]
    for b in (b1, b2):
        for sgn in (1.0, -1.0):
            samples.append((o + sgn * EPS_POS * b, d))
            dd = d + sgn * EPS_ANG * b
            samples.append((o, dd / np.linalg.norm(dd, axis=1, keepdims=True)))
    lo, hi = np.full(o.shape[0], np.inf), np.full(o.shape[0], -np.inf)
    tmin, tmax, tol0 = lo.copy(), hi.copy(), None
    for oo, dd in samples:
        t, nd = cast(scene, oo, dd, near, far)
        coord = np.maximum(np.abs(oo).max(1), np.abs(oo + t[:, None] * dd).max(1))
        tol = np.where(np.isnan(nd), ATOL, ATOL + C_TOL * 2.0 ** -23 * (coord + t) / np.where(np.isnan(nd), 1.0, nd))
        if tol0 is None:
            tol0 = tol + np.where(np.isnan(nd), 0.0, 2.0 * (EPS_POS + EPS_ANG * t) / np.where(np.isnan(nd), 1.0, nd))
        lo, hi = np.minimum(lo, t - tol), np.maximum(hi, t + tol)
        tmin, tmax = np.minimum(tmin, t), np.maximum(tmax, t)
    return lo, hi, (tmax - tmin) <= tol0


def check(scene, root_states, mount, dirs, near, far, got, scale=None, label=""):
    """assert the cap on unstable rays on the reference alone, then that every value of `got` [N, R] lies in its interval; returns the share"""
    o, d = rays(root_states, mount, dirs)
    N, R = d.shape[:2]
    lo, hi, stable = envelope(scene, o, d, near, far)
    share = 1.0 - stable.mean()
    print(f"raycast {label}: {N * R} rays, unstable share {share:.4%}")
    assert share <= MAX_UNSTABLE, (label, share)
    sc = np.ones(R) if scale is None else np.asarray(scale, np.float32).astype(np.float64)
    sc = np.broadcast_to(sc[None, :], (N, R)).reshape(-1)
    g = np.asarray(got, np.float64).reshape(-1)
    assert np.isfinite(g).all(), label
    lo_s, hi_s = lo * sc - ATOL, hi * sc + ATOL            # scale > 0; the product's own rounding
    bad = ~((g >= lo_s) & (g <= hi_s))
    if bad.any():
        k = np.flatnonzero(bad)[:5]
        raise AssertionError(f"{label}: {bad.sum()} of {g.size} rays outside the envelope; first: " +
                             "; ".join(f"ray {i}: got {g[i]:.7f}, interval [{lo_s[i]:.7f}, {hi_s[i]:.7f}], o {o.reshape(-1, 3)[i]}, d {d.reshape(-1, 3)[i]}" for i in k))
    return share
