"""TEST INFRASTRUCTURE -- numpy reference of the elevation-map launch, written from the comment of lsim_elevation_map in include/lsim.h (not
from the kernel source), in float64 from the fp32 inputs: which envs are visited, cleared and due, the points of the rays, the window, the
maximum per cell, the toroidal slots, and the scan.

Exact scenes.  With res = 2^-4, poses, mount, depths and directions multiples of 2^-6 and the quaternions the identity or (0, 0, 1, 0), every
product and sum of the header is exact in fp32, so float64 computes the same numbers and the comparison is bit for bit (`RefMap.step`).

General poses (`bracket`).  A point is AMBIGUOUS when its float64 position lies within EPS of a cell boundary in x or y.  EPS, per component,
from the operation count, u = 2^-24 (one rounding per operation; a fused product-sum has fewer, never more), L = |mpos| + t_hi:
  R(q) v = v + 2 w (u x v) + 2 u x (u x v) for |q| = 1:  the first cross product 4 u |v| per component (two products, a difference, on
      |u_i v_j| + |u_j v_i| <= |v|), the second 4 u |v| of its own and 7 u |v| carried in, the product with w 6 u |v|, the two sums 10 u |v|
      -> 27 u |v|, taken as 30;
  t = (a * depth + b) * inv_scale: 3 u, v = dirs * t: 1 more -> 4 u |v| carried through both rotations (each of norm 1: sqrt(3) per component);
  m = mpos + R(mq) v: 30 u |v| + u L;   R(q) m: 30 u L + sqrt(3) of what m carries;   P = p + that: u (|p| + L);   x * rinv: u |P| more
  -> EPS = u (2 |p|_inf + 120 L), which is 3.75e-5 m for a 5 m camera near the origin and 6.0e-5 m 190 m from it.  With 1/16 m cells a point is
     within EPS of one of its cell's four edges with probability 4 EPS / res = 0.25 % .. 0.4 %: below the 1 % the tests insist on.
The robot's own cell (the window's centre) is kept unambiguous by the scenes (they place p.xy at cell centres).  Neither EPS nor the
brackets have seen the kernel's output."""
import numpy as np

from helpers import abi

FILL_ALL, RESETS_ONLY = abi.DEFINES["LSIM_SENSOR_FILL_ALL"], abi.DEFINES["LSIM_SENSOR_RESETS_ONLY"]
F = np.float32
U = 2.0 ** -24
MUTANTS = ("last_ray_wins", "truncate", "upper_edge_inclusive", "clear_when_due", "scan_full_quat")


def rot(q, v):
    """R(q) v of the header for xyzw rows, float64"""
    u, w = q[..., :3], q[..., 3:4]
    t = 2.0 * np.cross(u, v)
    return v + w * t + np.cross(u, t)


def due_set(N, env_stride, flags, episode_length, tick, period, stagger):
    """(visited, fill, due) [N] bool: lsim_sensor_capture's rule"""
    e = np.arange(N, dtype=np.int64)
    visited = e % env_stride == 0
    fill = visited & (bool(flags & FILL_ALL) | (np.asarray(episode_length) == 0))
    on_tick = (tick + (e if stagger else 0)) % period == 0
    due = visited & (fill | (on_tick & (not flags & RESETS_ONLY)))
    return visited, fill, due


def pack(ix, iy):
    return ((np.asarray(ix, np.int64) + 32768) << 16 | (np.asarray(iy, np.int64) + 32768)).astype(np.uint32)


def eps(p, mount_pos, t_hi):
    """the module docstring's EPS for a robot at `p`"""
    return U * (2.0 * np.abs(p).max() + 120.0 * (np.linalg.norm(mount_pos) + t_hi))


class Params:
    def __init__(self, G, res, dirs, pts, inv_scale=None, env_stride=1, period=1, stagger=0, a=1.0, b=0.0, t_lo=0.0, t_hi=100.0, unknown_drop=0.5):
        self.G, self.res, self.rinv = int(G), float(F(res)), float(F(1.0 / float(F(res))))
        self.dirs, self.pts = np.asarray(dirs, F).astype(np.float64).reshape(-1, 3), np.asarray(pts, F).astype(np.float64).reshape(-1, 2)
        self.inv_scale = None if inv_scale is None else np.asarray(inv_scale, F).astype(np.float64)
        self.env_stride, self.period, self.stagger = env_stride, period, stagger
        self.a, self.b, self.t_lo, self.t_hi, self.unknown_drop = (float(F(v)) for v in (a, b, t_lo, t_hi, unknown_drop))

    @classmethod
    def of(cls, rig):
        em = rig.em
        inv = rig.get("inv_scale") if "inv_scale" in rig.a else None
        return cls(rig.G, em.res, rig.get("dirs"), rig.get("pts"), inv, em.env_stride, em.period, em.stagger, em.a, em.b, em.t_lo, em.t_hi, em.unknown_drop)


def points(par, inp, e):
    """(P [R, 3] float64, valid [R] bool) of env e"""
    rs, mt = inp["root_states"][e].astype(np.float64), inp["mount"][e].astype(np.float64)
    with np.errstate(all="ignore"):
        d = par.a * inp["depth"][e].astype(np.float64) + par.b
        t = d if par.inv_scale is None else d * par.inv_scale
        valid = np.isfinite(d) & (np.abs(d) <= np.finfo(F).max) & (par.t_lo < t) & (t < par.t_hi)
        if inp.get("labels") is not None:
            valid &= inp["labels"][e] == 1
        tt = np.where(valid, t, 0.0)
        P = rs[:3] + rot(rs[3:7], mt[:3] + rot(mt[3:7], par.dirs * tt[:, None]))
    return P, valid


class RefMap:
    """the state of N envs and `step`, one launch; everything a launch writes is kept as the header's types"""

    def __init__(self, N, par, like):
        self.N, self.par = N, par
        self.height, self.stamp, self.cell = like["height"].copy(), like["stamp"].copy(), like["cell"].copy()
        self.scan, self.known, self.state = like["scan"].copy(), like["known"].copy(), int(like["state"])

    def cellof(self, x, mutant=None):
        v = np.asarray(x, np.float64) * self.par.rinv
        return (np.trunc(v) if mutant == "truncate" else np.floor(v)).astype(np.int64)

    def step(self, inp, tick, flags=0, mutant=None):
        par, G = self.par, self.par.G
        visited, fill, due = due_set(self.N, par.env_stride, flags, inp["episode_length"], tick, par.period, par.stagger)
        for e in np.nonzero(visited)[0]:
            rs, mt = inp["root_states"][e].astype(np.float64), inp["mount"][e].astype(np.float64)
            ok = bool(np.isfinite(rs[:7]).all() and np.isfinite(mt).all())
            if fill[e] or (mutant == "clear_when_due" and due[e]):
                self.stamp[e] = -1
            if not ok:
                self.state += 1
                self.scan[e], self.known[e] = 0.0, 0
                continue
            if due[e]:
                P, valid = points(par, inp, e)
                valid &= np.isfinite(P).all(axis=1)
                cx, cy = (int(np.clip(self.cellof(rs[k], mutant), -40000, 40000)) for k in (0, 1))
                best = {}
                for r in np.nonzero(valid)[0]:
                    fx, fy = (np.trunc if mutant == "truncate" else np.floor)(P[r, :2] * par.rinv)
                    if not (-32768 < fx < 32768 and -32768 < fy < 32768):
                        continue
                    ix, iy = int(fx), int(fy)
                    hi = G // 2 + (1 if mutant == "upper_edge_inclusive" else 0)
                    if not (-G // 2 <= ix - cx < hi and -G // 2 <= iy - cy < hi):
                        continue
                    z = P[r, 2]
                    if mutant == "last_ray_wins" or (ix, iy) not in best or z > best[ix, iy]:
                        best[ix, iy] = z
                for (ix, iy), z in best.items():
                    s = (ix & (G - 1), iy & (G - 1))
                    self.height[e][s], self.stamp[e][s], self.cell[e][s] = F(z), np.int32(int(tick) & 0x7FFFFFFF), pack(ix, iy)
            q = rs[3:7]
            with np.errstate(all="ignore"):
                qy = q if mutant == "scan_full_quat" else np.array([0.0, 0.0, q[2], q[3]]) / np.sqrt(q[2] ** 2 + q[3] ** 2)
                w = rs[:2] + rot(qy, np.concatenate((par.pts, np.zeros((len(par.pts), 1))), axis=1))[:, :2]
                f = np.floor(w * par.rinv)
            for j in range(len(par.pts)):
                self.scan[e, j], self.known[e, j] = F(F(rs[2]) - F(par.unknown_drop)), 0
                if np.isfinite(f[j]).all() and (np.abs(f[j]) < 32768).all():
                    ix, iy = int(f[j, 0]), int(f[j, 1])
                    s = (ix & (G - 1), iy & (G - 1))
                    if self.stamp[e][s] >= 0 and self.cell[e][s] == pack(ix, iy):
                        self.scan[e, j], self.known[e, j] = self.height[e][s], 1
        return visited, fill, due


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 1: np.uint8, 8: np.uint64}[a.dtype.itemsize])


def assert_same(got, ref, what=""):
    """every array a launch writes, bit for bit"""
    for k in ("stamp", "cell", "height", "known", "scan"):
        np.testing.assert_array_equal(bits(got[k]), bits(getattr(ref, k)), err_msg=f"{what}: {k}")
    assert got["state"] == ref.state, what


def bracket(par, inp, e):
    """for ONE launch of env e (finite pose, due) into an empty map: {(ix, iy): [sure_max, possible_max, possible_min]} (sure_max -inf
    when only ambiguous points may lie in the cell), EPS, and how many of the valid points are ambiguous, and how many there are"""
    G = par.G
    rs = inp["root_states"][e].astype(np.float64)
    E = eps(rs[:3], inp["mount"][e][:3], par.t_hi)
    P, valid = points(par, inp, e)
    c = np.floor(rs[:2] * par.rinv).astype(np.int64)
    assert (np.abs(rs[:2] * par.rinv - np.round(rs[:2] * par.rinv)) > 0.25).all(), "the scene keeps the robot's own cell unambiguous"
    cells, amb, n = {}, 0, 0
    for r in np.nonzero(valid)[0]:
        lo, hi = np.floor((P[r, :2] - E) * par.rinv).astype(np.int64), np.floor((P[r, :2] + E) * par.rinv).astype(np.int64)
        sure = bool((lo == hi).all())
        cand = [(ix, iy) for ix in {lo[0], hi[0]} for iy in {lo[1], hi[1]}
                if -G // 2 <= ix - c[0] < G // 2 and -G // 2 <= iy - c[1] < G // 2 and abs(ix) < 32768 and abs(iy) < 32768]
        n += 1
        amb += (not sure)
        for key in cand:
            rec = cells.setdefault(key, [-np.inf, -np.inf, np.inf])
            if sure:
                rec[0] = max(rec[0], P[r, 2])
            rec[1], rec[2] = max(rec[1], P[r, 2]), min(rec[2], P[r, 2])
    return cells, E, amb, n


def check_bracket(par, inp, e, got, tick):
    """the comparison rule for general poses, on env e of a launch into an empty map; returns (ambiguous points, valid points)"""
    G = par.G
    cells, E, amb, n = bracket(par, inp, e)
    seen = np.zeros((G, G), bool)
    for (ix, iy), (sure_max, poss_max, poss_min) in cells.items():
        s = (ix & (G - 1), iy & (G - 1))
        seen[s] = True
        knows = got["stamp"][e][s] >= 0
        if sure_max > -np.inf:
            assert knows, (e, ix, iy, "a cell with a sure point is unknown")
        if knows:
            assert got["stamp"][e][s] == tick and got["cell"][e][s] == pack(ix, iy), (e, ix, iy)
            h = float(got["height"][e][s])
            lower = sure_max if sure_max > -np.inf else poss_min
            assert lower - E <= h <= poss_max + E, (e, ix, iy, h, lower, poss_max)
    assert (got["stamp"][e][~seen] == -1).all(), "a slot no point can reach was written"
    return amb, n
