"""TEST INFRASTRUCTURE -- numpy reference of lsim_elevation_map_fused and lsim_map_rows_fused, written from their comments in include/lsim.h
(not from the kernel source), in float64 from the fp32 inputs, on top of elevation_map_reference (the rules the two launches share), and
FusedRig: elevation_map_emu_binding.Rig with the fused launch's struct and its two arrays, guarded like the others.

What is exact.  stamp, cell, known and -- on the dyadic scenes, where every point, zmax and df * 65536 are exact -- sum and count are
integers and compared exactly.  height, var, scan and scan_var carry a BOUND per element, propagated through the captures from the
operation count, u = 2^-24, one rounding per operation (a fused product-sum has fewer, never more).  For a touched slot, first order:
  mean = sum / count: u mean;  * 2^-16 exact;  zm = zmax - that: u |zm|                          -> e_zm = u (band + |zm|)       (mean 2^-16 <= band)
  X = (ix + 0.5) res: u |X|;  ex = X - p.x: u |ex|;  ex^2, ey^2 and their sum: 3 u rho2      -> e_rho = 2 u (|ex| (|X| + |ex|) + |ey| (|Y| + |ey|)) + 3 u rho2
  sigma = s0 + s2 (rho2 + z2): a sum, a product, a sum                                           -> e_sig = s2 e_rho + 3 u sigma
  vm = sigma^2 / nc + floor: a product, a quotient, a sum                                        -> e_vm = 2 sigma e_sig / nc + 3 u vm
  age: an integer below 2^31, rounded once when above 2^24;  vp = var + g age                    -> e_vp = e_var + 3 u vp
  d = zm - h                                                                                     -> e_d = e_zm + e_h + u |d|
  S = vp + vm                                                                                    -> e_S = e_vp + e_vm + u S
  K = vp / S                                                                                     -> e_K = e_vp / S + vp e_S / S^2 + u K
  h' = h + K d                                                                                   -> e_h' = e_h + |d| e_K + K e_d + u |K d| + u |h'|
  var' = K vm                                                                                    -> e_var' = vm e_K + K e_vm + u var'
  overwrite: e_h' = e_zm, e_var' = e_vm;  the clamp moves nothing apart;  scan_var = min(var + g age, var_max): e_var + 3 u (var + g age).
The bound asserted is TWICE that sum (the second-order terms are below 2^-20 of it).  A gate decision is AMBIGUOUS when
|d^2 - gate2 S| <= 2 |d| e_d + gate2 e_S + 2 u (d^2 + gate2 S), unless both sides are exact and equal: the scenes avoid it and `step`
asserts so.  Nothing here has seen the kernel's or the shim's output.

MUTANTS, each with the scene of tests/test_elevation_fuse.py that misses its bound by more than 10 x:
  no_growth (the growth not applied to the prior)          ageing        K_swapped (K = vm / S)                       ageing
  gate_inclusive (d^2 <= gate2 S)                          gate_edge     no_gate                                      steps
  no_clamp                                                 clamps        no_cap (min(count, cap) dropped)             counts
  no_wrap (the age's 31-bit wrap dropped)                  wrap          band_on_z (z <= band)                        spread
  sum_all (the second pass sums every kept point)          spread"""
import numpy as np

import elevation_map_emu_binding as EB
import elevation_map_reference as ER
import emu_binding
from helpers import abi

F = np.float32
U = 2.0 ** -24
MUTANTS = ("no_growth", "K_swapped", "gate_inclusive", "no_gate", "no_clamp", "no_cap", "no_wrap", "band_on_z", "sum_all")
FIELDS = ("sigma0", "sigma2", "range_z2", "band", "var_floor", "var_growth", "var_max", "gate2")
DEFAULTS = dict(sigma0=0.01, sigma2=0.002, range_z2=0.16, band=0.0625, var_floor=2.5e-5, var_growth=1e-6, var_max=0.25, gate2=9.0, count_cap=4)
GUARD_VALUE = {"var": -77.25, "scan_var": -55.5}
INITIAL = {"var": 333.0, "scan_var": 444.0}


def lib():
    return emu_binding.shim("elevation_fuse")


class FusedRig(EB.Rig):
    """Rig with var [N, G, G] and scan_var [N, P + 3] (guarded) and the fused struct; `fusion`: the by-value fields (DEFAULTS).  `edit` of
    launch() sees the inner lsim_elevation_map_t, as Rig's does, `edit_fused` the whole struct."""

    def __init__(self, N, G, dirs, pts, fusion=None, device=None, entry=None, **kw):
        super().__init__(N, G, dirs, pts, device=device, entry=entry, **kw)
        self.var_stride = self.P + 3
        self.add("var", np.full((self.N, G, G), INITIAL["var"], F), guard=GUARD_VALUE["var"])
        self.add("scan_var", np.full((self.N, self.var_stride), INITIAL["scan_var"], F), guard=GUARD_VALUE["scan_var"])
        self.fusion = dict(DEFAULTS, **(fusion or {}))
        ef = abi.LsimElevationMapFused()
        ef.em = self.em
        self.point(ef, ("var", "scan_var"))
        ef.var_stride = self.var_stride
        for k, v in self.fusion.items():
            setattr(ef, k, v)
        self.em = self.bind(ef, entry if device is not None else lib().emu_elevation_map_fused).em        # the inner struct, in place

    def launch(self, tick, flags=0, edit=None, stream=None, edit_fused=None):
        def edits(ef):
            ef.em.tick, ef.em.flags = tick, flags
            if edit:
                edit(ef.em)
            if edit_fused:
                edit_fused(ef)
        return super().launch(edit=edits, stream=stream)

    def read(self):
        out = super().read()
        out["var"] = self.get("var")
        rows = self.get("scan_var")
        out["scan_var"], out["scan_var_pad"] = rows[:, :self.P], rows[:, self.P:]
        return out


def fused_rig(fusion=None, **fixed):
    """a make_rig for the scenes of elevation_map_scenes"""
    return lambda N, G, dirs, pts, **kw: FusedRig(N, G, dirs, pts, **{"fusion": fusion, **fixed, **kw})


class RefFused:
    """the state of N envs in float64 with the bound of every float next to it, and `step`, one launch"""

    def __init__(self, N, par, like, fusion):
        self.N, self.par = N, par
        self.f = {k: float(F(v)) for k, v in dict(DEFAULTS, **(fusion or {})).items() if k != "count_cap"}
        self.cap = int(dict(DEFAULTS, **(fusion or {}))["count_cap"])
        self.height, self.var = like["height"].astype(np.float64), like["var"].astype(np.float64)
        self.e_h, self.e_v = np.zeros_like(self.height), np.zeros_like(self.var)
        self.stamp, self.cell = like["stamp"].copy(), like["cell"].copy()
        self.scan, self.scan_var, self.known = like["scan"].astype(np.float64), like["scan_var"].astype(np.float64), like["known"].copy()
        self.e_scan, self.e_sv = np.zeros_like(self.scan), np.zeros_like(self.scan_var)
        self.state = int(like["state"])
        self.exact_ties = False
        self.sums = {}                      # (e, ix, iy) -> (sum, count) of the last launch
        self.fused = {}                       # (e, ix, iy) -> whether the last launch fused

    def age(self, tick, stamp, mutant=None):
        a = (int(tick) % 2 ** 32 - int(stamp)) % 2 ** 32
        return float(a if mutant == "no_wrap" else a & 0x7FFFFFFF)

    def step(self, inp, tick, flags=0, mutant=None):
        par, G, f = self.par, self.par.G, self.f
        res = float(F(par.res))
        visited, fill, due = ER.due_set(self.N, par.env_stride, flags, inp["episode_length"], tick, par.period, par.stagger)
        self.sums, self.fused = {}, {}
        for e in np.nonzero(visited)[0]:
            rs, mt = inp["root_states"][e].astype(np.float64), inp["mount"][e].astype(np.float64)
            ok = bool(np.isfinite(rs[:7]).all() and np.isfinite(mt).all())
            if fill[e]:
                self.stamp[e] = -1
            if not ok:
                self.state += 1
                self.scan[e], self.known[e], self.scan_var[e] = 0.0, 0, f["var_max"]
                self.e_scan[e] = self.e_sv[e] = 0.0
                continue
            if due[e]:
                P, valid = ER.points(par, inp, e)
                valid &= np.isfinite(P).all(axis=1)
                cx, cy = (int(np.clip(np.floor(rs[k] * par.rinv), -40000, 40000)) for k in (0, 1))
                cells = {}
                for r in np.nonzero(valid)[0]:
                    fx, fy = np.floor(P[r, :2] * par.rinv)
                    if not (-32768 < fx < 32768 and -32768 < fy < 32768):
                        continue
                    ix, iy = int(fx), int(fy)
                    if -G // 2 <= ix - cx < G // 2 and -G // 2 <= iy - cy < G // 2:
                        cells.setdefault((ix, iy), []).append(float(F(P[r, 2])))
                for (ix, iy), zs in cells.items():
                    zs = np.array(zs)
                    zmax = zs.max()
                    df = zmax - zs
                    part = np.ones(len(zs), bool) if mutant == "sum_all" else (zs <= f["band"]) if mutant == "band_on_z" else (df <= f["band"])
                    part |= df == 0.0
                    q = np.floor(np.abs(df[part]) * 65536.0 + 0.5).astype(np.int64)
                    ssum, n = int(q.sum()), int(part.sum())
                    self.sums[e, ix, iy] = (ssum, n)
                    zm = zmax - (ssum / n) * 2.0 ** -16
                    e_zm = U * (abs(ssum / n) * 2.0 ** -16 + abs(zm))
                    X, Y = (ix + 0.5) * res, (iy + 0.5) * res
                    ex, ey = X - rs[0], Y - rs[1]
                    rho2 = ex * ex + ey * ey
                    e_rho = 2 * U * (abs(ex) * (abs(X) + abs(ex)) + abs(ey) * (abs(Y) + abs(ey))) + 3 * U * rho2
                    sigma = f["sigma0"] + f["sigma2"] * (rho2 + f["range_z2"])
                    e_sig = f["sigma2"] * e_rho + 3 * U * sigma
                    nc = n if mutant == "no_cap" else min(n, self.cap)
                    vm = sigma * sigma / nc + f["var_floor"]
                    e_vm = 2 * sigma * e_sig / nc + 3 * U * vm
                    s = (ix & (G - 1), iy & (G - 1))
                    h, var, e_h, e_v = zm, vm, e_zm, e_vm
                    fusedit = False
                    if self.stamp[e][s] >= 0 and self.cell[e][s] == ER.pack(ix, iy):
                        age = self.age(tick, self.stamp[e][s], mutant)
                        vp = self.var[e][s] + (0.0 if mutant == "no_growth" else f["var_growth"] * age)
                        e_vp = self.e_v[e][s] + 3 * U * vp
                        d = zm - self.height[e][s]
                        e_d = e_zm + self.e_h[e][s] + U * abs(d)
                        S = vp + vm
                        e_S = e_vp + e_vm + U * S
                        lhs, rhs = d * d, f["gate2"] * S
                        margin = 2 * abs(d) * e_d + f["gate2"] * e_S + 2 * U * (lhs + rhs)
                        exact_tie = self.exact_ties and lhs == rhs          # a scene whose operands are all dyadic says so
                        assert exact_tie or abs(lhs - rhs) > margin or f["gate2"] == 0.0, ("the scene leaves a gate decision ambiguous", e, ix, iy, lhs, rhs)
                        opens = True if mutant == "no_gate" else (lhs <= rhs) if mutant == "gate_inclusive" else (lhs < rhs)
                        if opens and np.isfinite(S):
                            K = (vm / S) if mutant == "K_swapped" else (vp / S)
                            e_K = e_vp / S + vp * e_S / (S * S) + U * K
                            h = self.height[e][s] + K * d
                            e_h = self.e_h[e][s] + abs(d) * e_K + K * e_d + U * abs(K * d) + U * abs(h)
                            var = K * vm
                            e_v = vm * e_K + K * e_vm + U * var
                            fusedit = True
                    if mutant != "no_clamp":
                        var = min(max(var, f["var_floor"]), f["var_max"])
                    self.fused[e, ix, iy] = fusedit
                    self.height[e][s], self.var[e][s], self.e_h[e][s], self.e_v[e][s] = h, var, e_h, e_v
                    self.stamp[e][s], self.cell[e][s] = np.int32(int(tick) & 0x7FFFFFFF), ER.pack(ix, iy)
            q = rs[3:7]
            with np.errstate(all="ignore"):
                qy = np.array([0.0, 0.0, q[2], q[3]]) / np.sqrt(q[2] ** 2 + q[3] ** 2)
                w = rs[:2] + ER.rot(qy, np.concatenate((par.pts, np.zeros((len(par.pts), 1))), axis=1))[:, :2]
                fl = np.floor(w * par.rinv)
            for j in range(len(par.pts)):
                self.scan[e, j], self.known[e, j], self.scan_var[e, j] = float(F(F(rs[2]) - F(par.unknown_drop))), 0, f["var_max"]
                self.e_scan[e, j] = self.e_sv[e, j] = 0.0
                if np.isfinite(fl[j]).all() and (np.abs(fl[j]) < 32768).all():
                    ix, iy = int(fl[j, 0]), int(fl[j, 1])
                    s = (ix & (G - 1), iy & (G - 1))
                    if self.stamp[e][s] >= 0 and self.cell[e][s] == ER.pack(ix, iy):
                        aged = self.var[e][s] + f["var_growth"] * self.age(tick, self.stamp[e][s], mutant)
                        self.scan[e, j], self.known[e, j], self.e_scan[e, j] = self.height[e][s], 1, self.e_h[e][s]
                        self.scan_var[e, j], self.e_sv[e, j] = (aged if mutant == "no_clamp" else min(aged, f["var_max"])), self.e_v[e][s] + 3 * U * aged
        return visited, fill, due


def worst_miss(got, ref):
    """the largest |got - ref| / (2 bound) over the four float outputs (where the slot / point is known); integers are asserted exact"""
    for k in ("stamp", "cell", "known"):
        np.testing.assert_array_equal(got[k], getattr(ref, k), err_msg=k)
    assert got["state"] == ref.state
    kn = ref.stamp >= 0
    worst = 0.0
    for name, val, err, mask in (("height", ref.height, ref.e_h, kn), ("var", ref.var, ref.e_v, kn), ("scan", ref.scan, ref.e_scan, None),
                                 ("scan_var", ref.scan_var, ref.e_sv, None)):
        g = got[name].astype(np.float64)
        assert np.isfinite(g[mask] if mask is not None else g).all(), name
        miss = np.abs(g - val) / (2.0 * err + 1e-300)
        miss = np.where(np.abs(g - val) == 0.0, 0.0, miss)
        worst = max(worst, float((miss[mask] if mask is not None else miss).max(initial=0.0)))
    return worst


def check_fused_bracket(par, fusion, inp, e, got, tick):
    """The comparison rule for general poses, on env e of ONE launch into an empty map (finite pose, due): every touched cell is a first
    write, height = zm and var = vm.  E = elevation_map_reference.eps, per component.  A point is AMBIGUOUS when it lies within E of a
    cell edge (it may belong to either cell: elevation_map_reference.bracket's rule) or when |zmax - z - band| <= 2 E for a zmax the cell
    can have (it may or may not take part; both z carry E).  Over every choice of the cell's edge points: zmax is the chosen points'
    maximum, the points surely inside the band take part, and the mean is highest without the band's ambiguous points and lowest with all
    of them (each lies below every sure one).  zm must lie between the lowest and the highest such mean, widened by E (the points'), 2^-16
    (two roundings of q) and 4 u |z|; the count between the smallest and largest, which brackets vm (its own arithmetic: the bound of
    RefFused, doubled).  Returns (ambiguous points, valid points): the share is a condition on the scene."""
    import itertools
    G = par.G
    f = {k: float(F(v)) for k, v in dict(DEFAULTS, **(fusion or {})).items() if k != "count_cap"}
    cap = int(dict(DEFAULTS, **(fusion or {}))["count_cap"])
    rs = inp["root_states"][e].astype(np.float64)
    E = ER.eps(rs[:3], inp["mount"][e][:3], par.t_hi)
    assert f["band"] > 4.0 * E
    P, valid = ER.points(par, inp, e)
    c = np.floor(rs[:2] * par.rinv).astype(np.int64)
    cells, ambiguous, n = {}, set(), 0
    for r in np.nonzero(valid)[0]:
        lo, hi = np.floor((P[r, :2] - E) * par.rinv).astype(np.int64), np.floor((P[r, :2] + E) * par.rinv).astype(np.int64)
        sure = bool((lo == hi).all())
        n += 1
        if not sure:
            ambiguous.add(r)
        for ix in {lo[0], hi[0]}:
            for iy in {lo[1], hi[1]}:
                if -G // 2 <= ix - c[0] < G // 2 and -G // 2 <= iy - c[1] < G // 2 and abs(ix) < 32768 and abs(iy) < 32768:
                    cells.setdefault((int(ix), int(iy)), ([], []))[0 if sure else 1].append((r, P[r, 2]))
    seen = np.zeros((G, G), bool)
    res = float(F(par.res))
    for (ix, iy), (S, M) in cells.items():
        s = (ix & (G - 1), iy & (G - 1))
        seen[s] = True
        knows = got["stamp"][e][s] >= 0
        assert len(M) <= 10, "a cell with more than 10 edge points: choose another scene"
        lo_h, hi_h, n_lo, n_hi = np.inf, -np.inf, 10 ** 9, 0
        for k in range(len(M) + 1):
            for chosen in itertools.combinations(M, k):
                pts = S + list(chosen)
                if not pts:
                    continue
                idx, zs = np.array([p[0] for p in pts]), np.array([p[1] for p in pts])
                df = zs.max() - zs
                inside, maybe = df < f["band"] - 2.0 * E, np.abs(df - f["band"]) <= 2.0 * E
                ambiguous.update(idx[maybe].tolist())
                hi_h, lo_h = max(hi_h, zs[inside].mean()), min(lo_h, zs[inside | maybe].mean())
                n_lo, n_hi = min(n_lo, int(inside.sum())), max(n_hi, int((inside | maybe).sum()))
        if S:
            assert knows, (e, ix, iy, "a cell with a sure point is unknown")
        if not knows:
            continue
        assert got["stamp"][e][s] == tick and got["cell"][e][s] == ER.pack(ix, iy), (e, ix, iy)
        h, v = float(got["height"][e][s]), float(got["var"][e][s])
        tol = E + 2.0 ** -16 + 4.0 * U * abs(h)
        assert lo_h - tol <= h <= hi_h + tol, (e, ix, iy, h, lo_h, hi_h, tol)
        X, Y = (ix + 0.5) * res, (iy + 0.5) * res
        ex, ey = X - rs[0], Y - rs[1]
        rho2 = ex * ex + ey * ey
        e_rho = 2 * U * (abs(ex) * (abs(X) + abs(ex)) + abs(ey) * (abs(Y) + abs(ey))) + 3 * U * rho2
        sigma = f["sigma0"] + f["sigma2"] * (rho2 + f["range_z2"])
        e_sig = f["sigma2"] * e_rho + 3 * U * sigma
        vm = lambda cnt: min(max(sigma * sigma / min(cnt, cap) + f["var_floor"], f["var_floor"]), f["var_max"])
        e_vm = 2.0 * (2 * sigma * e_sig + 3 * U * vm(1))
        assert vm(n_hi) - e_vm <= v <= vm(max(n_lo, 1)) + e_vm, (e, ix, iy, v, vm(n_hi), vm(n_lo), e_vm)
    assert (got["stamp"][e][~seen] == -1).all(), "a slot no point can reach was written"
    return len(ambiguous), n


# the general-pose scene on which the band matters: the synthetic ground's slope spreads a cell's points over up to 9 mm, and 3072 rays put
# several into most cells
DENSE, DENSE_FUSION = dict(seed=5, N=2, G=16, width=64, height=48), {"band": 0.006}


def general_poses(make_rig, N=5, G=16, width=16, height=12, seed=0, tick=7, fusion=None, **kw):
    """elevation_map_scenes.random_rig under the rule above, with a non-zero band: one FILL_ALL launch into an empty map; the scan's height
    and known against the launch's own arrays as the plain map's scene does, scan_var against the launch's own var (the age is 0).
    Returns (read, the scene's ambiguous share)"""
    import elevation_map_scenes as ES
    rig = ES.random_rig(make_rig, N, G, width, height, seed, **kw)
    par, inp = ER.Params.of(rig), rig.inputs()
    assert rig.launch(tick, ER.FILL_ALL) == 0
    got = rig.read()
    amb = n = 0
    for e in range(0, N, par.env_stride):
        a_, n_ = check_fused_bracket(par, fusion, inp, e, got, tick)
        amb, n = amb + a_, n + n_
        ES.check_scan(par, inp, e, got)
        kn = got["known"][e] != 0
        assert np.isin(got["scan_var"][e][kn], got["var"][e][got["stamp"][e] >= 0]).all() and (got["scan_var"][e][~kn] == F(dict(DEFAULTS, **(fusion or {}))["var_max"])).all()
    share = amb / max(n, 1)
    assert share <= 0.01, f"{share:.4f} of the scene's points are ambiguous: choose another seed"
    return got, share


def rows_fused(scan, known, pose_z, scan_var, z_offset, scale, var_ref):
    """lsim_map_rows_fused with channels == 2 in numpy: fp32 operations in the header's order, one correctly rounded quotient"""
    z, s = pose_z.astype(F)[:, None], scan.astype(F)
    with np.errstate(all="ignore"):
        t = (z - F(z_offset)).astype(F) - s
        first = np.where(np.isfinite(z) & np.isfinite(s), np.clip(t, F(-1), F(1)) * F(scale), F(0)).astype(F)
        sv = scan_var.astype(F)
        denom = (F(var_ref) + sv).astype(F)
        conf = (np.float64(F(var_ref)) / denom.astype(np.float64)).astype(F)
        second = np.where((known != 0) & np.isfinite(sv) & (sv >= 0), conf, F(0)).astype(F)
    return np.concatenate((first, second), axis=1)
