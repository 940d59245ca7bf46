"""TEST INFRASTRUCTURE -- float64 reference of the elevation map's visibility clean-up, written from the comment of
lsim_elevation_map_cleanup in include/lsim.h (not from the kernel source), on top of elevation_map_reference (the rules the map launches
share), and CleanupRig: elevation_map_emu_binding.Rig with the clean-up's struct, its `cleared` row and an optional `var`, guarded like the
others, which can launch the map's own entry point on the same arrays too.

What the launch writes are integers (stamps, counts), so the comparison is a BRACKET.  For every used ray and every slot that knows its
window cell the reference decides, in float64 from the fp32 inputs, between three answers -- the ray certainly counts for the cell,
certainly does not, or the pair is AMBIGUOUS:
  * position.  The launch's O and E carry elevation_map_reference.eps (its docstring: u (2 |p|_inf + 120 (|mpos| + t_hi)) metres, the two
    rotations and the sums of P); in cell units dc = EPS rinv + u max(|o|, |e|) (the product with rinv).  u_a = (b - o_a) (1 / d_a) has three
    more roundings, 4 u |u_a| <= 4 u: a displacement of at most 4 u len cells along a segment of len cells.  DELTA = 4 dc + 8 u len is twice
    what the boundary of a cell can move against the segment.  The ray POSSIBLY crosses a cell when the float64 segment meets the cell
    grown by DELTA on every side, and CERTAINLY when it runs for a positive length through the cell shrunk by DELTA; the launch's u_in
    and u_out then lie between the two intersections' parameters.  (A cell whose centre is further than 0.75 + DELTA cells from the
    segment -- half a diagonal is 0.71 -- cannot be met and is left out of the arithmetic.)
  * the walk's cap.  Cell (ix, iy) is the (|ix - ix0| + |iy - iy0| + 1)-th cell of the walk; 2 G + 2 are visited.  Certain needs that
    Manhattan distance <= 2 G - 1, possible <= 2 G + 3 (the first cell itself may be off by one per axis).
  * height.  val = max(z(u_in), z(u_out)) + clear_slope L u_out is monotone in u_in and in u_out, so over the box of parameters its extremes
    lie at the corners (a ray that only possibly crosses: min over the grown intersection).  Rounding: z(u) two operations on
    |O.z| + |dz|, each carrying EPS; L three; the products and the sum with clear_slope three; thr three on |height| + margin + sigma sqrt(var):
    EPS_z = 3 EPS + 8 u (|O.z| + |dz| + clear_slope L + |thr| + clear_margin + clear_sigma sqrt(var)).
    certain:  certainly crossed and val_max + EPS_z < thr;      not:  not possibly crossed, or val_min - EPS_z >= thr, or thr NaN;      else ambiguous.
A slot MUST be forgotten when its certain rays number >= min_rays, MUST NOT when certain + ambiguous < min_rays; otherwise either passes and
the slot is counted as ambiguous.  The tests insist that at most 1 % of the known slots are.  Nothing here has seen the launch's output.

MUTANTS: deliberately wrong variants of this reference, each caught by a scene of elevation_cleanup_scenes (test_elevation_cleanup.py):
  hi_min (min for max in hi)             planted_block       no_end_gap (E = the ray's own end)        planted_block
  no_slope (the slope term dropped)      slope_term          window_on_end (the ray's end must lie in the window)   end_outside_window
  clean_fresh (fresh envs are cleaned)   due_sets            min_rays_strict (count > min_rays)        planted_block"""
import ctypes

import numpy as np

import elevation_map_emu_binding as EB
import elevation_map_reference as ER
import emu_binding
from helpers import abi

F = np.float32
U = 2.0 ** -24
MUTANTS = ("hi_min", "no_end_gap", "no_slope", "window_on_end", "clean_fresh", "min_rays_strict")
DEFAULTS = dict(clear_margin=0.05, clear_slope=0.05, clear_sigma=3.0, end_gap=1.5 * 2.0 ** -4, min_rays=2)
GUARD_VALUE = {"cleared": 0x3C3C3C3C, "var": -77.25}
INITIAL = {"cleared": 11, "var": 0.0}
_lib = None


def lib():
    """tests/emu/emu_elevation_cleanup.cpp built and bound, the point hook typed by hand (it is no entry point of lsim.h)"""
    global _lib
    if _lib is None:
        _lib = emu_binding.load_shim("elevation_cleanup", ["ls_raycast.h", "ls_raycast_bodies.h", "ls_sensor_model.h", "ls_math.h", "ls_elevation_map.h", "ls_elevation_cleanup.h"])
        _lib.emu_elevation_cleanup_point.restype = ctypes.c_int
        _lib.emu_elevation_cleanup_point.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int),
                                                     ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float)]
    return _lib


class CleanupRig(EB.Rig):
    """Rig with cleared [N] (guarded), var [N, G, G] when `var` (guarded: the launch only reads it) and the clean-up's struct; `cleanup`:
    its by-value fields (DEFAULTS).  launch() is the clean-up, map_launch() the map's own launch on the same arrays (`map_entry`: the
    library's lsim_elevation_map on a device).  `edit` sees the inner lsim_elevation_map_t, `edit_cleanup` the whole struct."""

    def __init__(self, N, G, dirs, pts, cleanup=None, var=False, device=None, entry=None, map_entry=None, **kw):
        super().__init__(N, G, dirs, pts, device=device, entry=map_entry, **kw)
        self._map_entry = self._entry
        self.add("cleared", np.full(self.N, INITIAL["cleared"], np.int32), guard=GUARD_VALUE["cleared"])
        if var:
            self.add("var", np.full((self.N, G, G), INITIAL["var"], F), guard=GUARD_VALUE["var"])
        self.cleanup = dict(DEFAULTS, **(cleanup or {}))
        ec = abi.LsimElevationMapCleanup()
        ec.em = self.em
        self.point(ec, ("var", "cleared"))
        for k, v in self.cleanup.items():
            setattr(ec, k, v)
        self.em = self.bind(ec, entry if device is not None else lib().emu_elevation_map_cleanup).em        # the inner struct, in place

    def launch(self, tick, flags=0, edit=None, stream=None, edit_cleanup=None, entry=None):
        def edits(ec):
            ec.em.tick, ec.em.flags = tick, flags
            if edit:
                edit(ec.em)
            if edit_cleanup:
                edit_cleanup(ec)
        return super().launch(edit=edits, stream=stream, entry=entry)

    def map_launch(self, tick, flags=0, stream=None):
        """lsim_elevation_map on the same arrays: the struct opens with the map's own"""
        s = type(self.struct).from_buffer_copy(self.struct)
        s.em.tick, s.em.flags = tick, flags
        return self._map_entry(ctypes.byref(s.em), self.stream(stream))

    def read(self):
        out = super().read()
        out["cleared"] = self.get("cleared")
        if "var" in self.a:
            out["var"] = self.get("var")
        return out

    def params(self):
        """the clean-up's by-value fields as the launch sees them (fp32)"""
        return {k: (int(v) if k == "min_rays" else float(F(v))) for k, v in self.cleanup.items()}


def cleanup_rig(cleanup=None, **fixed):
    """a make_rig for the scenes"""
    return lambda N, G, dirs, pts, **kw: CleanupRig(N, G, dirs, pts, **{"cleanup": cleanup, **fixed, **kw})


def window_cells(par, rs):
    """(ix, iy) [G, G] int64: the window cell that lives in each slot, for a robot at rs"""
    G = par.G
    c = np.clip(np.floor(rs[:2].astype(np.float64) * par.rinv), -40000, 40000).astype(np.int64)
    w = c - G // 2
    s = np.arange(G, dtype=np.int64)
    ix = w[0] + ((s - w[0]) & (G - 1))
    iy = w[1] + ((s - w[1]) & (G - 1))
    return np.broadcast_to(ix[:, None], (G, G)), np.broadcast_to(iy[None, :], (G, G))


def _slab(o, d, lo, hi):
    """the parameters at which o + u d, u in [0, 1], enters and leaves the boxes [lo, hi], pair by pair: o [1, 2], d, lo, hi [M, 2] -> u_in, u_out [M]"""
    with np.errstate(all="ignore"):
        ua, ub = (lo - o) / d, (hi - o) / d
    still, inside = np.broadcast_to(d == 0.0, ua.shape), (o >= lo) & (o <= hi)
    near = np.where(still, np.where(inside, -np.inf, np.inf), np.minimum(ua, ub))
    far = np.where(still, np.where(inside, np.inf, -np.inf), np.maximum(ua, ub))
    return np.maximum(0.0, near.max(axis=-1)), np.minimum(1.0, far.min(axis=-1))


def classify(par, cp, inp, before, e, mutant=None):
    """env e, worked on: (known [G, G] bool, certain [G, G] int, ambiguous [G, G] int) -- the rays that certainly, and that perhaps, count
    for each slot that knows its window cell (the module docstring's rule)"""
    G = par.G
    rs, mt = inp["root_states"][e].astype(np.float64), inp["mount"][e].astype(np.float64)
    EPS = ER.eps(rs[:3], mt[:3], par.t_hi)
    wix, wiy = window_cells(par, rs)
    known = (before["stamp"][e] >= 0) & (before["cell"][e] == ER.pack(wix, wiy))
    certain, ambiguous = np.zeros((G, G), np.int64), np.zeros((G, G), np.int64)
    if not known.any():
        return known, certain, ambiguous
    height = before["height"][e].astype(np.float64)[known]
    spread = cp["clear_sigma"] * np.sqrt(before["var"][e].astype(np.float64)[known]) if "var" in before else np.zeros_like(height)
    with np.errstate(all="ignore"):
        thr = height - cp["clear_margin"] - spread
    cells = np.stack((wix[known], wiy[known]), axis=-1).astype(np.float64)            # [K, 2]
    with np.errstate(all="ignore"):
        d = par.a * inp["depth"][e].astype(np.float64) + par.b
        t = d if par.inv_scale is None else d * par.inv_scale
        used = np.isfinite(d) & (np.abs(d) <= np.finfo(F).max) & (par.t_lo < t) & (t < par.t_hi)
        if inp.get("labels") is not None:
            used &= inp["labels"][e] == 1
        gap = 0.0 if mutant == "no_end_gap" else cp["end_gap"]
        used &= t > gap
        te = np.where(used, t - gap, 0.0)
        O = rs[:3] + ER.rot(rs[3:7], mt[:3])
        E = rs[:3] + ER.rot(rs[3:7], mt[:3] + ER.rot(mt[3:7], par.dirs * te[:, None]))
        used &= np.isfinite(E).all(axis=1) & bool(np.isfinite(O).all())
        if mutant == "window_on_end":
            P = rs[:3] + ER.rot(rs[3:7], mt[:3] + ER.rot(mt[3:7], par.dirs * np.where(used, t, 0.0)[:, None]))
            c = np.floor(rs[:2] * par.rinv)
            rel = np.floor(P[:, :2] * par.rinv) - c
            used &= ((rel >= -G // 2) & (rel < G // 2)).all(axis=1)
    r = np.nonzero(used)[0]
    if not len(r):
        return known, certain, ambiguous
    o, en = O[:2] * par.rinv, E[r, :2] * par.rinv
    assert (np.abs(np.floor(o)) < 32768).all() and (np.abs(np.floor(en)) < 32768).all(), "the scene keeps every segment inside the packed range"
    dxy = en - o
    length = np.linalg.norm(dxy, axis=1)
    dc = EPS * par.rinv + U * max(np.abs(o).max(), np.abs(en).max())
    # only the (ray, cell) pairs whose cell centre lies within reach of the segment are worked out: the others are certainly not crossed
    DELTA = 4.0 * dc + 8.0 * U * length                                              # [R]
    rel = cells[None] + 0.5 - o[None, None, :]                                        # [R, K, 2] by broadcasting below
    safe = np.maximum(length, 1e-300)[:, None]
    across = np.abs(rel[..., 0] * dxy[:, None, 1] - rel[..., 1] * dxy[:, None, 0]) / safe
    along = (rel[..., 0] * dxy[:, None, 0] + rel[..., 1] * dxy[:, None, 1]) / safe
    reach = 0.75 + DELTA[:, None]
    ri, ki = np.nonzero((across <= reach) & (along >= -reach) & (along <= length[:, None] + reach))
    dl = DELTA[ri, None]
    o3, d3, lo, hi = o[None, :], dxy[ri], cells[ki], cells[ki] + 1.0
    gin, gout = _slab(o3, d3, lo - dl, hi + dl)                  # the cell grown: possible
    sin, sout = _slab(o3, d3, lo + dl, hi - dl)                  # the cell shrunk: certain
    steps = np.abs(cells[ki] - np.floor(o)[None]).sum(axis=1)
    possible = (gout >= gin) & (steps <= 2 * G + 3)
    sure = (sout > sin) & (steps <= 2 * G - 1)
    Oz, dz, L = O[2], (E[r, 2] - O[2])[ri], np.linalg.norm(E[r, :2] - O[:2], axis=1)[ri]
    slope = 0.0 if mutant == "no_slope" else cp["clear_slope"]
    pick = np.minimum if mutant == "hi_min" else np.maximum

    def val(ui, uo):
        return pick(Oz + ui * dz, Oz + uo * dz) + slope * L * uo
    with np.errstate(all="ignore"):
        corners = np.stack([val(a, b) for a in (gin, sin) for b in (sout, gout)])
        vmax = corners.max(axis=0)
        vmin = np.where(sure, corners.min(axis=0), np.minimum(Oz + gin * dz, Oz + gout * dz) + slope * L * gin)
        EZ = 3.0 * EPS + 8.0 * U * (abs(Oz) + np.abs(dz) + cp["clear_slope"] * L + np.abs(thr)[ki] + cp["clear_margin"] + spread[ki])
        ok = np.isfinite(thr)[ki]
        yes = sure & ok & (vmax + EZ < thr[ki])
        no = ~possible | ~ok | (vmin - EZ >= thr[ki])
    K = len(thr)
    certain[known] = np.bincount(ki[yes], minlength=K)
    ambiguous[known] = np.bincount(ki[~yes & ~no], minlength=K)
    return known, certain, ambiguous


def check(par, cp, inp, before, after, tick, flags=0, mutant=None):
    """one launch's output against the header: which envs are touched at all, what is never written, and per worked env the bracket.
    Returns (ambiguous slots, known slots, slots forgotten [N])"""
    N = before["stamp"].shape[0]
    visited, fill, due = ER.due_set(N, par.env_stride, flags, inp["episode_length"], tick, par.period, par.stagger)
    for k in ("height", "cell", "scan", "known", "scan_pad", "known_pad") + (("var",) if "var" in before else ()):
        np.testing.assert_array_equal(ER.bits(after[k]), ER.bits(before[k]), err_msg=f"{k} is never written")
    assert after["state"] == before["state"], "a bad pose is not counted by this launch"
    amb = n = 0
    gone = np.zeros(N, np.int64)
    need = cp["min_rays"] + (1 if mutant == "min_rays_strict" else 0)
    for e in range(N):
        rs, mt = inp["root_states"][e], inp["mount"][e]
        ok = bool(np.isfinite(rs[:7]).all() and np.isfinite(mt).all())
        fresh = bool(fill[e])
        worked = bool(due[e]) and ok and (not fresh or mutant == "clean_fresh")
        if not worked:
            np.testing.assert_array_equal(after["stamp"][e], before["stamp"][e], err_msg=f"env {e} is not worked on")
            assert after["cleared"][e] == (0 if fresh else before["cleared"][e]), (e, "cleared of an env that is not worked on")
            continue
        known, certain, ambiguous = classify(par, cp, inp, before, e, mutant)
        changed = after["stamp"][e] != before["stamp"][e]
        assert (after["stamp"][e][changed] == -1).all() and (before["stamp"][e][changed] >= 0).all(), (e, "a stamp only ever becomes -1")
        assert not changed[~known].any(), (e, "a slot that does not know its window cell was touched")
        must, may = known & (certain >= need), known & (certain + ambiguous >= need)
        assert changed[must].all(), (e, "not forgotten", np.argwhere(must & ~changed)[:4].tolist())
        assert not changed[~may].any(), (e, "forgotten", np.argwhere(changed & ~may)[:4].tolist())
        gone[e] = int(changed.sum())
        assert after["cleared"][e] == (0 if fresh else before["cleared"][e]) + gone[e], (e, "cleared grows by the slots forgotten")
        amb, n = amb + int((may & ~must).sum()), n + int(known.sum())
    return amb, n, gone
