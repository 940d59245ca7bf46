"""TEST INFRASTRUCTURE -- the scenes of the elevation-map launch, shared by the CPU tests (the shim) and the GPU tests (the library): each
takes `make_rig` (elevation_map_emu_binding.Rig or its device form), drives launches, checks them against elevation_map_reference and
returns what it read, so a GPU test can also compare the device's output with the CPU build's.

Exact scenes are dyadic (the reference's docstring): res = 2^-4, everything else a multiple of 2^-6, quaternions the identity and
(0, 0, 1, 0); they are compared bit for bit.  `mutant` runs the reference with one of its MUTANTS in place of the header's rule: the
comparison must then fail somewhere (tests/test_elevation_map.py)."""
import numpy as np

import elevation_map_reference as ER
import sensor_model_reference as SR

F = np.float32
RES = 2.0 ** -4
Q = 2.0 ** -6
YAW_PI = (0.0, 0.0, 1.0, 0.0)
# eight axis-parallel and diagonal directions with dyadic components (not unit: the launch uses dirs as given)
DIRS8 = np.array([[1, 0, -0.5], [1, 0.25, -0.5], [0.5, -1, -0.25], [-1, 0, -0.5], [0, 1, -0.75], [1, 0, -0.5], [0.75, 0.25, -0.5], [-0.5, -0.5, -1]], F)
PTS = np.array([[0, 0], [0.5, 0], [0.5, 0.25], [-0.5, 0], [0, 0.5], [-0.25, -0.5], [0.375, 0.125], [4.0, 4.0], [0.5 - Q, 0], [-0.5, -0.5]], F)


def _pose(rig, e, pos, quat=(0, 0, 0, 1)):
    rs = rig.get("root_states")
    rs[e, :3], rs[e, 3:7] = pos, quat
    rig.put("root_states", rs)


def _launch_and_compare(rig, ref, tick, flags=0, mutant=None, what=""):
    assert rig.launch(tick, flags) == 0
    sets = ref.step(rig.inputs(), tick, flags, mutant)
    got = rig.read()
    ER.assert_same(got, ref, f"{what} tick {tick}")
    return got, sets


def _start(make_rig, N, G, dirs=DIRS8, pts=PTS, **kw):
    rig = make_rig(N, G, dirs, pts, res=RES, **kw)
    return rig, ER.RefMap(N, ER.Params.of(rig), rig.read())


def exact_depths(N, R, seed=0):
    """[N, R] multiples of 2^-6 in [0.5, 2.5): several rays share a cell, none is a miss"""
    g = np.random.RandomState(seed)
    return (g.randint(32, 160, (N, R)) * Q).astype(F)


def exact_basic(make_rig, mutant=None, reverse=False, stream=None):
    """N = 3, G = 16, R = 8: three poses (one with negative coordinates, one turned by pi), two captures each; with `reverse` the rays run
    backwards -- the state must be the same bits"""
    N, G = 3, 16
    order = slice(None, None, -1) if reverse else slice(None)
    rig, ref = _start(make_rig, N, G, dirs=DIRS8[order])
    depth = exact_depths(N, 8) * F(0.25)
    depth[0, 0], depth[0, 5] = 2 * RES, 2 * RES + Q     # rays 0 and 5 share a direction and here a cell (x = 0.75 + t); the later one is lower
    depth[1, 5] = depth[1, 0]
    rig.put("depth", depth[:, order])
    for e, (pos, quat) in enumerate((((0.5, 0.25, 0.5), (0, 0, 0, 1)), ((-3.0 - 3 * Q, -1.5 + Q, 0.375), YAW_PI), ((20.0 + Q, -7.25, 0.25), (0, 0, 0, 1)))):
        _pose(rig, e, pos, quat)
    mt = rig.get("mount")
    mt[:, :3] = (0.25, 0.0, 0.125)
    rig.put("mount", mt)
    got1, _ = _launch_and_compare(rig, ref, 4, 0, mutant, "first capture")
    assert ((got1["stamp"] == 4).sum(axis=(1, 2)) >= 2).all()
    rig.put("depth", (depth[:, order] + F(4 * Q)))
    for e in range(N):
        rs = rig.get("root_states")
        _pose(rig, e, rs[e, :3] + np.array([2 * RES, -RES, Q], F), rs[e, 3:7])
    got2, _ = _launch_and_compare(rig, ref, 5, 0, mutant, "second capture")
    assert ((got2["stamp"] == 4).sum(axis=(1, 2)) > 0).all(), "cells of the first capture are still held"
    return got2


def window_edges(make_rig, mutant=None):
    """points at ix - cx = -G/2 (kept), G/2 - 1 (kept), G/2 (not), -G/2 - 1 (not), in x and in y, with the robot in a negative cell"""
    G = 16
    dirs = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]] * 2, F)
    rig, ref = _start(make_rig, 1, G, dirs=dirs)
    _pose(rig, 0, (-1.0 + RES / 2, -2.0 + RES / 2, 0.5))
    half = G // 2 * RES
    rig.put("depth", np.array([[half - RES, half, half - RES, half, half, half + RES, half, half + RES]], F))
    got, _ = _launch_and_compare(rig, ref, 1, 0, mutant, "window edges")
    assert (got["stamp"] == 1).sum() == 4
    return got


def negative_coordinates(make_rig, mutant=None):
    """points whose x / res and y / res are negative and not whole: floor and truncation differ"""
    rig, ref = _start(make_rig, 1, 16)
    _pose(rig, 0, (-0.5 - Q, -0.25 - Q, 0.5))
    rig.put("depth", exact_depths(1, 8, seed=3) * F(0.25))
    got, _ = _launch_and_compare(rig, ref, 2, 0, mutant, "negative coordinates")
    assert (got["stamp"] == 2).sum() >= 4
    return got


def scrolling(make_rig, G=16, mutant=None):
    """the robot moves by 1, G - 1, G and G + 3 cells between captures: cells still in the window keep their bits (the reference keeps them
    too and is compared bit for bit), re-used slots read unknown until rewritten"""
    rig, ref = _start(make_rig, 2, G)
    depth = exact_depths(2, 8, seed=5) * F(0.5)
    rig.put("depth", depth)
    x = np.array([0.5 + Q, -0.5 + Q])
    out = []
    for k, move in enumerate((0, 1, G - 1, G, G + 3)):
        x = x + move * RES
        for e in range(2):
            _pose(rig, e, (x[e], 0.25 * (e + 1) + Q, 0.5), YAW_PI if e else (0, 0, 0, 1))
        before = rig.read()
        got, _ = _launch_and_compare(rig, ref, 10 + k, 0, mutant, f"scroll by {move}")
        kept = got["stamp"] != 10 + k
        for name in ("height", "cell", "stamp"):
            np.testing.assert_array_equal(ER.bits(got[name][kept]), ER.bits(before[name][kept]))
        out.append(got)
    # after the last move no cell of the first capture is inside the window: a scan point over such a slot reads unknown
    rig.put("depth", 1e9)
    got, _ = _launch_and_compare(rig, ref, 20, 0, mutant, "scan after scrolling")
    ix = (got["cell"] >> 16).astype(np.int64) - 32768
    stale = (got["stamp"] >= 0) & (np.abs(ix - np.floor(x / RES).astype(np.int64)[:, None, None]) > G)
    assert stale.any(), "slots written before the window moved on are still there, and read unknown (the reference says so bit for bit)"
    out.append(got)
    return out


def due_sets(make_rig, flags=0, stagger=0, env_stride=1, N=7, mutant=None):
    """period 3: over six ticks the launch's due set is the capture's rule; a not-due env keeps its three arrays (bits) and has its scan
    rewritten from its new pose; episode_length 0 clears, then inserts; rows of unvisited envs and every guard stay"""
    rig, ref = _start(make_rig, N, 16, period=3, stagger=stagger, env_stride=env_stride)
    rig.put("depth", exact_depths(N, 8, seed=7) * F(0.5))
    for e in range(N):
        _pose(rig, e, (e * 0.5 + Q, -e * 0.25 + Q, 0.5))
    _launch_and_compare(rig, ref, 0, ER.FILL_ALL, mutant, "fill")
    seen = np.zeros(N, bool)
    out = []
    for tick in range(1, 7):
        el = np.ones(N, np.int64)
        if tick == 4:
            el[[0, N - 1]] = 0
        rig.put("episode_length", el)
        for e in range(N):
            _pose(rig, e, (e * 0.5 + Q + tick * RES, -e * 0.25 + Q, 0.5 + tick * Q))
        before = rig.read()
        got, (visited, fill, due) = _launch_and_compare(rig, ref, tick, flags, mutant, f"due set flags {flags}")
        np.testing.assert_array_equal(due, SR.due_sets(N, env_stride, tick, 3, stagger, flags, el)[0])      # the capture's own reference
        wrote = (got["stamp"] == tick).any(axis=(1, 2))
        np.testing.assert_array_equal(wrote, due)
        for name in ("height", "cell", "stamp"):
            np.testing.assert_array_equal(ER.bits(got[name][~due]), ER.bits(before[name][~due]))
        assert (got["scan"][visited & ~due] != before["scan"][visited & ~due]).any(axis=1).all(), "the scan of a not-due env follows its pose"
        for name in ("scan", "known"):
            np.testing.assert_array_equal(ER.bits(got[name][~visited]), ER.bits(before[name][~visited]))
            np.testing.assert_array_equal(ER.bits(got[name + "_pad"]), ER.bits(before[name + "_pad"]))
        for e in np.nonzero(fill)[0]:
            assert ((got["stamp"][e] == tick) | (got["stamp"][e] == -1)).all(), "a reset env holds this capture only"
        seen |= due
        out.append(got)
    assert (seen == (np.arange(N) % env_stride == 0)).all() or flags == ER.RESETS_ONLY
    return out


def invalid_rays(make_rig, mutant=None):
    """one env per way a ray can be invalid: nothing is inserted; the last env has a valid ray, to show the scene can insert at all"""
    ways = ("miss", "t <= t_lo", "dropped", "nan", "inf", "label 0", "label 2", "label 255", "valid")
    N = len(ways)
    rig, ref = _start(make_rig, N, 16, dirs=np.array([[1, 0, -0.5]], F), labels=True, t_lo=0.3125, t_hi=4.0, inv_scale=np.array([1.25], F), a=2.0, b=0.125)
    # d = 2 * stored + 0.125, t = 1.25 d: 0.0625 -> t = t_lo exactly, -0.0625 -> d = 0 (a dropped pixel reads drop_value)
    stored = {"miss": 2.0, "t <= t_lo": 0.0625, "dropped": -0.0625, "nan": np.nan, "inf": np.inf, "label 0": 0.125, "label 2": 0.125, "label 255": 0.125, "valid": 0.125}
    rig.put("depth", np.array([[stored[w]] for w in ways], F))
    lab = np.ones((N, 1), np.uint8)
    lab[ways.index("label 0")], lab[ways.index("label 2")], lab[ways.index("label 255")] = 0, 2, 255
    rig.put("labels", lab)
    for e in range(N):
        _pose(rig, e, (0.5 + Q, 0.25 + Q, 0.5))
    got, _ = _launch_and_compare(rig, ref, 3, 0, mutant, "invalid rays")
    wrote = (got["stamp"] >= 0).any(axis=(1, 2))
    np.testing.assert_array_equal(wrote, np.array([w == "valid" for w in ways]))
    return got


def nonfinite_pose(make_rig, mutant=None):
    """a non-finite component of the root pose or of the assumed mount: nothing inserted, a zero scan row with known 0, one count per launch;
    q.z = q.w = 0 is a finite pose whose scan points are not: they read unknown"""
    N = 5
    rig, ref = _start(make_rig, N, 16)
    rig.put("depth", exact_depths(N, 8, seed=11) * F(0.5))
    for e in range(N):
        _pose(rig, e, (0.5 + Q, 0.25 + Q, 0.5))
    _launch_and_compare(rig, ref, 0, ER.FILL_ALL, mutant, "before")
    rs, mt = rig.get("root_states"), rig.get("mount")
    rs[0, 1], rs[1, 6], mt[2, 4] = np.nan, np.inf, -np.inf
    rs[3, 3:7] = (1.0, 0.0, 0.0, 0.0)
    rig.put("root_states", rs)
    rig.put("mount", mt)
    before = rig.read()
    got, _ = _launch_and_compare(rig, ref, 1, 0, mutant, "non-finite poses")
    assert got["state"] == 3 and (got["scan"][:3] == 0).all() and (got["known"][:4] == 0).all()
    assert (got["scan"][3] == F(0.0)).all() and np.isfinite(got["scan"]).all() and np.isfinite(got["height"]).all()
    for name in ("height", "cell", "stamp"):
        np.testing.assert_array_equal(ER.bits(got[name][:3]), ER.bits(before[name][:3]))
    got, _ = _launch_and_compare(rig, ref, 2, ER.FILL_ALL, mutant, "non-finite poses, fill")
    assert got["state"] == 6 and (got["stamp"][:3] == -1).all()
    return got


def scan_frame(make_rig, mutant=None):
    """the scan turns with the yaw of q only: q = (0.5, 0.5, 0, 0.5) (not unit; the launch uses q as given) has qy = (0, 0, 0, 1) exactly"""
    dirs = np.array([[1, 0, -1], [0, 1, -1], [-1, 0, -1], [0, -1, -1]], F)
    pts = np.array([[0.25, 0], [0, 0.25], [-0.25, 0], [0, -0.25], [0.25, 0.25]], F)
    rig, ref = _start(make_rig, 1, 16, dirs=dirs, pts=pts)
    _pose(rig, 0, (0.5 + Q, 0.25 + Q, 0.5))
    rig.put("depth", 0.25)
    _launch_and_compare(rig, ref, 0, ER.FILL_ALL, mutant, "insert")
    rig.put("depth", 1e9)
    _pose(rig, 0, (0.5 + Q, 0.25 + Q, 0.5), (0.5, 0.5, 0.0, 0.5))
    got, _ = _launch_and_compare(rig, ref, 1, 0, mutant, "scan frame")
    np.testing.assert_array_equal(got["known"][0], [1, 1, 1, 1, 0])
    return got


def big_ticks(make_rig, mutant=None):
    """ticks whose low word has bit 31 set: the stamp is the low 31 bits, never negative, and the capture's cells are known"""
    rig, ref = _start(make_rig, 1, 16)
    _pose(rig, 0, (0.5 + Q, 0.25 + Q, 0.5))
    rig.put("depth", exact_depths(1, 8, seed=13) * F(0.25))
    for tick in (2 ** 31 + 5, 2 ** 32 - 1, 2 ** 63 - 1):
        got, _ = _launch_and_compare(rig, ref, tick, ER.FILL_ALL, mutant, "big tick")
        assert set(np.unique(got["stamp"])) == {-1, tick & 0x7FFFFFFF} and (got["stamp"] >= 0).sum() >= 2
    return got


# ---- general poses: the comparison rule of the reference's docstring
def camera_dirs(width, height, hfov_deg=87.0):
    tx = np.tan(np.radians(hfov_deg) / 2.0)
    ys = (1.0 - (2.0 * np.arange(width) + 1.0) / width) * tx
    zs = (1.0 - (2.0 * np.arange(height) + 1.0) / height) * tx * height / width
    v = np.stack((np.ones((height, width)), np.broadcast_to(ys[None, :], (height, width)), np.broadcast_to(zs[:, None], (height, width))), axis=-1)
    n = np.linalg.norm(v, axis=-1, keepdims=True)
    return (v / n).reshape(-1, 3).astype(F), n.reshape(-1).astype(F)


def random_rig(make_rig, N, G, width, height, seed, far_env=True, res=RES, **kw):
    """a pitched camera over a bumpy synthetic ground: roll and pitch up to 0.4 rad, any yaw, one env 190 m from the origin; the stored
    depth is the z-depth of the ray's meeting with z = 0.05 sin(3 x) cos(2 y) near enough (the launch does not care where depths come from)"""
    g = np.random.RandomState(seed)
    dirs, inv_scale = camera_dirs(width, height)
    R = dirs.shape[0]
    pts = np.stack(np.meshgrid(np.linspace(-0.8, 0.8, 6), np.linspace(-0.5, 0.5, 5), indexing="ij"), axis=-1).reshape(-1, 2)
    rig = make_rig(N, G, dirs, pts, res=res, inv_scale=inv_scale, t_lo=0.05, t_hi=4.9, unknown_drop=0.4, **kw)
    rs = rig.get("root_states")
    cells = g.randint(-40, 40, (N, 2))
    if far_env:
        cells[N - 1] = (int(190.0 / res), -int(190.0 / res))
    rs[:, :2] = (cells + 0.5) * res                 # the robot's own cell is unambiguous (the reference insists)
    rs[:, 2] = g.uniform(0.3, 0.5, N)
    roll, pitch, yaw = g.uniform(-0.4, 0.4, N), g.uniform(-0.4, 0.4, N), g.uniform(-np.pi, np.pi, N)
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    rs[:, 3:7] = np.stack((sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy), axis=1)
    rig.put("root_states", rs)
    mt = rig.get("mount")
    h = np.radians(60.0) / 2.0
    mt[:] = (0.3, 0.0, 0.05, 0.0, np.sin(h), 0.0, np.cos(h))
    rig.put("mount", mt)
    rs, mt = rs.astype(np.float64), mt.astype(np.float64)
    d = ER.rot(rs[:, None, 3:7], ER.rot(mt[:, None, 3:7], dirs[None].astype(np.float64)))
    o = rs[:, None, :3] + ER.rot(rs[:, None, 3:7], mt[:, None, :3])
    with np.errstate(all="ignore"):
        t = np.where(d[..., 2] < -0.05, -o[..., 2] / d[..., 2], 1e9)
        hit = o + d * np.minimum(t, 10.0)[..., None]
        t = t * (1.0 - 0.05 * np.sin(3 * hit[..., 0]) * np.cos(2 * hit[..., 1]) / np.maximum(o[..., 2], 0.1))
    t = np.where(g.uniform(size=t.shape) < 0.03, 1e9, t)          # holes
    rig.put("depth", np.where(t < 1e8, t / inv_scale[None], 5.0 / inv_scale[None]).astype(F))
    return rig


def random_poses(make_rig, N=5, G=16, width=16, height=12, seed=0, tick=7, stream=None, **kw):
    """one FILL_ALL launch into an empty map under the comparison rule; the scan against the launch's own map.  Returns (read, the scene's ambiguous share)"""
    rig = random_rig(make_rig, N, G, width, height, seed, **kw)
    par, inp = ER.Params.of(rig), rig.inputs()
    assert rig.launch(tick, ER.FILL_ALL, stream=stream) == 0
    got = rig.read()
    amb = n = scanned = 0
    visited = range(0, N, par.env_stride)
    for e in visited:
        a_, n_ = ER.check_bracket(par, inp, e, got, tick)
        amb, n = amb + a_, n + n_
        scanned += check_scan(par, inp, e, got)
    assert scanned >= 0.95 * len(visited) * len(par.pts), "the scene's scan points: at most 5 % next to a cell edge (a condition on the scene)"
    worst = amb / max(n, 1)
    assert worst <= 0.01, f"{worst:.4f} of the scene's points are ambiguous: choose another seed"
    assert (got["stamp"][::par.env_stride] == tick).any(axis=(1, 2)).mean() > 0.5 or width * height < 8
    return got, worst


def check_scan(par, inp, e, got):
    """scan points at least EPS from a cell boundary: the value and `known` follow from the launch's own map arrays; returns how many were
    such points (a regular grid of points can put several of one env next to cell edges at once: the share is judged over the scene)"""
    G = par.G
    rs = inp["root_states"][e].astype(np.float64)
    E = ER.eps(rs[:3], inp["mount"][e][:3], par.t_hi)
    q = rs[3:7]
    qy = np.array([0.0, 0.0, q[2], q[3]]) / np.sqrt(q[2] ** 2 + q[3] ** 2)
    w = rs[:2] + ER.rot(qy, np.concatenate((par.pts, np.zeros((len(par.pts), 1))), axis=1))[:, :2]
    checked = 0
    for j in range(len(par.pts)):
        lo, hi = np.floor((w[j] - E) * par.rinv).astype(np.int64), np.floor((w[j] + E) * par.rinv).astype(np.int64)
        if (lo != hi).any():
            continue
        s = (lo[0] & (G - 1), lo[1] & (G - 1))
        knows = got["stamp"][e][s] >= 0 and got["cell"][e][s] == ER.pack(lo[0], lo[1])
        assert got["known"][e, j] == int(knows), (e, j)
        want = got["height"][e][s] if knows else F(F(rs[2]) - F(par.unknown_drop))
        assert ER.bits(np.array([got["scan"][e, j]], F))[0] == ER.bits(np.array([want], F))[0], (e, j)
        checked += 1
    return checked
