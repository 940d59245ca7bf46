"""TEST INFRASTRUCTURE -- the scenes of the elevation map's visibility clean-up, shared by the CPU tests (the shim) and the GPU tests (the
library): each takes `make_rig` (elevation_cleanup_reference.cleanup_rig or its device form), plants a map, drives launches, checks every
one against elevation_cleanup_reference.check and returns what it read, so a GPU test can also compare with the CPU build's output.

Dyadic scenes: res = 2^-4, G = 16, the robot at the centre of a cell, the camera 1/4 m above it (identity quaternions unless said), ray
directions with dyadic components (not unit: the launch uses dirs as given, and "range" is the multiple of dirs), depths multiples of
2^-6.  Every ray runs through the middle of a row of cells and ends in the middle of a cell, and every height it is compared with lies
centimetres from the threshold, so every crossing and every comparison is far from a tie and the reference finds NO ambiguous slot: the
scenes assert that, and what must be forgotten is then exactly what is.  `mutant` runs the reference with one of its MUTANTS: the check must then fail (test_elevation_cleanup.py)."""
import numpy as np

import elevation_cleanup_reference as CR
import elevation_map_reference as ER
import elevation_map_scenes as EMS

F = np.float32
RES, Q = EMS.RES, EMS.Q
GAP = RES                        # one cell of a ray along x with dirs.x = 1
CAM = 0.25
DOWN = (1.0, 0.0, -1.0)          # reaches the floor 4 cells ahead (range 1/4)
FLAT = (1.0, 0.0, -0.25)         # reaches the floor 16 cells ahead (range 1): outside a G = 16 window
STEP = (1.0, 0.0, -0.5)
PTS = np.array([[0.0, 0.0], [0.25, 0.0]], F)


def start(make_rig, N, dirs, G=16, cell=(0, 0), yaw_pi=False, **kw):
    """a rig whose robots all stand at the centre of `cell` with the camera CAM above them, and the clean-up's fields of the dyadic scenes"""
    kw.setdefault("cleanup", dict(end_gap=GAP))
    rig = make_rig(N, G, np.asarray(dirs, F), PTS, res=RES, **kw)
    rs, mt = rig.get("root_states"), rig.get("mount")
    rs[:, 0], rs[:, 1] = (cell[0] + 0.5) * RES, (cell[1] + 0.5) * RES
    if yaw_pi:
        rs[:, 3:7] = EMS.YAW_PI
    mt[:, 2] = CAM
    rig.put("root_states", rs)
    rig.put("mount", mt)
    return rig


def plant(rig, e, cells=None, floor=0.0, stamp=3, var=None, known=True):
    """env e's map: every window cell known at height `floor` (known=False: never written), then `cells` {(dx, dy) relative to the robot's
    cell: height}; `var` {(dx, dy): variance}"""
    par = ER.Params.of(rig)
    G = rig.G
    rs = rig.get("root_states")[e]
    wix, wiy = CR.window_cells(par, rs)
    c = np.floor(rs[:2].astype(np.float64) * par.rinv).astype(np.int64)
    h, st, ce = rig.get("height"), rig.get("stamp"), rig.get("cell")
    h[e], st[e], ce[e] = floor, (stamp if known else -1), ER.pack(wix, wiy)
    for (dx, dy), z in (cells or {}).items():
        s = ((c[0] + dx) & (G - 1), (c[1] + dy) & (G - 1))
        h[e][s], st[e][s] = z, stamp
    rig.put("height", h), rig.put("stamp", st), rig.put("cell", ce)
    if var is not None:
        v = rig.get("var")
        v[e] = 0.0
        for (dx, dy), x in var.items():
            v[e][(c[0] + dx) & (G - 1), (c[1] + dy) & (G - 1)] = x
        rig.put("var", v)


def run(rig, tick, flags=0, mutant=None, exact=True, what=""):
    """one clean-up launch checked against the reference; returns (read, slots forgotten [N])"""
    par, cp, inp, before = ER.Params.of(rig), rig.params(), rig.inputs(), rig.read()
    assert rig.launch(tick, flags) == 0
    after = rig.read()
    amb, n, gone = CR.check(par, cp, inp, before, after, tick, flags, mutant)
    if exact:
        assert amb == 0, f"{what}: a dyadic scene has no ambiguous slot, the reference found {amb}"
    return after, gone


def forgotten(rig, after, e):
    """the cells of env e, relative to the robot's, whose slot reads -1"""
    par = ER.Params.of(rig)
    rs = rig.get("root_states")[e]
    wix, wiy = CR.window_cells(par, rs)
    c = np.floor(rs[:2].astype(np.float64) * par.rinv).astype(np.int64)
    gone = after["stamp"][e] == -1
    return sorted((int(x - c[0]), int(y - c[1])) for x, y in zip(wix[gone], wiy[gone]))


def planted_block(make_rig, mutant=None, reverse=False, G=16, cell=(0, 0)):
    """N = 3.  Env 0: cells 2 and 4 ahead stand 0.25 m above a flat floor and two rays reach the floor behind them at cell 4: cell 2 is
    crossed and forgotten (min_rays = 2, exactly two rays), cell 4 lies inside the end gap and stays.  Env 1: a real step from cell 2
    on, 0.125 m high, hit on its top at cell 4 by its own rays, which skim cells 2 and 3; cell 3 holds 29/128 m, which the rays
    undercut at the lower end of their passage only (hi is the higher end): nothing is forgotten.  Env 2: the block of
    env 0 crossed by ONE ray (min_rays - 1): it stays."""
    dirs = np.array([DOWN, STEP, DOWN, STEP, FLAT], F)
    order = slice(None, None, -1) if reverse else slice(None)
    rig = start(make_rig, 3, dirs[order], G=G, cell=cell)
    depth = np.full((3, 5), 1e9, F)
    depth[0, [0, 2]] = 0.25
    depth[1, [1, 3]] = 0.25
    depth[2, 0] = 0.25
    rig.put("depth", depth[:, order])
    plant(rig, 0, {(2, 0): 0.25, (4, 0): 0.25})
    plant(rig, 1, {**{(k, 0): 0.125 for k in range(2, G // 2)}, (3, 0): 29.0 / 128.0})
    plant(rig, 2, {(2, 0): 0.25, (4, 0): 0.25})
    after, gone = run(rig, 5, 0, mutant, what="planted block")
    assert forgotten(rig, after, 0) == [(2, 0)] and forgotten(rig, after, 1) == [] and forgotten(rig, after, 2) == []
    assert after["cleared"].tolist() == [CR.INITIAL["cleared"] + 1, CR.INITIAL["cleared"], CR.INITIAL["cleared"]]
    return after


def slope_term(make_rig, mutant=None, G=16):
    """a cell 6 ahead whose threshold the ray undercuts by less than clear_slope * rho: it stays, and goes without the slope term"""
    rig = start(make_rig, 1, np.array([FLAT, FLAT], F), cleanup=dict(end_gap=GAP, clear_slope=0.25), G=G)
    rig.put("depth", np.full((1, 2), 1.0, F))
    # at cell 6 the ray enters at x = 6 / 16, range 11 / 32: z = 0.25 - 11 / 128 = 0.1640625; rho at its exit 13 / 32: 0.25 * 13 / 32 = 0.1015625
    plant(rig, 0, {(6, 0): 0.25})           # thr = 0.2: 0.164 < 0.2 <= 0.266
    after, _ = run(rig, 5, 0, mutant, what="slope term")
    assert forgotten(rig, after, 0) == []
    return after


def older_window_and_unknown(make_rig, mutant=None, G=16):
    """the slot of the block holds a cell of an older window (its cell word is G cells off), and in env 1 was never written: both stay as
    they are"""
    rig = start(make_rig, 2, np.array([DOWN, DOWN], F), G=G)
    rig.put("depth", np.full((2, 2), 0.25, F))
    plant(rig, 0, {(2, 0): 0.25})
    plant(rig, 1, {(2, 0): 0.25})
    ce, st = rig.get("cell"), rig.get("stamp")
    ce[0][2, 0] = ER.pack(2 - G, 0)
    st[1][2, 0] = -1
    rig.put("cell", ce), rig.put("stamp", st)
    after, gone = run(rig, 5, 0, mutant, what="older window")
    assert gone.tolist() == [0, 0] and after["stamp"][0][2, 0] == 3
    return after


def negative_wrap(make_rig, mutant=None, G=16):
    """the robot in cell (-3, -2), looking along -x (yaw pi): the block's cell has negative coordinates and wraps to the far end of the slots"""
    rig = start(make_rig, 1, np.array([DOWN, DOWN], F), cell=(-3, -2), yaw_pi=True, G=G)
    rig.put("depth", np.full((1, 2), 0.25, F))
    plant(rig, 0, {(-2, 0): 0.25, (-4, 0): 0.25, (2, 0): 0.25})
    after, _ = run(rig, 5, 0, mutant, what="negative wrap")
    assert forgotten(rig, after, 0) == [(-2, 0)]
    assert after["stamp"][0][(-5) & (G - 1), (-2) & (G - 1)] == -1
    return after


def end_outside_window(make_rig, mutant=None, G=16):
    """two rays that reach the floor 16 cells ahead, outside a G = 16 window, still clear the block at cell 6 inside it"""
    rig = start(make_rig, 1, np.array([FLAT, FLAT], F), G=G)
    rig.put("depth", np.full((1, 2), 1.0, F))
    plant(rig, 0, {(6, 0): 0.25})
    after, _ = run(rig, 5, 0, mutant, what="end outside the window")
    assert forgotten(rig, after, 0) == [(6, 0)]
    return after


def variance_protects(make_rig, mutant=None, G=16):
    """env 0: the block's variance is 1/64 m^2, three standard deviations are 0.375 m: it stays.  Env 1: variance 0: forgotten"""
    rig = start(make_rig, 2, np.array([DOWN, DOWN], F), var=True, G=G)
    rig.put("depth", np.full((2, 2), 0.25, F))
    plant(rig, 0, {(2, 0): 0.25}, var={(2, 0): 2.0 ** -6})
    plant(rig, 1, {(2, 0): 0.25}, var={})
    after, _ = run(rig, 5, 0, mutant, what="variance")
    assert forgotten(rig, after, 0) == [] and forgotten(rig, after, 1) == [(2, 0)]
    return after


def due_sets(make_rig, flags=0, stagger=0, env_stride=1, N=7, mutant=None, G=16):
    """period 3 over six ticks, the block planted anew before every launch: exactly the envs that are due and not fresh forget it; at
    tick 4 two envs start an episode: their `cleared` is 0 and their map untouched.  Unvisited envs and every guard stay."""
    rig = start(make_rig, N, np.array([DOWN, DOWN], F), period=3, stagger=stagger, env_stride=env_stride, G=G)
    rig.put("depth", np.full((N, 2), 0.25, F))
    out = []
    for tick in range(1, 7):
        el = np.ones(N, np.int64)
        if tick == 4:
            el[[0, N - 1]] = 0
        rig.put("episode_length", el)
        for e in range(N):
            plant(rig, e, {(2, 0): 0.25})
        after, gone = run(rig, tick, flags, mutant, what=f"due sets, flags {flags}")
        visited, fill, due = ER.due_set(N, env_stride, flags, el, tick, 3, stagger)
        np.testing.assert_array_equal(gone == 1, due & ~fill)
        np.testing.assert_array_equal(gone == 0, ~(due & ~fill))
        assert (after["cleared"][fill] == 0).all()
        out.append(after)
    return out


def nonfinite_pose(make_rig, mutant=None, G=16):
    """a non-finite component of the pose or of the assumed mount: nothing of the env is written, nothing is counted"""
    rig = start(make_rig, 4, np.array([DOWN, DOWN], F), G=G)
    rig.put("depth", np.full((4, 2), 0.25, F))
    for e in range(4):
        plant(rig, e, {(2, 0): 0.25})
    rs, mt = rig.get("root_states"), rig.get("mount")
    rs[0, 1], rs[1, 6], mt[2, 4] = np.nan, np.inf, -np.inf
    rig.put("root_states", rs), rig.put("mount", mt)
    after, gone = run(rig, 5, 0, mutant, what="non-finite pose")
    assert gone.tolist() == [0, 0, 0, 1] and after["state"] == 0
    return after


def unused_rays(make_rig, mutant=None, G=16):
    """one env per way a ray is not used, two such rays each: the block stays; the last env's two rays are used and clear it"""
    ways = ("miss", "t <= t_lo", "t >= t_hi", "nan", "inf", "label 0", "label 2", "t <= end_gap", "used")
    N = len(ways)
    # the rays are DOWN at 0.25 unless said: d = stored
    rig = start(make_rig, N, np.array([DOWN, DOWN], F), labels=True, t_lo=Q, t_hi=0.5, G=G)
    stored = {"miss": 1e9, "t <= t_lo": Q, "t >= t_hi": 0.5, "nan": np.nan, "inf": np.inf, "t <= end_gap": GAP}
    rig.put("depth", np.array([[stored.get(w, 0.25)] * 2 for w in ways], F))
    lab = np.ones((N, 2), np.uint8)
    lab[ways.index("label 0")], lab[ways.index("label 2")] = 0, 2
    rig.put("labels", lab)
    for e in range(N):
        plant(rig, e, {(2, 0): 0.25, (0, 0): 0.5})         # the robot's own cell too: even the shortest used ray would pass below it
    after, gone = run(rig, 5, 0, mutant, what="unused rays")
    np.testing.assert_array_equal(gone > 0, np.array([w == "used" for w in ways]))
    return after


def vertical_ray(make_rig, mutant=None, G=16):
    """two rays straight down: neither axis steps, the walk visits the camera's own cell alone, with hi the camera's height.  Env 0: the
    floor stays.  Env 1: a phantom above the camera in that cell goes."""
    rig = start(make_rig, 2, np.array([[0, 0, -1], [0, 0, -1]], F), G=G)
    rig.put("depth", np.full((2, 2), 0.25, F))
    plant(rig, 0)
    plant(rig, 1, {(0, 0): 1.0, (1, 0): 1.0})
    after, _ = run(rig, 5, 0, mutant, what="vertical ray")
    assert forgotten(rig, after, 0) == [] and forgotten(rig, after, 1) == [(0, 0)]
    return after


EXACT = {"planted_block": planted_block, "slope_term": slope_term, "older_window_and_unknown": older_window_and_unknown,
         "negative_wrap": negative_wrap, "end_outside_window": end_outside_window, "variance_protects": variance_protects,
         "nonfinite_pose": nonfinite_pose, "unused_rays": unused_rays, "vertical_ray": vertical_ray}
CATCHES = {"hi_min": planted_block, "no_end_gap": planted_block, "min_rays_strict": planted_block, "no_slope": slope_term,
           "window_on_end": end_outside_window, "clean_fresh": due_sets}


# ---- general poses: the bracket of the reference's docstring
SHAPES = {(1, 64, 1): dict(width=1, height=1, min_rays=1), (3, 16, 193): dict(width=193, height=1), (3, 64, 513): dict(width=27, height=19),
          (257, 16, 193): dict(width=193, height=1, env_stride=3), (257, 64, 513): dict(width=27, height=19)}


def general(make_rig, N, G, R, seed=0, var=False, stream=None, reverse=False):
    """elevation_map_scenes.random_rig (res 1/8 m at G = 16, 1/16 m at G = 64): one capture inserted by the map's own
    launch, every other window cell given the synthetic ground's height at its centre, then a sixth of the cells lifted by 0.15, 0.3 or 0.5 m
    (phantoms); the second visited env of three or more starts an episode.  One clean-up launch under the bracket.  Returns (read,
    ambiguous share of the known slots, slots forgotten [N], the env that starts an episode or None)"""
    shape = SHAPES[N, G, R]
    kw = {k: v for k, v in shape.items() if k == "env_stride"}
    res = 0.125 if G == 16 else RES
    cleanup = dict(end_gap=1.5 * res, min_rays=shape.get("min_rays", 2))
    rig = EMS.random_rig(lambda *a, **k: make_rig(*a, cleanup=cleanup, var=var, **k), N, G, shape["width"], shape["height"], seed, res=res, **kw)
    assert rig.R == R
    if reverse:
        rig.put("dirs", rig.get("dirs")[::-1].copy())
        rig.put("inv_scale", rig.get("inv_scale")[::-1].copy())
        rig.put("depth", rig.get("depth")[:, :R][:, ::-1].copy())
    assert rig.map_launch(7, ER.FILL_ALL, stream=stream) == 0
    g = np.random.RandomState(seed + 100)
    par, got, rs = ER.Params.of(rig), rig.read(), rig.get("root_states")
    h, st, ce = got["height"], got["stamp"], got["cell"]
    for e in range(0, N, par.env_stride):
        wix, wiy = CR.window_cells(par, rs[e])
        ground = 0.05 * np.sin(3.0 * (wix + 0.5) * res) * np.cos(2.0 * (wiy + 0.5) * res)
        h[e] = np.where(st[e] >= 0, h[e], ground.astype(F))
        st[e], ce[e] = np.where(st[e] >= 0, st[e], 6), ER.pack(wix, wiy)
    lift = (st >= 0) & (g.uniform(size=h.shape) < 1.0 / 6.0)
    rig.put("height", np.where(lift, h + g.choice([0.15, 0.3, 0.5], size=h.shape).astype(F), h).astype(F)), rig.put("stamp", st), rig.put("cell", ce)
    if var:
        rig.put("var", g.choice([0.0, 1e-4, 2.5e-3], size=h.shape).astype(F))
    fresh = par.env_stride if N >= 3 else None
    if fresh is not None:
        el = rig.get("episode_length")
        el[fresh] = 0
        rig.put("episode_length", el)
    cp, inp, before = rig.params(), rig.inputs(), rig.read()
    assert rig.launch(8, 0, stream=stream) == 0
    after = rig.read()
    amb, n, gone = CR.check(par, cp, inp, before, after, 8, 0)
    share = amb / max(n, 1)
    print(f"clean-up (N, G, R) = {(N, G, R)}: {int(gone.sum())} of {n} known slots forgotten, {amb} ambiguous ({100.0 * share:.3f} %)")
    assert share <= 0.01, f"{share:.4f} of the known slots are ambiguous: choose another seed"
    return after, share, gone, fresh
