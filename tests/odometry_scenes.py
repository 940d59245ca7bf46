"""TEST INFRASTRUCTURE -- the scenarios of the odometry launch, run by tests/test_odometry.py on the CPU shim and by tests/test_gpu_odometry.py
on the HIP launch: each takes `make_rig`, a Rig factory of tests/odometry_emu_binding.py, drives launches and checks them against
tests/odometry_reference.py."""
import numpy as np

import odometry_reference as OR

SEED, RANK, STREAM = 7, 2, 3
BIG_TICK = 2 ** 32 + 5
# K R <= 1 with K = 40: the regime OR.bounds is derived for.  scale, yaw (rad/m), z (m/m), then the three per-step noises
RANGES = (0.006, 0.004, 0.006, 0.003, 0.002, 0.003)
L_MAX = 0.05
MUTANTS = ("true_yaw", "redraw_bias", "prev_fixed", "fresh_keeps", "whole_angle")
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def plus_zero(a):
    """-0 -> +0, every other value unchanged: what adding +0 does"""
    return (np.asarray(a, F) + F(0.0)).astype(F)


def quat(roll, pitch, yaw):
    """xyzw of Rz(yaw) Ry(pitch) Rx(roll), fp64"""
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    return np.stack((sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy), axis=-1)


def walk(N, K, seed=11, far_env=None, reset=None):
    """root_states [K + 1, N, 13] fp32 of a scripted walk: steps shorter than L_MAX, the heading turning, roll and pitch up to 0.4 rad, the
    velocities arbitrary.  `far_env`: that env starts at (-190, 37) m.  `reset` = (step, env): the env jumps to a new place at that step"""
    g = np.random.RandomState(seed)
    pos = np.concatenate((g.uniform(-8.0, 8.0, (N, 2)), g.uniform(0.3, 0.6, (N, 1))), axis=1)
    if far_env is not None:
        pos[far_env, :2] = (-190.0, 37.0)
    heading = g.uniform(-np.pi, np.pi, N)
    out = np.zeros((K + 1, N, 13), F)
    for t in range(K + 1):
        if t:
            heading = heading + g.uniform(-0.2, 0.2, N)
            length = g.uniform(0.01, 0.049, N)
            pos[:, 0] += length * np.cos(heading)
            pos[:, 1] += length * np.sin(heading)
            pos[:, 2] += g.uniform(-0.01, 0.01, N)
            if reset is not None and t == reset[0]:
                pos[reset[1]] = (3.0, -5.0, 0.42)
        out[t, :, 0:3] = pos
        out[t, :, 3:7] = quat(g.uniform(-0.4, 0.4, N), g.uniform(-0.4, 0.4, N), heading)
        out[t, :, 7:13] = g.uniform(-1.0, 1.0, (N, 6))
    d = np.diff(out[:, :, 0:2].astype(np.float64), axis=0)
    if reset is not None:
        d[reset[0] - 1, reset[1]] = 0.0
    assert np.hypot(d[..., 0], d[..., 1]).max() <= L_MAX
    return out


def start(make_rig, rs0, ranges=RANGES, tick=0, **kw):
    """a rig whose first launch (FILL_ALL, as an attach does) has run on rs0"""
    rig = make_rig(rs0.shape[0], ranges, **dict(dict(seed=SEED, rank=RANK, stream_id=STREAM), **kw))
    rig.put("root_states", rs0)
    assert rig.launch(tick, OR.FILL_ALL) == 0
    return rig


def zero_ranges(make_rig, N=3, K=10):
    """all-zero ranges: est[0:7] is root_states[0:7] bit for bit (up to -0 -> +0), the drift stays 0, prev follows the robot"""
    rs = walk(N, K, far_env=N - 1 if N >= 3 else None)
    rs[3 if K >= 3 else 0, 0, 3] = -0.0                      # a component -0 comes out as +0
    rig = start(make_rig, rs[0], ranges=(0.0,) * 6)
    for t in range(K + 1):
        if t:
            rig.put("root_states", rs[t])
            rig.put("episode_length", t)
            assert rig.launch(t) == 0
        odo, est = rig.read()
        np.testing.assert_array_equal(bits(est[:, 0:7]), bits(plus_zero(rs[t, :, 0:7])), err_msg=f"step {t}")
        np.testing.assert_array_equal(bits(est[:, 7:13]), bits(rs[t, :, 7:13]))
        np.testing.assert_array_equal(bits(odo[:, 0:4]), 0)
        assert (odo[:, 4:8] == 0).all()                       # a bias is s * 0: either zero
        np.testing.assert_array_equal(bits(odo[:, 8:10]), bits(rs[t, :, 0:2]))
        np.testing.assert_array_equal(bits(odo[:, 10:12]), 0)
    return rig


def _reference_chain(rs, el, ticks, flags, env_stride, ranges, T, mutant=None):
    """the reference run over the same launches: lists of (odo, est) per launch, in dtype T"""
    N = rs.shape[1]
    odo, est = np.zeros((N, 12), T), np.full((N, 13), float(F(777.0)), T)
    out = []
    for t, tick in enumerate(ticks):
        odo, est = OR.step(rs[t], odo, est, el[t], tick, flags[t], env_stride, SEED, RANK, STREAM, ranges, T=T, mutant=mutant)
        out.append((odo, est))
    return out


def general(make_rig, N=5, K=40, env_stride=1, tick0=0, stream=None):
    """K steps with all six ranges non-zero and one reset in the middle: odo and est within OR.bounds of the float64 reference at every
    launch, the reference's own fp32 twin below half of it, and each mutant outside it somewhere.  Returns the (odo, est) of every launch"""
    reset = (K // 2, env_stride if N > env_stride else 0)        # a visited env
    rs = walk(N, K, reset=reset)
    el = np.tile(np.arange(K + 1, dtype=np.int64)[:, None], (1, N))
    el[reset[0]:, reset[1]] -= reset[0]                  # the reset env starts an episode at that step
    el[0] = 1                                            # the first launch is FILL_ALL: the lengths play no part
    ticks = [tick0 + t for t in range(K + 1)]
    flags = [OR.FILL_ALL] + [0] * K
    rig = make_rig(N, RANGES, env_stride=env_stride, seed=SEED, rank=RANK, stream_id=STREAM)
    got = []
    for t in range(K + 1):
        rig.put("root_states", rs[t])
        rig.put("episode_length", el[t])
        assert rig.launch(ticks[t], flags[t], stream=stream) == 0
        got.append(rig.read())
    want = _reference_chain(rs, el, ticks, flags, env_stride, RANGES, np.float64)
    twin = _reference_chain(rs, el, ticks, flags, env_stride, RANGES, np.float32)
    vis = OR.visited_set(N, env_stride)
    worst = twin_worst = 0.0
    for t in range(K + 1):
        otol, etol = OR.bounds(max(t, 1), L_MAX, RANGES, rs[t])
        for g, w, tw, tol, name in ((got[t][0], want[t][0], twin[t][0], otol, "odo"), (got[t][1], want[t][1], twin[t][1], etol, "est")):
            exact = tol[vis] == 0.0
            np.testing.assert_array_equal(g[vis][exact].astype(np.float64), w[vis][exact], err_msg=f"{name} step {t}")
            np.testing.assert_array_equal(bits(g[~vis]), bits(np.asarray(w[~vis], F)), err_msg=f"{name} step {t}: a row that is not visited")
            err, terr = np.abs(g[vis].astype(np.float64) - w[vis])[~exact], np.abs(tw[vis].astype(np.float64) - w[vis])[~exact]
            assert (terr < 0.5 * tol[vis][~exact]).all(), f"{name} step {t}: the reference's fp32 twin uses {float((terr / tol[vis][~exact]).max()):.2f} of the bound"
            assert (err <= tol[vis][~exact]).all(), f"{name} step {t}: worst error / bound {float((err / tol[vis][~exact]).max()):.2f}"
            worst, twin_worst = max(worst, float((err / tol[vis][~exact]).max())), max(twin_worst, float((terr / tol[vis][~exact]).max()))
    print(f"odometry N {N} K {K} stride {env_stride}: worst error {worst:.3f} of the bound, the reference's fp32 twin {twin_worst:.3f}")
    for m in MUTANTS:
        bad = _reference_chain(rs, el, ticks, flags, env_stride, RANGES, np.float64, mutant=m)
        caught = False
        for t in range(K + 1):
            otol, etol = OR.bounds(max(t, 1), L_MAX, RANGES, rs[t])
            caught = caught or bool((np.abs(got[t][0].astype(np.float64) - bad[t][0])[vis] > otol[vis]).any()) \
                or bool((np.abs(got[t][1].astype(np.float64) - bad[t][1])[vis] > etol[vis]).any())
        assert caught, f"the mutant {m} passes the scene"
    return got


def same_tick_again(make_rig, N=3):
    """a second launch on the same tick with unmoved robots changes neither odo nor est -- for a fresh env (same draws) and the others"""
    rs = walk(N, 3)
    rig = start(make_rig, rs[0])
    for t in (1, 2, 3):
        rig.put("root_states", rs[t])
        rig.put("episode_length", np.where(np.arange(N) == 1, 0, t) if t == 3 else t)
        assert rig.launch(t) == 0
    odo, est = rig.read()
    assert (odo[np.arange(N) != 1, 0:4] != 0).all() and (odo[1, 0:4] == 0).all()
    assert rig.launch(3) == 0
    odo2, est2 = rig.read()
    np.testing.assert_array_equal(bits(odo2), bits(odo))
    np.testing.assert_array_equal(bits(est2), bits(est))
    return odo, est


def fresh_env(make_rig, N=3, tick=BIG_TICK):
    """an env that starts an episode: zero drift, prev = p.xy, est[0:7] = its pose, the biases the exact fp32 products of the header's draws;
    RESETS_ONLY equals flags 0; FILL_ALL makes every visited env fresh"""
    rs = walk(N, 2)
    out = []
    for flags in (0, OR.RESETS_ONLY, OR.FILL_ALL):
        rig = start(make_rig, rs[0], tick=tick)
        rig.put("root_states", rs[1])
        assert rig.launch(tick + 1) == 0
        rig.put("root_states", rs[2])
        el = np.where(np.arange(N) == N - 1, 0, 2).astype(np.int64)
        rig.put("episode_length", el)
        assert rig.launch(tick + 2, flags) == 0
        odo, est = rig.read()
        fresh = OR.fresh_set(N, 1, flags, el)
        assert fresh.sum() == (N if flags == OR.FILL_ALL else 1)
        s = OR.draws(SEED, RANK, np.nonzero(fresh)[0], tick + 2, STREAM, 1)
        np.testing.assert_array_equal(bits(odo[fresh, 0:4]), 0)
        np.testing.assert_array_equal(bits(odo[fresh, 4:7]), bits(s * np.array(rig.ranges[:3], F)[None, :]))
        np.testing.assert_array_equal(bits(odo[fresh, 8:10]), bits(rs[2, fresh, 0:2]))
        np.testing.assert_array_equal(bits(est[fresh, 0:7]), bits(plus_zero(rs[2, fresh, 0:7])))
        assert (odo[~fresh, 0:4] != 0).all()
        out.append((odo, est))
    np.testing.assert_array_equal(bits(out[0][0]), bits(out[1][0]))
    np.testing.assert_array_equal(bits(out[0][1]), bits(out[1][1]))
    return out


def strided(make_rig, N=7, env_stride=3):
    """env_stride 3: the rows of the envs in between keep every bit, in odo and in est (the guards are checked by every read)"""
    rs = walk(N, 2)
    rig = make_rig(N, RANGES, env_stride=env_stride, seed=SEED, rank=RANK, stream_id=STREAM)
    rig.fill("odo", F(-55.25))
    rig.put("root_states", rs[0])
    assert rig.launch(0, OR.FILL_ALL) == 0
    rig.put("root_states", rs[1])
    assert rig.launch(1) == 0
    odo, est = rig.read()
    vis = OR.visited_set(N, env_stride)
    assert vis.sum() == (N + env_stride - 1) // env_stride
    assert (odo[~vis] == F(-55.25)).all() and (est[~vis] == F(777.0)).all()
    assert (odo[vis, 0:4] != 0).all() and (est[vis] != F(777.0)).all()
    return odo, est


def nan_pose(make_rig, N=3):
    """a non-finite pose: the row is copied to est, the drift is cleared, the biases are kept and prev is NaN; the step after integrates
    D = 0 (the drift still 0, prev the new place) and the one after that drifts again"""
    rs = walk(N, 4)
    bad = rs[2].copy()
    bad[1, 4] = np.nan
    bad[2, 0] = np.inf
    rig = start(make_rig, rs[0])
    rig.put("root_states", rs[1])
    assert rig.launch(1) == 0
    before, _ = rig.read()
    rig.put("root_states", bad)
    assert rig.launch(2) == 0
    odo, est = rig.read()
    np.testing.assert_array_equal(bits(est[1:3]), bits(bad[1:3]))
    np.testing.assert_array_equal(bits(odo[1:3, 0:4]), 0)
    np.testing.assert_array_equal(bits(odo[1:3, 4:8]), bits(before[1:3, 4:8]))
    np.testing.assert_array_equal(bits(odo[1:3, 8:10]), 0x7FC00000)
    assert (odo[0, 0:4] != 0).all() and np.isfinite(est[0]).all()
    rig.put("root_states", rs[3])
    assert rig.launch(3) == 0
    odo3, est3 = rig.read()
    np.testing.assert_array_equal(bits(odo3[1:3, 0:4]), 0)
    np.testing.assert_array_equal(bits(odo3[1:3, 8:10]), bits(rs[3, 1:3, 0:2]))
    np.testing.assert_array_equal(bits(est3[1:3, 0:7]), bits(plus_zero(rs[3, 1:3, 0:7])))
    rig.put("root_states", rs[4])
    assert rig.launch(4) == 0
    odo4, est4 = rig.read()
    assert (odo4[:, 0:4] != 0).all() and np.isfinite(est4).all() and np.isfinite(odo4).all()
    return odo, est, odo3, est3, odo4, est4


def refusals(make_rig, null_call, launches=True):
    """every LSIM_E_INVALID of the header, and nothing written by any of them.  `launches` False: only the refused calls are made (the
    library's entry on host arrays: its host-side check runs, no valid struct is ever handed to it)"""
    from helpers import abi
    rig = make_rig(3, RANGES)
    before = [bits(a) for a in rig.read()]
    E = abi.E_INVALID
    assert null_call() == E

    def field(name, value):
        def edit(od):
            setattr(od, name, value)
        return edit

    def shifted(name, by):
        def edit(od):
            setattr(od, name, getattr(od, name) + by)
        return edit

    edits = [field("root_states", None), field("est", None), field("odo", None), field("episode_length", None),
             shifted("root_states", 2), shifted("est", 2), shifted("odo", 4), shifted("odo", 8), shifted("episode_length", 4),
             lambda od: setattr(od, "est", od.root_states), field("num_envs", 0), field("env_stride", 0), field("stream_id", 65536)]
    for name in OR.RANGE_NAMES:
        edits += [field(name, -1e-6), field(name, float("nan")), field(name, float("inf"))]
    for e in edits:
        assert rig.launch(1, edit=e) == E
    assert rig.launch(-1) == E
    assert rig.launch(1, 4) == E and rig.launch(1, OR.FILL_ALL | OR.RESETS_ONLY) == E
    for a, b in zip(before, rig.read()):
        np.testing.assert_array_equal(a, bits(b))
    if launches:
        assert rig.launch(1, OR.RESETS_ONLY) == 0 and rig.launch(1, edit=field("stream_id", 65535)) == 0
