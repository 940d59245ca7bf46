"""TEST INFRASTRUCTURE -- the inputs and the three scenarios shared by tests/test_sensor_model.py (CPU shim) and tests/test_gpu_sensor_model.py
(HIP launch): each scenario drives a sensor_model_emu_binding.Rig made by `make_rig(**keywords)` and asserts against
tests/sensor_model_reference.py; it returns what it recorded so that two builds can be compared with each other.

Shapes, the smallest that can still go wrong: N = 7 envs (more than the period 3 and no multiple of it), R = 260 rays (two blocks of 256 lanes
per env, the second with 4 live lanes), hist_stride = 264, the plane z = 0.  Even rays look down (elevation -0.35 .. -1.25 rad: with a base
0.4 .. 0.7 m up and pitched by at most 0.05 rad they hit at 0.4 .. 2.4 m), odd rays look up by the same angles and miss.  Base height and pitch
change with every launch, so every capture of an env differs from the one before."""
import math

import numpy as np

import raycast_reference as REF
import sensor_model_reference as SR

N, R, HIST_STRIDE = 7, 260, 264
NEAR, FAR = 0.05, 5.0
PLANE = REF.plane_scene()
MODEL3 = dict(sigma0=0.02, sigma2=0.01, p_drop=0.1, drop_value=0.0, clip_lo=0.1, clip_hi=3.0, offset=(0.1 + 3.0) / 2.0, gain=1.0 / (3.0 - 0.1),
              seed=7, rank=2, stream_id=3)


def dirs():
    r = np.arange(R)
    el = (0.35 + 0.9 * (r // 2) / (R // 2 - 1)) * np.where(r % 2 == 0, -1.0, 1.0)
    az = 2.0 * math.pi * r / R * 3.0
    return np.stack((np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)), axis=-1).astype(np.float32)


def scale():
    return (1.0 - 0.3 * np.arange(R) / R).astype(np.float32)


def mount():
    return np.tile(np.array([0, 0, 0, 0, 0, 0, 1], np.float32), (N, 1))


def pose(step):
    """root_states [N, 13] of launch number `step`"""
    rs = np.zeros((N, 13), np.float32)
    for e in range(N):
        h = 0.05 * math.sin(1.0 + step + 0.7 * e) / 2.0
        rs[e, :7] = [0.5 * e, -0.3 * e, 0.4 + 0.02 * e + 0.03 * (step % 7), 0.0, math.sin(h), 0.0, math.cos(h)]
    return rs


def plane_rig(make_rig, **kw):
    kw.setdefault("hist_stride", HIST_STRIDE)
    return make_rig(PLANE, pose(0), mount(), dirs(), NEAR, FAR, scale=scale(), **kw)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _prefill(rig):
    rig.put("out", np.nan)
    rig.put("labels", 255)


def identity(make_rig, plain_cast):
    """period 1, no latency, one frame, no noise, clip (0, far): out and hist[:, 0] are lsim_raycast's output bit for bit"""
    rig = plane_rig(make_rig)
    assert rig.launch(0) == 0
    out, lab, hist, state = rig.read()
    want, _ = plain_cast(PLANE, pose(0), mount(), dirs(), NEAR, FAR, scale=scale())
    np.testing.assert_array_equal(bits(out), bits(want))
    np.testing.assert_array_equal(bits(hist[:, 0]), bits(want))
    hit = np.broadcast_to(np.arange(R) % 2 == 0, (N, R))
    np.testing.assert_array_equal(lab, hit.astype(np.uint8))          # terrain-only labels: 1 for t < far
    assert state[0] == 0 and (want[hit] < 2.5).all() and (want[~hit] == np.float32(FAR) * np.broadcast_to(scale(), (N, R))[~hit]).all()
    return out, hist


def schedule(make_rig, plain_cast, env_stride=1):
    """period 3 staggered, latency 1, frames 2: FILL_ALL, ticks 0..9 with resets at ticks 4 and 5, RESETS_ONLY after tick 6.  Returns the
    list of (due, hist) after every launch"""
    p = dict(period=3, stagger=1, latency=1, frames=2)
    rig = plane_rig(make_rig, env_stride=env_stride, **p)
    K = 3
    ref_hist = np.full((N, K, R), -7.0, np.float32)
    recorded = []
    step = [0]

    def launch(tick, flags, zero_envs):
        nonlocal ref_hist
        rs = pose(step[0])
        step[0] += 1
        rig.put("root_states", rs)
        el = np.full(N, 5, np.int64)
        el[list(zero_envs)] = 0
        rig.put("episode_length", el)
        _prefill(rig)
        before = rig.read()[2]
        assert rig.launch(tick, flags) == 0
        out, lab, hist, state = rig.read()
        due, fill = SR.due_sets(N, env_stride, tick, p["period"], p["stagger"], flags, el)
        # rows of envs that are not due: untouched bit for bit, the NaN / 255 pre-fill included
        assert np.isnan(out[~due]).all() and (lab[~due] == 255).all()
        np.testing.assert_array_equal(bits(hist[~due]), bits(before[~due]))
        # rows of due envs: the clean frame of this pose
        want, _ = plain_cast(PLANE, rs, mount(), dirs(), NEAR, FAR, scale=scale())
        np.testing.assert_array_equal(bits(out[due]), bits(want[due]))
        y, _ = SR.model(out[due], lab[due] != 0, np.nonzero(due)[0], tick, rig.p)
        full = np.zeros((N, R), np.float32)
        full[due] = y
        ref_hist = SR.advance(ref_hist, full, due, fill)
        np.testing.assert_array_equal(bits(hist), bits(ref_hist))
        assert state[0] == 0
        recorded.append((due.copy(), hist.copy()))
        return due, fill, hist

    visited = np.arange(N) % env_stride == 0
    due, fill, hist = launch(0, SR.FILL_ALL, ())
    assert (due == visited).all() and (fill == visited).all()
    for k in range(1, K):
        np.testing.assert_array_equal(bits(hist[visited, k]), bits(hist[visited, 0]))      # all K slots
    assert (hist[~visited] == -7.0).all()
    seen = np.zeros(N, int)
    for tick in range(10):
        zero = {4: (2, 5), 5: (2,)}.get(tick, ())
        due, fill, _ = launch(tick, 0, zero)
        want_due = visited & (((tick + np.arange(N)) % 3 == 0) | np.isin(np.arange(N), zero))
        assert (due == want_due).all() and (fill == (visited & np.isin(np.arange(N), zero))).all()
        seen += due
        if tick == 6:
            due, fill, _ = launch(6, SR.RESETS_ONLY, (1, 4))
            assert (due == (visited & np.isin(np.arange(N), (1, 4)))).all() and (fill == due).all()
    assert (seen[visited] >= 3).all(), "every visited env captured several times: the shifts ran"
    return recorded


def model(make_rig):
    """the full model on period 1 / one frame, 64 ticks: every launch against the reference, then the statistics of the kernel's own draws.
    Returns the list of y [N, R] per tick"""
    rig = plane_rig(make_rig, **MODEL3)
    p = rig.p
    tol = SR.atol(p, FAR)
    hit = np.broadcast_to(np.arange(R) % 2 == 0, (N, R))
    y_lo = (np.float32(p["clip_lo"]) - np.float32(p["offset"])) * np.float32(p["gain"])          # what a dropped pixel reads: clip(0)
    ys, gs, drops = [], [], []
    worst = 0.0
    for tick in range(64):
        rig.put("root_states", pose(tick))
        assert rig.launch(tick) == 0
        out, lab, hist, state = rig.read()
        assert state[0] == 0
        np.testing.assert_array_equal(lab != 0, hit)
        y = hist[:, 0]
        want, dropped = SR.model(out, lab != 0, np.arange(N), tick, p)
        worst = max(worst, float(np.abs(y - want).max()))
        assert np.abs(y - want).max() <= tol, (tick, float(np.abs(y - want).max()), tol)
        np.testing.assert_array_equal(hit & (y == y_lo), dropped)                            # dropped pixels: exactly the reference's
        np.testing.assert_array_equal(bits(y[~hit]), bits(want[~hit]))                       # a miss carries no noise: clip and normalise only
        keep = hit & ~dropped
        v = y[keep].astype(np.float64) / p["gain"] + p["offset"]
        assert (v > p["clip_lo"] + 0.05).all() and (v < p["clip_hi"] - 0.05).all(), "no hit of this geometry reaches the clip bounds"
        raw = out[keep].astype(np.float64)
        gs.append((v - raw) / (p["sigma0"] + p["sigma2"] * raw * raw))
        drops.append(dropped[hit])
        ys.append(y.copy())
    print(f"sensor model: max |y - reference| {worst:.3e} (bound {tol:.3e})")
    # the same (seed, rank, tick) twice: identical; another stream_id: other draws, still the reference's
    rig.put("root_states", pose(5))
    assert rig.launch(5) == 0
    again = rig.read()[2][:, 0]
    np.testing.assert_array_equal(bits(again), bits(ys[5]))
    assert rig.launch(5, edit=lambda sm: setattr(sm, "stream_id", 4)) == 0
    out, lab, hist, _ = rig.read()
    other = hist[:, 0]
    assert (other[hit] != ys[5][hit]).mean() > 0.9
    want, _ = SR.model(out, lab != 0, np.arange(N), 5, dict(p, stream_id=4))
    assert np.abs(other - want).max() <= tol
    # statistics of what the kernel drew
    g, d = np.concatenate(gs), np.concatenate(drops)
    n, nh = g.size, d.size
    print(f"sensor model: {n} noise draws: mean {g.mean():+.4f} (bound {5 / math.sqrt(n):.4f}), variance {g.var():.4f}, |g| max {np.abs(g).max():.3f}; "
          f"dropped {d.mean():.4f} of {nh} hits (bound {5 * math.sqrt(0.09 / nh):.4f} around 0.1)")
    assert abs(g.mean()) <= 5.0 / math.sqrt(n)
    assert abs(g.var() - 1.0) <= 0.05
    assert np.abs(g).max() <= 3.0 + 1e-3
    assert abs(d.mean() - 0.1) <= 5.0 * math.sqrt(0.09 / nh)
    return ys
