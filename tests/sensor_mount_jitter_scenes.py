"""TEST INFRASTRUCTURE -- the scenarios of the mount-jitter launch, run by tests/test_sensor_mount_jitter.py on the CPU shim and by
tests/test_gpu_sensor_mount_jitter.py on the HIP launch: each takes `make_rig`, a Rig factory of tests/sensor_mount_jitter_emu_binding.py."""
import math

import numpy as np

import sensor_mount_jitter_emu_binding as MB
import sensor_mount_jitter_reference as MR

POS_RANGE = (0.01, 0.02, 0.005)
ROT_RANGE = tuple(math.radians(d) for d in (1.0, 5.0, 2.0))
SEED, RANK = 7, 2
BIG_TICK = 2 ** 32 + 5


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def episode_lengths(N):
    """mixed: envs 0, 1 of every four start an episode"""
    e = np.arange(N)
    return np.where(e % 4 < 2, 0, e + 1).astype(np.int64)


def check(rig, nominal, before, fresh, tick, stream_id, what):
    """the launch just made wrote exactly the rows of `fresh`, each within the reference's bound, and the mutants do not pass for it"""
    got, guard = rig.read()
    assert (guard == MB.GUARD_VALUE).all(), what
    np.testing.assert_array_equal(bits(got[~fresh]), bits(before[~fresh]), err_msg=what)
    if not fresh.any():
        return got
    assert np.isfinite(got[fresh]).all(), what
    want, tol = MR.expected(nominal, before, fresh, SEED, RANK, tick, stream_id, rig.pos_range, rig.rot_range)
    err = np.abs(got.astype(np.float64)[fresh] - want[fresh])
    assert (err <= tol[fresh]).all(), f"{what}: worst error / bound {float((err / tol[fresh]).max()):.2f}"
    # pos_range per axis and the largest angle of d = m_quat (x) n_quat^-1
    slack = tol[fresh]
    assert (np.abs(got[fresh, :3].astype(np.float64) - nominal[fresh, :3]) <= rig.pos_range.astype(np.float64) + slack[:, :3]).all(), what
    n = nominal[fresh, 3:].astype(np.float64)
    d = MR.qmul(got[fresh, 3:].astype(np.float64), n * np.array([-1.0, -1.0, -1.0, 1.0]))      # unit nominals: the conjugate is the inverse
    limit = 2.0 * math.atan(np.linalg.norm(rig.rot_range.astype(np.float64)) / 2.0)
    assert (MR.angle(d) <= limit + 4.0 * slack[:, 3:].max()).all(), what
    if np.any(rig.rot_range > 0):
        # n (x) d differs from d (x) n in the vector part only (the scalar part of a product commutes, and the position has no part in it)
        m1, _ = MR.expected(nominal, before, fresh, SEED, RANK, tick, stream_id, rig.pos_range, rig.rot_range, swap_product=True)
        missed = np.abs(got.astype(np.float64) - m1)[fresh, 3:6] > tol[fresh, 3:6]
        assert missed.mean() > 0.9, f"{what}: the mutant n (x) d passes on {1.0 - missed.mean():.2f} of the quaternion's vector outputs"
    if np.any(rig.rot_range > 0) and np.any(rig.pos_range > 0):
        # every draw changes; a coordinate whose range is 0 has no draw in it, and cannot tell
        m2, _ = MR.expected(nominal, before, fresh, SEED, RANK, tick, stream_id, rig.pos_range, rig.rot_range, swap_blocks=True)
        cols = np.concatenate((rig.pos_range > 0, np.ones(4, bool)))
        missed = (np.abs(got.astype(np.float64) - m2)[fresh] > tol[fresh])[:, cols]
        assert missed.mean() > 0.9, f"{what}: the mutant with the Philox blocks swapped passes on {1.0 - missed.mean():.2f} of the outputs"
    return got


def freshness(make_rig, N, env_stride, stream_id, tick):
    """mixed episode lengths under flags 0 and RESETS_ONLY, a second launch on the same tick, FILL_ALL; returns the mounts of the launches"""
    nominal = MR.nominal_rows(N)
    rig = make_rig(nominal, POS_RANGE, ROT_RANGE, env_stride=env_stride, seed=SEED, rank=RANK, stream_id=stream_id)
    el = episode_lengths(N)
    rig.put("episode_length", el)
    what = f"N {N} stride {env_stride} stream {stream_id} tick {tick}"
    before, _ = rig.read()
    assert rig.launch(tick) == 0
    fresh = MR.fresh_set(N, env_stride, 0, el)
    first = check(rig, nominal, before, fresh, tick, stream_id, what + " flags 0")
    assert rig.launch(tick) == 0                 # again on the same tick: the same bits
    np.testing.assert_array_equal(bits(rig.read()[0]), bits(first))
    rig.fill_mount(np.nan)
    assert rig.launch(tick, MR.RESETS_ONLY) == 0
    np.testing.assert_array_equal(bits(rig.read()[0]), bits(first), err_msg=what + " RESETS_ONLY equals flags 0")
    rig.fill_mount(np.nan)
    before, _ = rig.read()
    assert rig.launch(tick, MR.FILL_ALL) == 0
    everyone = MR.fresh_set(N, env_stride, MR.FILL_ALL, el)
    assert everyone.sum() == (N + env_stride - 1) // env_stride
    full = check(rig, nominal, before, everyone, tick, stream_id, what + " FILL_ALL")
    np.testing.assert_array_equal(bits(full[fresh]), bits(first[fresh]))
    rig.put("episode_length", 3)                 # nobody fresh: nothing written
    rig.fill_mount(np.nan)
    assert rig.launch(tick) == 0
    assert np.isnan(rig.read()[0]).all()
    return first, full


def draws_exact(make_rig, N, env_stride, stream_id, tick):
    """the launch's own six draws (identity nominal, unit ranges: MR.draws_of) equal the reference's, exactly"""
    rig = make_rig(np.tile(MR.IDENTITY_ROW, (N, 1)), (1.0, 1.0, 1.0), (1.0, 1.0, 1.0), env_stride=env_stride, seed=SEED, rank=RANK, stream_id=stream_id)
    assert rig.launch(tick, MR.FILL_ALL) == 0
    got, _ = rig.read()
    envs = np.arange(0, N, env_stride)
    assert np.isnan(got[np.setdiff1d(np.arange(N), envs)]).all()
    s = MR.draws_of(got[envs])
    np.testing.assert_array_equal(bits(s), bits(MR.draws(SEED, RANK, envs, tick, stream_id)))
    return s


def zero_ranges(make_rig, N):
    nominal = MR.nominal_rows(N)
    rig = make_rig(nominal, seed=SEED, rank=RANK)
    assert rig.launch(3, MR.FILL_ALL) == 0
    np.testing.assert_array_equal(bits(rig.read()[0]), bits(nominal))
    return rig


def sensitivity(make_rig, N=257):
    """the same nominal row for every env: rows differ from env to env, and a launch differs when tick, stream_id, seed or rank does"""
    nominal = np.tile(MR.nominal_rows(1), (N, 1))

    def run(tick=4, **kw):
        rig = make_rig(nominal, POS_RANGE, ROT_RANGE, **dict(dict(seed=SEED, rank=RANK, stream_id=1), **kw))
        assert rig.launch(tick, MR.FILL_ALL) == 0
        return rig.read()[0]
    base = run()
    assert len({row.tobytes() for row in base}) == N, "two envs drew the same pose"
    np.testing.assert_array_equal(bits(run()), bits(base))
    np.testing.assert_array_equal(bits(run(tick=4 + 2 ** 32)), bits(base))       # the step word is the low 32 bits of the tick
    for what, other in (("tick", run(tick=5)), ("stream_id", run(stream_id=2)), ("seed", run(seed=SEED + 1)), ("rank", run(rank=RANK + 1))):
        assert (bits(other) != bits(base)).any(axis=1).mean() > 0.99, what
        assert (bits(other) != bits(base)).mean() > 0.9, what
    return base


def statistics(make_rig, N=4096, ticks=4):
    """mean and variance of each of the launch's six draws: within five standard errors of 0 and 1/3.  A uniform on [-1, 1) has variance 1/3
    and fourth moment 1/5, so the sample variance has standard error sqrt((1/5 - 1/9) / n)"""
    s = np.concatenate([draws_exact(make_rig, N, 1, 0, t) for t in range(ticks)]).astype(np.float64)
    n = s.shape[0]
    se_mean, se_var = math.sqrt(1.0 / 3.0 / n), math.sqrt((1.0 / 5.0 - 1.0 / 9.0) / n)
    for k in range(6):
        mean, var = float(s[:, k].mean()), float(s[:, k].var())
        print(f"mount jitter: s_{k} over {n} draws: mean {mean:+.5f} (bound {5 * se_mean:.5f}), variance {var:.5f} (1/3 +- {5 * se_var:.5f})")
        assert abs(mean) <= 5.0 * se_mean and abs(var - 1.0 / 3.0) <= 5.0 * se_var, k
    assert s.min() >= -1.0 and s.max() < 1.0
