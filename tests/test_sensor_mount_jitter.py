"""CPU: the mount-jitter source (isaacgymloco_amd/csrc/ls_sensor_mount_jitter.h) compiled by g++ under LS_EMU, against the numpy reference of
tests/sensor_mount_jitter_reference.py (written from include/lsim.h; its docstring derives the bounds).  The same scenarios run on the HIP
launch in tests/test_gpu_sensor_mount_jitter.py."""
import math

import numpy as np
import pytest

import sensor_mount_jitter_emu_binding as MB
import sensor_mount_jitter_reference as MR
import sensor_mount_jitter_scenes as MS
from helpers import abi

SHAPES = [(N, stride) for N in (1, 255, 256, 257) for stride in (1, 3)]


@pytest.mark.parametrize("N,env_stride", SHAPES)
def test_fresh_rows_match_the_reference_and_the_others_are_untouched(N, env_stride):
    for stream_id, tick in ((0, 0), (3, MS.BIG_TICK)):
        MS.freshness(MB.Rig, N, env_stride, stream_id, tick)


@pytest.mark.parametrize("N,env_stride", SHAPES)
def test_the_draws_equal_the_reference_exactly(N, env_stride):
    for stream_id, tick in ((0, 0), (3, MS.BIG_TICK)):
        MS.draws_exact(MB.Rig, N, env_stride, stream_id, tick)


def test_the_big_tick_draws_what_its_low_word_draws():
    a = MS.draws_exact(MB.Rig, 257, 1, 3, MS.BIG_TICK)
    b = MS.draws_exact(MB.Rig, 257, 1, 3, 5)
    np.testing.assert_array_equal(MS.bits(a), MS.bits(b))


def test_zero_ranges_copy_the_nominal_pose_bit_for_bit():
    rig = MS.zero_ranges(MB.Rig, 257)
    # d = (0, 0, 0, 1) exactly: seen on the identity pose, where m_quat is d itself
    rig = MB.Rig(np.tile(MR.IDENTITY_ROW, (5, 1)), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    assert rig.launch(1, MR.FILL_ALL) == 0
    np.testing.assert_array_equal(MS.bits(rig.read()[0]), MS.bits(np.tile(MR.IDENTITY_ROW, (5, 1))))


def test_one_range_at_a_time_moves_one_axis():
    """pos_range[k] alone moves coordinate k alone; rot_range[k] alone turns about base axis k alone, by at most 2 atan(r / 2)"""
    N = 64
    nominal = np.tile(MR.IDENTITY_ROW, (N, 1))
    for k in range(3):
        r = [0.0, 0.0, 0.0]
        r[k] = 0.03
        rig = MB.Rig(nominal, r, (0.0, 0.0, 0.0), seed=3)
        assert rig.launch(2, MR.FILL_ALL) == 0
        m = rig.read()[0]
        others = [j for j in range(7) if j != k]
        np.testing.assert_array_equal(MS.bits(m[:, others]), MS.bits(nominal[:, others]))
        assert np.abs(m[:, k]).max() <= np.float32(0.03) and np.abs(m[:, k]).max() > 0.02 and m[:, k].min() < 0 < m[:, k].max()
        r[k] = math.radians(10.0)
        rig = MB.Rig(nominal, (0.0, 0.0, 0.0), r, seed=3)
        assert rig.launch(2, MR.FILL_ALL) == 0
        m = rig.read()[0]
        others = [j for j in range(6) if j != 3 + k]
        np.testing.assert_array_equal(MS.bits(m[:, others]), MS.bits(nominal[:, others]))
        ang = MR.angle(m[:, 3:])
        limit = 2.0 * math.atan(math.radians(10.0) / 2.0)
        assert ang.max() <= limit + 1e-6 and ang.max() > 0.9 * limit
        assert abs(limit / math.radians(10.0) - 1.0) < 0.0026          # the header's "0.25 % short at 10 degrees"


def test_a_launch_differs_with_tick_env_stream_seed_and_rank():
    MS.sensitivity(MB.Rig)


def test_the_draws_are_uniform_on_minus_one_to_one():
    MS.statistics(MB.Rig)


def _edits():
    nan, inf = math.nan, math.inf

    def s(name, value):
        return lambda mj: setattr(mj, name, value)

    def r(name, k, value):
        return lambda mj: getattr(mj, name).__setitem__(k, value)

    return {
        "nominal NULL": s("nominal", None), "mount NULL": s("mount", None), "episode_length NULL": s("episode_length", None),
        "nominal misaligned": lambda mj: setattr(mj, "nominal", mj.nominal + 2), "mount misaligned": lambda mj: setattr(mj, "mount", mj.mount + 1),
        "episode_length misaligned": lambda mj: setattr(mj, "episode_length", mj.episode_length + 4),
        "mount is nominal": lambda mj: setattr(mj, "mount", mj.nominal),
        "num_envs 0": s("num_envs", 0), "num_envs < 0": s("num_envs", -4), "env_stride 0": s("env_stride", 0), "env_stride < 0": s("env_stride", -1),
        "tick < 0": s("tick", -1), "stream_id 65536": s("stream_id", 65536),
        "pos_range < 0": r("pos_range", 1, -0.01), "pos_range nan": r("pos_range", 0, nan), "pos_range inf": r("pos_range", 2, inf),
        "rot_range < 0": r("rot_range", 2, -0.01), "rot_range nan": r("rot_range", 1, nan), "rot_range inf": r("rot_range", 0, inf),
        "unknown flag": s("flags", 4), "both flags": s("flags", MR.FILL_ALL | MR.RESETS_ONLY),
    }


def refusals(make_rig, null_call):
    """every refusal of the header, with `mount` and its guard untouched; the limits themselves are accepted"""
    nominal = MR.nominal_rows(9)

    def rv(edit, flags=0):
        rig = make_rig(nominal, MS.POS_RANGE, MS.ROT_RANGE)
        rig.put("episode_length", 0)
        r = rig.launch(3, flags, edit)
        m, guard = rig.read()
        assert (guard == MB.GUARD_VALUE).all()
        assert np.isnan(m).all() if r != 0 else np.isfinite(m).all()
        return r

    assert rv(None) == 0
    assert null_call() == abi.E_INVALID
    for what, edit in _edits().items():
        assert rv(edit) == abi.E_INVALID, what
    assert rv(lambda mj: setattr(mj, "stream_id", 65535)) == 0 and rv(None, MR.FILL_ALL) == 0 and rv(None, MR.RESETS_ONLY) == 0
    assert rv(lambda mj: setattr(mj, "tick", 2 ** 40)) == 0


def test_every_invalid_argument_is_refused_and_nothing_is_written():
    L = MB.lib()
    refusals(MB.Rig, lambda: L.emu_sensor_mount_jitter(None, None))


def test_the_library_refuses_the_same_arguments_before_any_launch():
    """through lib.load(): the argument check runs on the host before any HIP call, so host arrays serve and no device is needed"""
    from isaacgymloco_amd import lib
    L = lib.load()

    def host_rig(*a, **kw):
        rig = MB.Rig(*a, **kw)
        rig._entry = L.lsim_sensor_mount_jitter
        return rig

    nominal = MR.nominal_rows(9)
    assert L.lsim_sensor_mount_jitter(None, None) == abi.E_INVALID
    for what, edit in _edits().items():
        rig = host_rig(nominal, MS.POS_RANGE, MS.ROT_RANGE)
        rig.put("episode_length", 0)
        assert rig.launch(3, 0, edit) == abi.E_INVALID, what
        m, guard = rig.read()
        assert np.isnan(m).all() and (guard == MB.GUARD_VALUE).all(), what
