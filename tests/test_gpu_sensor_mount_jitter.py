"""GPU: the mount-jitter launch (lsim_sensor_mount_jitter, isaacgymloco_amd/csrc/ls_sensor_mount_jitter.h) on a real device: the scenarios
of tests/sensor_mount_jitter_scenes.py against the numpy reference (tests/sensor_mount_jitter_reference.py derives the bounds), against the
CPU build of the same source, on a side stream and after the ranges changed in place.  Every GPU step is one launch over at most 257 envs."""
import math

import numpy as np
import pytest

import sensor_mount_jitter_emu_binding as MB
import sensor_mount_jitter_reference as MR
import sensor_mount_jitter_scenes as MS

pytestmark = pytest.mark.gpu
CASES = [(1, 1, 0, 0), (1, 3, 3, MS.BIG_TICK), (257, 1, 3, MS.BIG_TICK), (257, 3, 0, 0)]


def hip_rig(*a, **kw):
    from isaacgymloco_amd import lib
    return MB.Rig(*a, device="cuda:0", entry=lib.load().lsim_sensor_mount_jitter, **kw)


def _against_the_cpu_build(hip, emu, N):
    """two fp32 evaluations, each within the reference's bound of the fp64 value: at most two bounds apart, the same rows written"""
    tol = MR.bound(MR.nominal_rows(N), MS.POS_RANGE, MS.ROT_RANGE)
    worst = 0.0
    for h, e in zip(hip, emu):
        np.testing.assert_array_equal(np.isnan(h), np.isnan(e))
        w = ~np.isnan(h)
        dist = np.abs(h.astype(np.float64) - e)
        assert (dist[w] <= 2.0 * tol[w]).all()
        worst = max(worst, float((dist[w] / tol[w]).max()), 0.0)
    return worst


@pytest.mark.parametrize("N,env_stride,stream_id,tick", CASES)
def test_the_cases_on_the_device_and_against_the_cpu_build(N, env_stride, stream_id, tick):
    hip = MS.freshness(hip_rig, N, env_stride, stream_id, tick)
    emu = MS.freshness(MB.Rig, N, env_stride, stream_id, tick)
    worst = _against_the_cpu_build(hip, emu, N)
    print(f"mount jitter N {N} stride {env_stride}: hip vs emu largest distance {worst:.3f} of the reference's bound")
    np.testing.assert_array_equal(MS.bits(MS.draws_exact(hip_rig, N, env_stride, stream_id, tick)),
                                  MS.bits(MS.draws_exact(MB.Rig, N, env_stride, stream_id, tick)))


def test_the_cases_on_a_side_stream():
    import torch
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for N, env_stride, stream_id, tick in CASES[1:3]:
            hip = MS.freshness(hip_rig, N, env_stride, stream_id, tick)
            _against_the_cpu_build(hip, MS.freshness(MB.Rig, N, env_stride, stream_id, tick), N)
            MS.draws_exact(hip_rig, N, env_stride, stream_id, tick)
    torch.cuda.synchronize()


def test_ranges_changed_in_place_and_zero_ranges():
    N = 257
    nominal = MR.nominal_rows(N)
    rig = hip_rig(nominal, MS.POS_RANGE, MS.ROT_RANGE, seed=MS.SEED, rank=MS.RANK, stream_id=2)
    before, _ = rig.read()
    everyone = np.ones(N, bool)
    assert rig.launch(9, MR.FILL_ALL) == 0
    first = MS.check(rig, nominal, before, everyone, 9, 2, "first ranges")
    rig.set_ranges((0.03, 0.0, 0.02), (math.radians(10.0), math.radians(2.0), 0.0))       # the same struct, the same buffers
    assert rig.launch(9, MR.FILL_ALL) == 0
    second = MS.check(rig, nominal, first, everyone, 9, 2, "second ranges")
    assert (MS.bits(second) != MS.bits(first)).any(axis=1).all()
    np.testing.assert_array_equal(MS.bits(second[:, 1]), MS.bits(nominal[:, 1]))           # pos_range[1] = 0
    rig.set_ranges((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    assert rig.launch(9, MR.FILL_ALL) == 0
    np.testing.assert_array_equal(MS.bits(rig.read()[0]), MS.bits(nominal))
    MS.zero_ranges(hip_rig, N)


def test_sensitivity_on_the_device_equals_the_cpu_builds_draws():
    hip, emu = MS.sensitivity(hip_rig), MS.sensitivity(MB.Rig)
    tol = MR.bound(np.tile(MR.nominal_rows(1), (257, 1)), MS.POS_RANGE, MS.ROT_RANGE)
    assert (np.abs(hip.astype(np.float64) - emu) <= 2.0 * tol).all()


def test_refusals_on_the_device_leave_the_mount_untouched():
    from isaacgymloco_amd import lib
    from test_sensor_mount_jitter import refusals
    L = lib.load()
    refusals(hip_rig, lambda: L.lsim_sensor_mount_jitter(None, None))
