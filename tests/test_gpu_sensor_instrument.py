"""GPU: the two instrument launches (lsim_sensor_instrument, lsim_sensor_capture_inst; isaacgymloco_amd/csrc/ls_sensor_instrument.h) on a real
device: the scenarios of tests/sensor_instrument_scenes.py against the numpy reference (tests/sensor_instrument_reference.py derives the
bounds), against the CPU build of the same source, on a side stream and after the ranges changed in place.  Every GPU step is one launch over
at most 257 envs (4096 for the statistics of the draws) or 7 envs x 260 rays."""
import numpy as np
import pytest

import sensor_instrument_emu_binding as IB
import sensor_instrument_reference as IR
import sensor_instrument_scenes as IS
import sensor_model_scenes as SC

pytestmark = pytest.mark.gpu
CASES = [(1, 1, 0, 0), (1, 3, 3, IS.BIG_TICK), (257, 1, 3, IS.BIG_TICK), (257, 3, 0, 0)]


def hip_draw(*a, **kw):
    from isaacgymloco_amd import lib
    return IB.DrawRig(*a, device="cuda:0", entry=lib.load().lsim_sensor_instrument, **kw)


def hip_rig(*a, **kw):
    from isaacgymloco_amd import lib
    return IB.CaptureRig(*a, device="cuda:0", entry=lib.load(), **kw)


def _against_the_cpu_build(hip, emu):
    """two fp32 evaluations, each within the reference's bound of the fp64 value: at most two bounds apart, the same rows written, lat equal"""
    tol = IR.bound(IS.RANGES)
    worst = 0.0
    for h, e in zip(hip[:2], emu[:2]):
        np.testing.assert_array_equal(np.isnan(h), np.isnan(e))
        w = ~np.isnan(h[:, 0])
        np.testing.assert_array_equal(h[w][:, [0, 5, 6, 7]], e[w][:, [0, 5, 6, 7]])
        dist = np.abs(h[w].astype(np.float64) - e[w])
        assert (dist <= 2.0 * tol[None, :]).all()
        worst = max(worst, float((dist[:, 1:5] / tol[None, 1:5]).max()) if w.any() else 0.0)
    return worst


@pytest.mark.parametrize("N,env_stride,stream_id,tick", CASES)
def test_the_draw_cases_on_the_device_and_against_the_cpu_build(N, env_stride, stream_id, tick):
    hip = IS.freshness(hip_draw, N, env_stride, stream_id, tick)
    emu = IS.freshness(IB.DrawRig, N, env_stride, stream_id, tick)
    worst = _against_the_cpu_build(hip, emu)
    print(f"instrument draw N {N} stride {env_stride}: device at {hip[2]:.2f} of the reference's bound, CPU build at {emu[2]:.2f}; hip vs emu {worst:.2f} of it")
    for h, e in zip(IS.latency_spans(hip_draw, N, env_stride, tick), IS.latency_spans(IB.DrawRig, N, env_stride, tick)):
        np.testing.assert_array_equal(h, e)


def test_the_draw_on_a_side_stream():
    import torch
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for N, env_stride, stream_id, tick in CASES[1:3]:
            hip = IS.freshness(hip_draw, N, env_stride, stream_id, tick)
            _against_the_cpu_build(hip, IS.freshness(IB.DrawRig, N, env_stride, stream_id, tick))
    torch.cuda.synchronize()


def test_ranges_changed_in_place_and_zero_ranges():
    N = 257
    rig = hip_draw(N, seed=IS.SEED, rank=IS.RANK, stream_id=2, **IS.RANGES)
    before, _ = rig.read()
    everyone = np.ones(N, bool)
    assert rig.launch(9, IR.FILL_ALL) == 0
    first, _ = IS.check_rows(rig, before, everyone, 9, 2, "first ranges")
    rig.set_ranges(lat_lo=1, lat_hi=1, gain_lo=1.0, gain_hi=3.0, scale_range=0.0, quad_range=0.01, fov_range=0.05)       # the same struct, the same buffer
    assert rig.launch(9, IR.FILL_ALL) == 0
    second, _ = IS.check_rows(rig, first, everyone, 9, 2, "second ranges")
    assert (second[:, 0] == 1).all() and (second[:, 2] == 0).all() and (IS.bits(second[:, [1, 3, 4]]) != IS.bits(first[:, [1, 3, 4]])).all()
    rig.set_ranges(**dict(IB.NEUTRAL, lat_lo=2, lat_hi=2))
    assert rig.launch(9, IR.FILL_ALL) == 0
    assert (rig.read()[0] == IB.neutral_rows(N, 2)).all()
    IS.zero_ranges(hip_draw, N)


def test_sensitivity_and_statistics_on_the_device():
    hip, emu = IS.sensitivity(hip_draw), IS.sensitivity(IB.DrawRig)
    np.testing.assert_array_equal(hip[:, 0], emu[:, 0])
    tol = IR.bound(dict(IS.RANGES, lat_lo=0, lat_hi=7))
    assert (np.abs(hip.astype(np.float64) - emu) <= 2.0 * tol[None, :]).all()
    IS.statistics(hip_draw)


def test_draw_refusals_on_the_device_leave_the_rows_untouched():
    from isaacgymloco_amd import lib
    from test_sensor_instrument import draw_refusals
    L = lib.load()
    draw_refusals(hip_draw, lambda: L.lsim_sensor_instrument(None, None))


# ---- the capture
def test_neutral_rows_write_the_bits_of_lsim_sensor_capture_on_the_device():
    from test_sensor_instrument import bodies_neutral
    model = dict(SC.MODEL3, **IS.SCHED)
    hist = IS.neutral(lambda: IS.plane_rig(hip_rig, **model))
    assert len({h.tobytes() for h in hist}) == len(hist)
    IS.neutral(lambda: IS.plane_rig(hip_rig, env_stride=2, **model))
    bodies_neutral(hip_rig)


def test_per_env_latency_on_the_device():
    hip, emu = IS.latency(hip_rig), IS.latency(IB.CaptureRig)
    import sensor_model_reference as SR
    tol = SR.atol(dict(IB.SB.IDENTITY, clip_lo=0.0, clip_hi=SC.FAR), SC.FAR)       # as the schedule of lsim_sensor_capture: two builds of the same fp32 model
    for h, e in zip(hip, emu):
        assert np.abs(h - e).max() <= tol


def test_calibration_and_noise_on_the_device_and_against_the_cpu_build():
    (hip, share_h), (emu, share_e) = IS.calibration(hip_rig), IS.calibration(IB.CaptureRig)
    print(f"instrument capture: device at {share_h:.2f} of the bound, CPU build at {share_e:.2f}")
    p = dict(IB.SB.IDENTITY, **SC.MODEL3)
    y_lo = (np.float32(p["clip_lo"]) - np.float32(p["offset"])) * np.float32(p["gain"])
    for yh, ye in zip(hip, emu):
        np.testing.assert_array_equal(yh == y_lo, ye == y_lo)            # the dropped pixels


@pytest.mark.parametrize("T", [0.95, 1.05])
def test_a_scaled_field_of_view_on_the_device(T):
    """the truth check (every ray in the float64 envelope at the host-transformed directions) and the consistency check: the device against
    the CPU build of the same source differs by more than 1e-4 m on no ray"""
    hip, emu = IS.fov(hip_rig, (T,))[T], IS.fov(IB.CaptureRig, (T,))[T]
    diff = np.abs(hip.astype(np.float64) - emu)
    print(f"instrument fov T {T}: hip vs emu max |difference| {diff.max():.3e} m, {int((diff > 1e-4).sum())} rays beyond 1e-4 m")
    assert not (diff > 1e-4).any()


def test_rays_at_or_behind_the_image_plane_on_the_device():
    hip, emu = IS.unscaled_rays(hip_rig), IS.unscaled_rays(IB.CaptureRig)
    assert np.abs(hip - emu).max() <= 1e-4


def test_capture_refusals_on_the_device_write_nothing():
    from isaacgymloco_amd import lib
    from test_sensor_instrument import capture_refusals
    L = lib.load()
    capture_refusals(hip_rig, lambda: L.lsim_sensor_capture_inst(None, None, None))
