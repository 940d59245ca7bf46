"""CPU: the instrument source (isaacgymloco_amd/csrc/ls_sensor_instrument.h) compiled by g++ under LS_EMU -- the draw launch
lsim_sensor_instrument and the capture lsim_sensor_capture_inst -- against the numpy reference of tests/sensor_instrument_reference.py (written
from include/lsim.h; its docstring derives the bounds).  The same scenarios run on the HIP launches in tests/test_gpu_sensor_instrument.py."""
import math

import numpy as np
import pytest

import raycast_bodies_scenes as BS
import sensor_instrument_emu_binding as IB
import sensor_instrument_reference as IR
import sensor_instrument_scenes as IS
import sensor_model_scenes as SC
from helpers import abi

SHAPES = [(N, stride) for N in (1, 255, 256, 257) for stride in (1, 3)]


# ---- the draw launch
@pytest.mark.parametrize("N,env_stride", SHAPES)
def test_fresh_rows_match_the_reference_and_the_others_are_untouched(N, env_stride):
    for stream_id, tick in ((0, 0), (3, IS.BIG_TICK)):
        _, _, worst = IS.freshness(IB.DrawRig, N, env_stride, stream_id, tick)
        print(f"instrument draw N {N} stride {env_stride} tick {tick}: CPU build at {worst:.2f} of the reference's bound")


@pytest.mark.parametrize("N,env_stride", SHAPES)
def test_the_latency_draw_equals_the_reference_exactly_for_spans_0_1_and_7(N, env_stride):
    for tick in (0, IS.BIG_TICK):
        IS.latency_spans(IB.DrawRig, N, env_stride, tick)


def test_the_big_tick_draws_what_its_low_word_draws():
    a = IS.freshness(IB.DrawRig, 257, 1, 3, IS.BIG_TICK)[1]
    b = IS.freshness(IB.DrawRig, 257, 1, 3, 5)[1]
    np.testing.assert_array_equal(IS.bits(a), IS.bits(b))


def test_zero_ranges_give_the_neutral_row_exactly():
    IS.zero_ranges(IB.DrawRig, 257)


def test_one_range_at_a_time_moves_one_column():
    N = 64
    neutral = IB.neutral_rows(N, 1)
    for col, r in ((0, dict(lat_lo=0, lat_hi=1)), (1, dict(gain_lo=0.5, gain_hi=2.0)), (2, dict(scale_range=0.02)), (3, dict(quad_range=0.005)),
                   (4, dict(fov_range=0.02))):
        rig = IB.DrawRig(N, seed=3, **dict(dict(IB.NEUTRAL, lat_lo=1, lat_hi=1), **r))
        assert rig.launch(2, IR.FILL_ALL) == 0
        got = rig.read()[0]
        others = [j for j in range(8) if j != col]
        assert (got[:, others] == neutral[:, others]).all(), col
        assert len(np.unique(got[:, col])) > (1 if col == 0 else N // 2), col


def test_a_launch_differs_with_tick_env_stream_seed_and_rank():
    IS.sensitivity(IB.DrawRig)


def test_the_draws_are_uniform_and_every_latency_is_as_likely():
    IS.statistics(IB.DrawRig)


def _draw_edits():
    nan, inf = math.nan, math.inf

    def s(name, value):
        return lambda si: setattr(si, name, value)

    edits = {
        "inst NULL": s("inst", None), "episode_length NULL": s("episode_length", None),
        "inst misaligned by 4": lambda si: setattr(si, "inst", si.inst + 4), "inst misaligned by 16": lambda si: setattr(si, "inst", si.inst + 16),
        "episode_length misaligned": lambda si: setattr(si, "episode_length", si.episode_length + 4),
        "num_envs 0": s("num_envs", 0), "num_envs < 0": s("num_envs", -4), "env_stride 0": s("env_stride", 0), "env_stride < 0": s("env_stride", -1),
        "tick < 0": s("tick", -1), "stream_id 65536": s("stream_id", 65536),
        "lat_lo < 0": s("lat_lo", -1), "lat_lo > lat_hi": s("lat_lo", 3), "lat_hi 8": s("lat_hi", abi.DEFINES["LSIM_SENSOR_MAX_HISTORY"]),
        "gain_lo < 0": s("gain_lo", -0.1), "gain_lo > gain_hi": s("gain_lo", 2.5), "gain_lo nan": s("gain_lo", nan), "gain_hi inf": s("gain_hi", inf),
        "gain_hi nan": s("gain_hi", nan), "fov_range 1": s("fov_range", 1.0),
        "unknown flag": s("flags", 4), "both flags": s("flags", IR.FILL_ALL | IR.RESETS_ONLY),
    }
    for name in ("scale_range", "quad_range", "fov_range"):
        edits.update({f"{name} < 0": s(name, -0.01), f"{name} nan": s(name, nan), f"{name} inf": s(name, inf)})
    return edits


def draw_refusals(make_rig, null_call):
    """every refusal of the header, with `inst` and its guard untouched; the limits themselves are accepted"""
    def rv(edit, flags=0):
        rig = make_rig(9, **IS.RANGES)
        rig.put("episode_length", 0)
        r = rig.launch(3, flags, edit)
        m, guard = rig.read()
        assert (guard == IB.GUARD_VALUE).all()
        assert np.isnan(m).all() if r != 0 else np.isfinite(m).all()
        return r

    assert rv(None) == 0
    assert null_call() == abi.E_INVALID
    for what, edit in _draw_edits().items():
        assert rv(edit) == abi.E_INVALID, what
    assert rv(lambda si: setattr(si, "stream_id", 65535)) == 0 and rv(None, IR.FILL_ALL) == 0 and rv(None, IR.RESETS_ONLY) == 0
    assert rv(lambda si: setattr(si, "tick", 2 ** 40)) == 0 and rv(lambda si: setattr(si, "lat_hi", 7)) == 0
    assert rv(lambda si: setattr(si, "fov_range", 0.999)) == 0 and rv(lambda si: setattr(si, "gain_lo", 2.0)) == 0


def test_every_invalid_draw_argument_is_refused_and_nothing_is_written():
    L = IB.lib()
    draw_refusals(IB.DrawRig, lambda: L.emu_sensor_instrument(None, None))


def test_the_library_refuses_the_same_draw_arguments_before_any_launch():
    """through lib.load(): the argument check runs on the host before any HIP call, so host arrays serve and no device is needed"""
    from isaacgymloco_amd import lib
    L = lib.load()
    assert L.lsim_sensor_instrument(None, None) == abi.E_INVALID
    for what, edit in _draw_edits().items():
        rig = IB.DrawRig(9, **IS.RANGES)
        rig._entry = L.lsim_sensor_instrument
        rig.put("episode_length", 0)
        assert rig.launch(3, 0, edit) == abi.E_INVALID, what
        m, guard = rig.read()
        assert np.isnan(m).all() and (guard == IB.GUARD_VALUE).all(), what


# ---- the capture
def bodies_rig(make_rig, **model):
    """the see-robot form: the staircase camera scene of tests/raycast_bodies_scenes.py (4 envs, two robots)"""
    sc, tabs, rs, th, mt, dirs, scale, flags = BS.case_inputs(BS.CASES[1])
    return make_rig(sc, rs, mt, dirs, BS.NEAR, BS.FAR, scale=scale, bodies=dict(tables=tabs, env_robot=BS.ENV_ROBOT, dof_pos=th, flags=flags), **model)


def test_neutral_rows_write_the_bits_of_lsim_sensor_capture_terrain_only():
    model = dict(SC.MODEL3, **IS.SCHED)
    hist = IS.neutral(lambda: IS.plane_rig(IB.CaptureRig, **model))
    assert len({h.tobytes() for h in hist}) == len(hist), "every launch changed the history"
    IS.neutral(lambda: IS.plane_rig(IB.CaptureRig, env_stride=2, **model))


def test_neutral_rows_write_the_bits_of_lsim_sensor_capture_with_the_robot_in_view():
    bodies_neutral(IB.CaptureRig)


def bodies_neutral(make_rig):
    """the schedule on the body scene's 4 envs: FILL_ALL, ticks with resets, RESETS_ONLY"""
    import sensor_model_reference as SR
    model = dict(SC.MODEL3, **IS.SCHED)
    a, b = bodies_rig(make_rig, **model), bodies_rig(make_rig, **model)
    assert a.N == 4
    bodies_seen = 0
    for tick, flags, zero in ((0, SR.FILL_ALL, ()), (1, 0, ()), (2, 0, (2,)), (3, 0, ()), (3, SR.RESETS_ONLY, (1, 3)), (4, 0, ()), (5, 0, (0,)), (6, 0, ())):
        el = np.full(4, 5, np.int64)
        el[list(zero)] = 0
        for r in (a, b):
            r.put("episode_length", el)
            r.put("out", np.nan)
            r.put("labels", 255)
        assert a.launch(tick, flags) == 0 and b.plain(tick, flags) == 0
        (oa, la, _, sa), (ob, lb, _, sb) = a.read(), b.read()
        np.testing.assert_array_equal(oa.view(np.int32), ob.view(np.int32))
        np.testing.assert_array_equal(la, lb)
        np.testing.assert_array_equal(a.get("hist").view(np.int32), b.get("hist").view(np.int32))
        np.testing.assert_array_equal(sa, sb)
        bodies_seen += int(((la >= 2) & (la != 255)).sum())
    assert bodies_seen > 0, "rays end on the robot"


def test_per_env_latency_follows_the_reference_state_machine_and_an_off_by_one_fails():
    IS.latency(IB.CaptureRig)


def test_calibration_error_and_noise_gain_lie_within_the_derived_bound():
    _, share = IS.calibration(IB.CaptureRig)
    print(f"instrument capture: the CPU build lands at {share:.2f} of the bound")


@pytest.mark.parametrize("T", [0.95, 1.05])
def test_a_scaled_field_of_view_casts_the_rays_the_header_says(T):
    IS.fov(IB.CaptureRig, (T,))


def test_rays_at_or_behind_the_image_plane_are_left_bit_for_bit():
    IS.unscaled_rays(IB.CaptureRig)


def _capture_edits():
    nan = math.nan

    def s(name, value):
        return lambda sm: setattr(sm, name, value)

    return {"episode_length NULL": s("episode_length", None), "hist NULL": s("hist", None), "hist misaligned": lambda sm: setattr(sm, "hist", sm.hist + 4),
            "tick < 0": s("tick", -1), "stream_id 65536": s("stream_id", 65536), "period 0": s("period", 0), "stagger 2": s("stagger", 2),
            "latency < 0": s("latency", -1), "frames 0": s("frames", 0), "latency + frames 9": s("latency", 7), "hist_stride < R": s("hist_stride", 256),
            "hist_stride odd": s("hist_stride", 262), "sigma0 < 0": s("sigma0", -1.0), "sigma2 nan": s("sigma2", nan), "p_drop > 1": s("p_drop", 1.5),
            "drop_value nan": s("drop_value", nan), "clip_lo > clip_hi": s("clip_lo", 9.0), "offset nan": s("offset", nan), "gain nan": s("gain", nan),
            "unknown flag": s("flags", 4), "both flags": s("flags", IR.FILL_ALL | IR.RESETS_ONLY),
            "rays: num_envs 0": lambda sm: setattr(sm.rb.rc, "num_envs", 0), "rays: out NULL": lambda sm: setattr(sm.rb.rc, "out", None),
            "rays: near >= far": lambda sm: setattr(sm.rb.rc, "near", 6.0), "robots NULL with num_robots 1": lambda sm: setattr(sm.rb, "num_robots", 1)}


def capture_refusals(make_rig, null_call):
    """what lsim_sensor_capture refuses, and inst NULL or not 16-byte aligned: nothing is written"""
    def rv(edit=None, **kw):
        rig = IS.plane_rig(make_rig, **IS.SCHED)
        rig.put("out", np.nan)
        r = rig.launch(3, IR.FILL_ALL, edit, **kw)
        out, lab, hist, state = rig.read()
        if r != 0:
            assert np.isnan(out).all() and (lab == 255).all() and (rig.get("hist") == -7.0).all() and (state == 0).all()
        else:
            assert np.isfinite(out).all() and np.isfinite(hist).all()
        return r

    assert rv() == 0
    assert null_call() == abi.E_INVALID
    for what, edit in _capture_edits().items():
        assert rv(edit) == abi.E_INVALID, what
    rig = IS.plane_rig(make_rig, **IS.SCHED)
    base = rig.ptr("inst")
    assert rv(inst=None) == abi.E_INVALID and rv(inst=base + 4) == abi.E_INVALID and rv(inst=base + 8) == abi.E_INVALID
    del rig


def test_every_invalid_capture_argument_is_refused_and_nothing_is_written():
    L = IB.lib()
    capture_refusals(IB.CaptureRig, lambda: L.emu_sensor_capture_inst(None, None, None))


def test_the_library_refuses_the_same_capture_arguments_before_any_launch():
    from isaacgymloco_amd import lib
    L = lib.load()

    def host_rig(*a, **kw):
        rig = IB.CaptureRig(*a, **kw)
        rig._inst_entry = L.lsim_sensor_capture_inst
        return rig
    assert L.lsim_sensor_capture_inst(None, None, None) == abi.E_INVALID
    for what, edit in _capture_edits().items():
        rig = IS.plane_rig(host_rig, **IS.SCHED)
        assert rig.launch(3, IR.FILL_ALL, edit) == abi.E_INVALID, what
        assert (rig.get("hist") == -7.0).all(), what
    rig = IS.plane_rig(host_rig, **IS.SCHED)
    assert rig.launch(3, 0, inst=None) == abi.E_INVALID and rig.launch(3, 0, inst=rig.ptr("inst") + 4) == abi.E_INVALID
    assert (rig.get("hist") == -7.0).all()
