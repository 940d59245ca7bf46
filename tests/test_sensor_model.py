"""CPU: the sensor-model source (isaacgymloco_amd/csrc/ls_sensor_model.h) compiled by g++ under LS_EMU, against the numpy reference of
tests/sensor_model_reference.py (written from include/lsim.h; its docstring states the tolerance), against the emulated lsim_raycast /
lsim_raycast_bodies launches bit for bit, and through envs/sensors.py on the emulated LeggedRobot.  The same scenarios run on the HIP launch
in tests/test_gpu_sensor_model.py."""
import math

import numpy as np
import pytest

import raycast_bodies_emu_binding as BE
import raycast_bodies_scenes as BS
import raycast_emu_binding as EMU
import sensor_model_emu_binding as SB
import sensor_model_reference as SR
import sensor_model_scenes as SC
from helpers import abi


def test_identity_model_equals_lsim_raycast_bit_for_bit():
    SC.identity(SB.Rig, EMU.cast)


def test_identity_model_on_a_body_scene_equals_lsim_raycast_bodies_bit_for_bit():
    sc, tabs, rs, th, mt, dirs, scale, flags = BS.case_inputs(BS.CASES[1])
    want, wlab, _, _ = BE.cast(sc, tabs, BS.ENV_ROBOT, rs, th, mt, dirs, BS.NEAR, BS.FAR, scale=scale, flags=flags)
    rig = SB.Rig(sc, rs, mt, dirs, BS.NEAR, BS.FAR, scale=scale, bodies=dict(tables=tabs, env_robot=BS.ENV_ROBOT, dof_pos=th, flags=flags))
    assert rig.launch(0) == 0
    out, lab, hist, state = rig.read()
    np.testing.assert_array_equal(SC.bits(out), SC.bits(want))
    np.testing.assert_array_equal(lab, wlab)
    np.testing.assert_array_equal(SC.bits(hist[:, 0]), SC.bits(want))
    assert state[0] == 0 and (lab >= 2).mean() > 0.02, "the scene must show the robot"


@pytest.mark.parametrize("env_stride", [1, 2])
def test_schedule_history_and_untouched_rows(env_stride):
    SC.schedule(SB.Rig, EMU.cast, env_stride)


def test_noise_dropout_clip_and_normalisation():
    SC.model(SB.Rig)


def test_the_three_uniform_normal_has_unit_variance_and_is_bounded():
    """the reference's own g over the same counters: what the header claims about it"""
    u = SR.uniforms(7, 2, np.arange(SC.N), 3, 3, SC.R)
    g = SR.gauss(u)
    assert np.abs(g).max() <= 3.0 and abs(float(g.var()) - 1.0) < 0.1 and abs(float(g.mean())) < 0.1
    assert (SR.uniforms(7, 2, np.arange(SC.N), 3, 4, SC.R) != u).mean() > 0.99          # stream_id enters the counter


def test_every_invalid_argument_is_refused_and_nothing_is_written():
    L = SB.lib()
    sc, tabs, rs, th, mt, dirs, scale, flags = BS.case_inputs(BS.CASES[0])
    body = dict(tables=tabs, env_robot=BS.ENV_ROBOT, dof_pos=th)

    def rv(edit, bodies=None, **kw):
        kw = dict(dict(latency=1, frames=2), **kw)
        rig = SC.plane_rig(SB.Rig, **kw) if bodies is None else SB.Rig(sc, rs, mt, dirs, BS.NEAR, BS.FAR, scale=scale, bodies=bodies, **kw)
        rig.put("out", -7.0)
        r = rig.launch(3, 0, edit)
        if r != 0:
            out, lab, hist, state = rig.read()
            assert (out == -7.0).all() and (lab == 255).all() and (hist == -7.0).all() and (state == 0).all()
        return r

    assert rv(None) == 0 and rv(None, body) == 0
    assert L.emu_sensor_capture(None, None) == abi.E_INVALID
    nan, inf = math.nan, math.inf

    def s(name, value):
        return lambda sm: setattr(sm, name, value)

    def rb(name, value):
        return lambda sm: setattr(sm.rb, name, value)

    def rc(name, value):
        return lambda sm: setattr(sm.rb.rc, name, value)

    edits = {
        "episode_length NULL": s("episode_length", None), "episode_length misaligned": lambda sm: setattr(sm, "episode_length", sm.episode_length + 4),
        "hist NULL": s("hist", None), "hist misaligned": lambda sm: setattr(sm, "hist", sm.hist + 8),
        "tick < 0": s("tick", -1), "stream_id 65536": s("stream_id", 65536), "period 0": s("period", 0), "period < 0": s("period", -3),
        "stagger 2": s("stagger", 2), "stagger -1": s("stagger", -1), "latency -1": s("latency", -1), "frames 0": s("frames", 0),
        "latency + frames 9": s("latency", abi.DEFINES["LSIM_SENSOR_MAX_HISTORY"] - 1), "frames huge": s("frames", 2 ** 31 - 1),
        "hist_stride < R": s("hist_stride", SC.R - 4), "hist_stride odd": s("hist_stride", SC.R + 2),
        "sigma0 < 0": s("sigma0", -0.01), "sigma0 nan": s("sigma0", nan), "sigma2 < 0": s("sigma2", -1.0), "sigma2 inf": s("sigma2", inf),
        "p_drop < 0": s("p_drop", -0.1), "p_drop > 1": s("p_drop", 1.5), "p_drop nan": s("p_drop", nan), "drop_value nan": s("drop_value", nan),
        "clip_lo > clip_hi": s("clip_lo", 6.0), "clip_lo -inf": s("clip_lo", -inf), "clip_hi inf": s("clip_hi", inf), "clip_hi nan": s("clip_hi", nan),
        "offset nan": s("offset", nan), "gain inf": s("gain", inf),
        "unknown flag": s("flags", 4), "both flags": s("flags", SR.FILL_ALL | SR.RESETS_ONLY),
        # the terrain-only form: what lsim_raycast refuses, and the fields that make it that form
        "rc: out NULL": rc("out", None), "rc: near = far": rc("near", SC.FAR), "rc: R 0": rc("num_rays", 0), "rc: env_stride 0": rc("env_stride", 0),
        "terrain only with rb.flags": rb("flags", abi.RAYCAST_FRAME_YAW), "robots NULL with num_robots 1": rb("num_robots", 1),
        "label_stride short": rb("label_stride", SC.R - 1),
    }
    for what, edit in edits.items():
        assert rv(edit) == abi.E_INVALID, what
    body_edits = {
        "dof_state NULL": rb("dof_state", None), "robots_host NULL": rb("robots_host", None), "num_robots 0 with robots": rb("num_robots", 0),
        "two robots without env_robot": rb("env_robot", None), "unknown rb flag": rb("flags", 2), "label_stride short": rb("label_stride", 3),
        "rc: state NULL": rc("state", None), "hist NULL": s("hist", None), "both flags": s("flags", 3),
    }
    for what, edit in body_edits.items():
        assert rv(edit, body) == abi.E_INVALID, what
    # the limits themselves are accepted: K = 8, p_drop 0 and 1, clip_lo == clip_hi, stream_id 65535, either flag alone
    assert rv(None, latency=3, frames=5) == 0 and rv(s("p_drop", 1.0)) == 0 and rv(s("clip_lo", SC.FAR)) == 0 and rv(s("stream_id", 65535)) == 0
    assert rv(s("flags", SR.FILL_ALL)) == 0 and rv(s("flags", SR.RESETS_ONLY)) == 0 and rv(rb("labels", None)) == 0


def test_ray_sensor_with_a_model_on_the_emulated_env():
    import torch
    import eval_emu_binding
    from helpers import C
    from isaacgymloco_amd import lib
    from isaacgymloco_amd.envs import sensors
    cfg = C.mixed_cfg("aliengo", {"aliengo": 0.5, "go2": 0.5})[0]
    cfg.env.num_envs = 4
    cfg.terrain.num_rows, cfg.terrain.num_cols = 2, 2
    cfg.terrain.terrain_proportions = [0.0, 0.0, 0.0, 0.0, 0.5, 0.5]
    env = eval_emu_binding.emu_mixed_env(cfg)
    env.reset()
    api = SB.EmuApi()
    seen = []
    capture = api.lsim_sensor_capture

    def recording(smp, stream):
        sm = smp._obj
        seen.append((int(sm.tick), int(sm.flags), int(sm.stream_id)))
        return capture(smp, stream)
    api.lsim_sensor_capture = recording

    # model=None: the launch and the allocations of before
    plain = env.add_sensor("plain", sensors.depth_camera(env, 6, 4, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, api=api, see_robot=True))
    assert api.calls == {"lsim_raycast": 0, "lsim_raycast_bodies": 0, "lsim_sensor_capture": 0}
    assert plain.model is None and plain.stage("capture") is None and plain.chain() == ("lsim_raycast_bodies",) and plain.stream_id == 0
    with pytest.raises(ValueError):
        plain.frames()
    with pytest.raises(ValueError):
        plain.refresh()

    class Old:                                # a library from before the entry point
        lsim_raycast = lsim_raycast_sizes = lsim_raycast_bodies = lsim_raycast_bodies_sizes = None
    with pytest.raises(lib.LsimError, match="lsim_sensor_capture"):
        sensors.depth_camera(env, 6, 4, 87.0, api=Old(), model=sensors.SensorModel())
    for bad in (dict(period=0), dict(frames=0), dict(latency=-1), dict(latency=4, frames=5), dict(noise=(-1.0, 0.0)), dict(dropout=1.5), dict(clip=(2.0, 1.0))):
        with pytest.raises(ValueError):
            sensors.SensorModel(**bad)

    m = sensors.SensorModel(period=2, stagger=True, latency=1, frames=2, clip=(0.1, 3.0), normalise=True)
    cam = sensors.depth_camera(env, 6, 4, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, api=api, see_robot=True, model=m)
    assert seen == [] and cam.tick == -1
    assert env.add_sensor("depth", cam) is cam
    # add_sensor: stream_id = the index in env.sensors, one refresh()
    assert seen == [(env.common_step_counter, SR.FILL_ALL, 1)] and cam.stream_id == 1 and cam.tick == env.common_step_counter
    sm = cam.stage("capture").struct
    assert (sm.seed, sm.rank) == (env.lcfg.seed, env.lcfg.rank) and sm.episode_length == env.episode_length_buf.data_ptr()
    assert abs(sm.offset - 1.55) < 1e-6 and abs(sm.gain - 1 / 2.9) < 1e-6 and (sm.clip_lo, sm.clip_hi) == (np.float32(0.1), np.float32(3.0))
    assert cam.frames().shape == (4, 2, 24) and cam.frame_images().shape == (4, 2, 4, 6) and cam.frame_images().data_ptr() == cam.history().data_ptr()
    assert cam.history().shape == (4, 3, 24)
    h = cam.history().numpy()
    assert (h[:, 1:] == h[:, :1]).all() and np.abs(h).max() <= 0.5
    plain.update()
    np.testing.assert_array_equal(cam.out.numpy(), plain.out.numpy())
    np.testing.assert_array_equal(h[:, 0], (np.clip(cam.out.numpy(), np.float32(0.1), np.float32(3.0)) - sm.offset) * sm.gain)
    # default clip and no normalisation
    lid = sensors.lidar(env, 2, 20.0, 8, far=6.0, api=api, model=sensors.SensorModel())
    assert (lid.stage("capture").struct.clip_lo, lid.stage("capture").struct.clip_hi, lid.stage("capture").struct.offset, lid.stage("capture").struct.gain) == (np.float32(0.05), 6.0, 0.0, 1.0) and lid.stage("capture").struct.rb.robots is None
    # step_device: the tick is common_step_counter before its increment, no flag
    del seen[:]
    g = torch.Generator().manual_seed(4)
    for k in range(2):
        before, t = cam.history().numpy().copy(), env.common_step_counter
        env.step_device(torch.randn(4, 12, generator=g) * 0.3)
        assert seen[-1] == (t, 0, 1) and cam.tick == t and env.common_step_counter == t + 1
        el = env.episode_length_buf.numpy()
        due, fill = SR.due_sets(4, 1, t, 2, True, 0, el)
        after = cam.history().numpy()
        np.testing.assert_array_equal(after[~due], before[~due])
        keep = due & ~fill
        np.testing.assert_array_equal(after[keep, :2], before[keep, 1:])
        assert keep.any() and not (after[keep, 2] == before[keep, 2]).all()
    assert api.calls["lsim_sensor_capture"] == 3 and api.calls["lsim_raycast_bodies"] == 3
    # reset_idx by hand: RESETS_ONLY, only the env that was reset changes
    before = cam.history().numpy().copy()
    env.reset_idx([2])
    assert seen[-1] == (env.common_step_counter, SR.RESETS_ONLY, 1)
    after = cam.history().numpy()
    others = np.array([True, True, False, True])
    np.testing.assert_array_equal(after[others], before[others])
    assert (after[2, 1:] == after[2, :1]).all() and not (after[2] == before[2]).all()
