"""GPU: the sensor-model launch (lsim_sensor_capture, isaacgymloco_amd/csrc/ls_sensor_model.h) on a real device: the scenarios of
tests/sensor_model_scenes.py against the numpy reference (tests/sensor_model_reference.py states the tolerance) and against the CPU build of
the same source, bit for bit against lsim_raycast / lsim_raycast_bodies on the device, a strided staircase scene with a non-finite env, and
envs/sensors.py on a full mixed-robot LeggedRobot.  Every GPU step is one launch or a few env steps."""
import numpy as np
import pytest

import raycast_bodies_scenes as BS
import raycast_scenes as S
import sensor_model_emu_binding as SB
import sensor_model_reference as SR
import sensor_model_scenes as SC

pytestmark = pytest.mark.gpu


def hip_rig(*a, **kw):
    from isaacgymloco_amd import lib
    return SB.Rig(*a, device="cuda:0", entry=lib.load().lsim_sensor_capture, **kw)


def test_identity_model_equals_lsim_raycast_on_the_device_bit_for_bit():
    from test_gpu_raycast import hip_cast
    SC.identity(hip_rig, hip_cast)


def test_identity_model_on_a_body_scene_equals_lsim_raycast_bodies_on_the_device_bit_for_bit():
    from test_gpu_raycast_bodies import hip_cast_bodies
    sc, tabs, rs, th, mt, dirs, scale, flags = BS.case_inputs(BS.CASES[1])
    want, wlab, _ = hip_cast_bodies(sc, tabs, BS.ENV_ROBOT, rs, th, mt, dirs, BS.NEAR, BS.FAR, scale=scale, flags=flags)
    rig = hip_rig(sc, rs, mt, dirs, BS.NEAR, BS.FAR, scale=scale, bodies=dict(tables=tabs, env_robot=BS.ENV_ROBOT, dof_pos=th, flags=flags))
    assert rig.launch(0) == 0
    out, lab, hist, state = rig.read()
    np.testing.assert_array_equal(SC.bits(out), SC.bits(want))
    np.testing.assert_array_equal(lab, wlab)
    np.testing.assert_array_equal(SC.bits(hist[:, 0]), SC.bits(want))
    assert state[0] == 0 and (lab >= 2).mean() > 0.02


def test_schedule_on_the_device_and_against_the_cpu_build():
    from test_gpu_raycast import hip_cast
    import raycast_emu_binding as EMU
    hip = SC.schedule(hip_rig, hip_cast)
    emu = SC.schedule(SB.Rig, EMU.cast)
    tol = SR.atol(dict(SB.IDENTITY, clip_lo=0.0, clip_hi=SC.FAR), SC.FAR)
    worst = 0.0
    for (due_h, hist_h), (due_e, hist_e) in zip(hip, emu):
        np.testing.assert_array_equal(due_h, due_e)
        worst = max(worst, float(np.abs(hist_h - hist_e).max()))
    print(f"schedule: hip vs emu max |hist difference| {worst:.3e} (bound {tol:.3e})")
    assert worst <= tol


def test_model_on_the_device_and_against_the_cpu_build():
    hip = SC.model(hip_rig)
    emu = SC.model(SB.Rig)
    p = dict(SB.IDENTITY, **SC.MODEL3)
    tol = SR.atol(p, SC.FAR)
    y_lo = (np.float32(p["clip_lo"]) - np.float32(p["offset"])) * np.float32(p["gain"])
    worst = 0.0
    for yh, ye in zip(hip, emu):
        np.testing.assert_array_equal(yh == y_lo, ye == y_lo)            # the dropped pixels
        worst = max(worst, float(np.abs(yh - ye).max()))
    print(f"model: hip vs emu max |y difference| {worst:.3e} (bound {tol:.3e})")
    assert worst <= tol


def test_staircase_with_env_stride_and_a_nonfinite_env():
    sc, rs, mt, dirs, scale = S.case_inputs(("stairs_up", "stairs_up", 2, None, S.BORDER))
    rs[2, 0] = np.nan
    N, R = rs.shape[0], dirs.shape[0]
    rig = hip_rig(sc, rs, mt, dirs, S.NEAR, S.FAR, scale=scale, env_stride=2, latency=1, frames=2, **SC.MODEL3)
    assert rig.launch(3) == 0
    out, lab, hist, state = rig.read()
    assert state[0] == R and np.isfinite(hist[0::2]).all() and np.isfinite(out[0::2]).all()
    assert np.isnan(out[1::2]).all() and (hist[1::2] == -7.0).all() and (lab[1::2] == 255).all()
    far_s = np.float32(S.FAR) * scale
    np.testing.assert_array_equal(out[2], far_s)
    assert (lab[2] == 0).all()
    p = rig.p
    want, dropped = SR.model(far_s[None, :], np.zeros((1, R), bool), [2], 3, p)       # the model applied to far * scale: a miss, so no noise and no hole
    np.testing.assert_array_equal(SC.bits(hist[2, 2]), SC.bits(want[0]))
    assert not dropped.any() and (hist[0::2, :2] == -7.0).all()                        # the two older slots: the shifted initial value
    # the finite envs: the model of the reference on the launch's own clean frame
    want, _ = SR.model(out[[0, 4]], lab[[0, 4]] != 0, [0, 4], 3, p)
    assert np.abs(hist[[0, 4], 2] - want).max() <= SR.atol(p, S.FAR)
    assert (lab[[0, 4]] == 1).mean() > 0.3


def _stairs_env():
    from test_gpu_raycast import stairs_env
    return stairs_env(256)


def test_modelled_camera_on_a_mixed_robot_env_on_stairs():
    """N = 256, Aliengo + Go2 on stairs, 12 steps of random actions with some envs timing out on the way: a see_robot camera with period 4
    staggered, latency 1, two frames, next to a plain twin with model=None"""
    import torch
    from isaacgymloco_amd.envs import sensors
    from test_gpu_raycast import MOUNTS
    env = _stairs_env()
    k = torch.arange(256, device="cuda:0") % 32
    near_end = torch.where((k >= 5) & (k <= 7), int(env.max_episode_length) - 5 - k, torch.zeros_like(k))
    env.episode_length_buf = near_end.to(env.episode_length_buf.dtype)
    kw = dict(mount_pos={n: (-0.1, 0.0, 0.02) for n in MOUNTS}, pitch_deg=35.0, near=0.05, far=5.0, see_robot=True)
    cam = env.add_sensor("depth", sensors.depth_camera(env, 12, 8, 87.0, model=sensors.SensorModel(period=4, stagger=True, latency=1, frames=2), **kw))
    twin = env.add_sensor("twin", sensors.depth_camera(env, 12, 8, 87.0, **kw))
    assert cam.frames().shape == (256, 2, 96) and cam.frame_images().shape == (256, 2, 8, 12) and cam.stream_id == 0
    torch.cuda.synchronize()
    h0 = cam.history().cpu().numpy()
    assert (h0[:, 1:] == h0[:, :1]).all(), "add_sensor fills every slot"
    g = torch.Generator().manual_seed(2)
    resets = shifts = 0
    for _ in range(12):
        tick = env.common_step_counter
        hist_b, out_b = cam.history().clone(), cam.out.clone()
        env.step_device((torch.randn(256, 12, generator=g) * 0.5).to("cuda:0"))
        torch.cuda.synchronize()
        assert cam.tick == tick
        fill = (env.episode_length_buf == 0).cpu().numpy()
        due = fill | ((tick + np.arange(256)) % 4 == 0)
        hist_a, out_a, tw = cam.history().cpu().numpy(), cam.out.cpu().numpy(), twin.out.cpu().numpy()
        hist_b, out_b = hist_b.cpu().numpy(), out_b.cpu().numpy()
        np.testing.assert_array_equal(SC.bits(out_a[due]), SC.bits(tw[due]))
        y = np.clip(out_a, np.float32(0.05), np.float32(5.0))               # the default model: clip to (near, far), nothing else
        shift = due & ~fill
        np.testing.assert_array_equal(SC.bits(hist_a[shift, :2]), SC.bits(hist_b[shift, 1:]))
        np.testing.assert_array_equal(SC.bits(hist_a[shift, 2]), SC.bits(y[shift]))
        np.testing.assert_array_equal(SC.bits(hist_a[fill]), SC.bits(np.repeat(y[fill][:, None], 3, axis=1)))
        np.testing.assert_array_equal(SC.bits(cam.frames().cpu().numpy()), SC.bits(hist_a[:, :2]))
        np.testing.assert_array_equal(SC.bits(hist_a[~due]), SC.bits(hist_b[~due]))
        np.testing.assert_array_equal(SC.bits(out_a[~due]), SC.bits(out_b[~due]))
        resets += int(fill.sum())
        shifts += int(shift.sum())
    assert resets > 0 and shifts >= 256 * 2, "envs reset on the way and every env shifted its history"
    assert int(cam.nonfinite_rays) == 0 and int(twin.nonfinite_rays) == 0 and int(env.nonfinite_envs) == 0
