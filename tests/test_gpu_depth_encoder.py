"""GPU: the depth-encoder launch (lsim_depth_encode, isaacgymloco_amd/csrc/ls_depth_encoder.h) on a real device: the shapes and the schedule of
tests/depth_encoder_emu_binding.py against the numpy fp64 reference within its derived bound (tests/depth_encoder_reference.py), an in-place
weight update, and envs/sensors.py attach_encoder on a full mixed-robot LeggedRobot.  Every GPU step is one launch or a few env steps."""
import numpy as np
import pytest

import depth_encoder_emu_binding as DB
import depth_encoder_reference as R

pytestmark = pytest.mark.gpu


def hip_rig(*a, **kw):
    from isaacgymloco_amd import lib
    return DB.Rig(*a, device="cuda:0", entry=lib.load().lsim_depth_encode, **kw)


@pytest.mark.parametrize("name", sorted(DB.SHAPES))
def test_shape_on_the_device_within_the_bound_of_the_reference(name):
    DB.check_shape(name, hip_rig)


def test_due_rule_on_the_device_and_against_the_cpu_build():
    hip = DB.schedule(hip_rig)
    emu = DB.schedule(DB.Rig)
    for (due_h, lat_h), (due_e, lat_e) in zip(hip, emu):
        np.testing.assert_array_equal(due_h, due_e)
        np.testing.assert_array_equal(np.isnan(lat_h), np.isnan(lat_e))          # the rows each build wrote


def test_sizes_on_the_device_library():
    import ctypes
    from isaacgymloco_amd import lib
    s = DB.SHAPES["C"]
    rig = DB.Rig(s, DB.params_of(DB.module(s)), DB.images(s))
    n, m = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.load().lsim_depth_encode_sizes(ctypes.byref(rig.de), ctypes.byref(n)) == 0
    assert DB.lib().emu_depth_encode_sizes(ctypes.byref(rig.de), ctypes.byref(m)) == 0
    assert n.value == m.value > 64 * 1024


@pytest.fixture(scope="module")
def encoded_env():
    """the 256-env Aliengo + Go2 staircase env with a period-4 staggered camera and the default network attached to it"""
    import torch
    from isaacgymloco_amd.envs import sensors
    from isaacgymloco_amd.learn.depth_encoder import DepthEncoder
    from test_gpu_raycast import MOUNTS, stairs_env
    env = stairs_env(256)
    k = torch.arange(256, device="cuda:0") % 32
    near_end = torch.where((k >= 5) & (k <= 7), int(env.max_episode_length) - 2 - k, torch.zeros_like(k))      # some envs time out on the way
    env.episode_length_buf = near_end.to(env.episode_length_buf.dtype)
    torch.manual_seed(11)
    enc = DepthEncoder(12, 16, 2).to("cuda:0")
    model = sensors.SensorModel(period=4, stagger=True, latency=1, frames=2, noise=(0.01, 0.002), dropout=0.02, normalise=True)
    cam = sensors.depth_camera(env, 16, 12, 87.0, mount_pos={n: (-0.1, 0.0, 0.02) for n in MOUNTS}, pitch_deg=35.0, near=0.05, far=5.0, see_robot=True, model=model)
    env.add_sensor("depth", cam)
    cam.attach_encoder(enc)
    return env, cam, enc


def _reference(cam, enc):
    import torch
    torch.cuda.synchronize()
    x = cam.frame_images().cpu().numpy().astype(np.float64)
    return R.encode(x, DB.params_of(enc), 2, 2, True)


def test_encoder_on_a_mixed_robot_env_on_stairs(encoded_env):
    import torch
    env, cam, enc = encoded_env
    assert cam.latent().shape == (256, 64)
    want, bound = _reference(cam, enc)
    got = cam.latent().cpu().numpy()
    assert (np.abs(got - want) <= bound).all(), "attach_encoder encodes every env from the present history"
    g = torch.Generator().manual_seed(2)
    worst, encoded, resets = 0.0, 0, 0
    for _ in range(8):
        tick, before = env.common_step_counter, cam.latent().cpu().numpy()
        env.step_device((torch.randn(256, 12, generator=g) * 0.5).to("cuda:0"))
        torch.cuda.synchronize()
        fill = (env.episode_length_buf == 0).cpu().numpy()
        due = fill | ((tick + np.arange(256)) % 4 == 0)
        want, bound = _reference(cam, enc)
        after = cam.latent().cpu().numpy()
        np.testing.assert_array_equal(after[~due].view(np.uint32), before[~due].view(np.uint32))
        worst = max(worst, float((np.abs(after[due] - want[due]) / bound[due]).max()))
        encoded += int(due.sum())
        resets += int(fill.sum())
    print(f"full env: {encoded} rows encoded over 8 steps ({resets} after a reset), worst |difference| / bound = {worst:.2e}")
    assert worst <= 1.0 and encoded >= 256 * 2 and resets > 0


def test_in_place_weight_update_is_seen_by_the_next_launch(encoded_env):
    import torch
    env, cam, enc = encoded_env
    before = cam.latent().cpu().numpy()
    ptrs = [p.data_ptr() for p in enc.parameters()]
    with torch.no_grad():
        for p in enc.parameters():
            p.add_(0.01 * torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())).to(p.device))
    assert ptrs == [p.data_ptr() for p in enc.parameters()]
    enc.encode_device(cam, env.common_step_counter, DB.FILL_ALL)          # the same history, the new weights
    want, bound = _reference(cam, enc)
    after = cam.latent().cpu().numpy()
    assert (np.abs(after - want) <= bound).all()
    assert (np.abs(after - before) > 10 * bound).mean() > 0.5, "the update moved the latent by far more than the bound"
