"""GPU: the map's visibility clean-up through envs/sensors.py on a full LeggedRobot: the planted phantom cells of
tests/test_elevation_cleanup_chain.py in front of robots walking over flat ground, forgotten with the clean-up and kept without it, and
the stage in a stepped env's chain on stairs."""
import pytest
import torch

from test_elevation_cleanup_chain import check_phantoms
from test_gpu_elevation_map_chain import DEV, FAR, N, _camera, _env

pytestmark = pytest.mark.gpu


def _plane_env(num_envs):
    from isaacgymloco_amd.envs import config as C
    from isaacgymloco_amd.envs.legged_robot import LeggedRobot
    from isaacgymloco_amd.learn.evaluate import play_cfg
    cfg = play_cfg(C.aliengo_cfg())
    cfg.env.num_envs = num_envs
    cfg.terrain.mesh_type = "plane"
    env = LeggedRobot(cfg, sim_device=DEV, seed=3)
    env.reset()
    return env


def test_planted_phantom_cells_are_forgotten_on_the_device_and_stay_without_the_cleanup():
    from isaacgymloco_amd.envs import sensors
    env = _plane_env(4)
    check_phantoms(env, _camera(env, None, 16, 12, model=sensors.SensorModel(clip=(0.0, FAR))))


def test_the_stage_runs_in_a_stepped_envs_chain_on_stairs():
    """a clean camera and the true pose on stairs: the chain holds the launch between the capture and the map's, nothing non-finite, and the
    share of the known cells forgotten per capture is printed"""
    from isaacgymloco_amd.envs import sensors
    env = _env(5)
    cam = env.add_sensor("depth", _camera(env))
    cam.attach_map(sensors.ElevationMap(size=32, source="clean", fusion=sensors.MapFusion(), cleanup=sensors.MapCleanup()))
    assert list(cam.chain()) == ["lsim_sensor_capture", "lsim_elevation_map_cleanup", "lsim_elevation_map_fused"]
    g = torch.Generator().manual_seed(2)
    forgotten = known = 0
    for step in range(30):
        before = cam.map_cleared().clone()
        known += int((cam.map_state()[1] >= 0).sum())
        env.step_device((torch.randn(N, 12, generator=g) * 0.3).to(DEV))
        now = cam.map_cleared()
        forgotten += int(torch.where(now >= before, now - before, now).sum())
    torch.cuda.synchronize()
    print(f"stairs, clean source, true pose, fused map, 30 steps of {N} envs: {forgotten} cells forgotten, {100.0 * forgotten / max(known, 1):.4f} % of the known cells per step")
    assert int(cam.map_nonfinite) == 0 and bool(torch.isfinite(cam.map_scan()).all()) and bool((cam.map_cleared() >= 0).all())
