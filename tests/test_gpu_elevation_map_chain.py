"""GPU: the elevation map through envs/sensors.py on a full LeggedRobot -- 64 Aliengo envs on stairs with a 64 x 48 camera and a "clean"
map, held to the terrain's own height grid -- and through a vision policy's checkpoint and evaluation."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, FAR = 64, 5.0


def _env(seed, num_envs=N, cls=None, device=DEV):
    from isaacgymloco_amd.envs import config as C
    from isaacgymloco_amd.envs.legged_robot import LeggedRobot
    from isaacgymloco_amd.learn.evaluate import play_cfg
    cfg = play_cfg(C.aliengo_cfg())
    cfg.env.num_envs = num_envs
    cfg.terrain.num_rows, cfg.terrain.num_cols = 2, 2
    cfg.terrain.terrain_proportions = [0.0, 0.0, 0.0, 0.0, 0.5, 0.5]       # stairs up and down
    env = (cls or LeggedRobot)(cfg, sim_device=device, seed=seed)
    env.reset()
    return env


def _camera(env, api=None, width=64, height=48, **kw):
    from isaacgymloco_amd.envs import sensors
    kw.setdefault("model", sensors.SensorModel(period=2, stagger=True, latency=1, frames=2))
    return sensors.depth_camera(env, width, height, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, near=0.05, far=FAR, api=api, **kw)


def envelope_violations(env, cam):
    """known scan values outside [min, max] of the terrain surface within res * sqrt(2) + horizontal_scale + EPS of their point, beyond EPS
    in z.  The surface is the height grid's, the terrain object's own (no sensor is asked): the vertices within the radius, whose
    horizontal_scale term covers the cell a point lies in and the grid step a slope-corrected vertex is moved by.  Returns (violations, checked)"""
    import elevation_map_reference as ER
    t = env.cfg.terrain
    hs, res = float(t.horizontal_scale), cam.map.resolution
    grid = env.terrain.heightsamples.astype(np.float64) * t.vertical_scale
    rs = env.root_states[:, :7].cpu().numpy().astype(np.float64)
    pts, scan, known = cam.stage("map").buffers["pts"].cpu().numpy().astype(np.float64), cam.map_scan().cpu().numpy(), cam.map_known().cpu().numpy().astype(bool)
    n = 1.0 / np.sqrt(rs[:, 5] ** 2 + rs[:, 6] ** 2)
    qy = np.stack((np.zeros(len(rs)), np.zeros(len(rs)), rs[:, 5] * n, rs[:, 6] * n), axis=1)
    w = rs[:, None, :2] + ER.rot(qy[:, None, :], np.concatenate((pts, np.zeros((len(pts), 1))), axis=1)[None])[..., :2]
    eps = ER.eps(np.abs(rs[:, :3]).max(axis=0), (0.3, 0.0, 0.05), FAR)
    radius = res * np.sqrt(2.0) + hs + eps
    k = int(np.ceil(radius / hs)) + 1
    off = np.arange(-k, k + 1)
    bad = checked = 0
    for e, j in zip(*np.nonzero(known)):
        c = np.round((w[e, j] + t.border_size) / hs).astype(int)
        a, b = np.clip(c[0] + off, 0, grid.shape[0] - 1), np.clip(c[1] + off, 0, grid.shape[1] - 1)
        vx, vy = a * hs - t.border_size, b * hs - t.border_size
        near = np.hypot((vx - w[e, j, 0])[:, None], (vy - w[e, j, 1])[None, :]) <= radius
        h = grid[np.ix_(a, b)][near]
        checked += 1
        bad += not (h.min() - eps <= scan[e, j] <= h.max() + eps)
    return bad, checked


def test_on_stairs_every_known_scan_value_lies_inside_the_terrains_envelope():
    from isaacgymloco_amd.envs import sensors
    env = _env(5)
    cam = env.add_sensor("depth", _camera(env))
    cam.attach_map(sensors.ElevationMap(size=32, source="clean"))
    g = torch.Generator().manual_seed(2)
    coverage = []
    for step in range(30):
        env.step_device((torch.randn(N, 12, generator=g) * 0.3).to(DEV))
        coverage.append(float(cam.map_known().float().mean()))
    torch.cuda.synchronize()
    bad, checked = envelope_violations(env, cam)
    print(f"elevation map on stairs: {checked} known scan points of {N * 187}, {bad} outside the envelope; coverage {coverage[0]:.3f} -> {coverage[-1]:.3f}")
    assert checked > N * 10 and bad == 0, "occlusion only makes points unknown, never wrong"
    assert int(cam.map_nonfinite) == 0 and int(cam.nonfinite_rays) == 0 and bool(torch.isfinite(cam.map_scan()).all())
    hts = cam.map_heights()
    assert tuple(hts.shape) == (N, 32, 32) and bool(torch.isnan(hts).any()) and bool((~torch.isnan(hts)).any())


def test_evaluate_with_the_two_columns_and_a_checkpoint_whose_camera_carries_a_map(tmp_path):
    from isaacgymloco_amd.envs import sensors
    from isaacgymloco_amd.learn.bench_train import train_cfg_dict
    from isaacgymloco_amd.learn.depth_encoder import DepthEncoder
    from isaacgymloco_amd.learn.evaluate import evaluate
    from isaacgymloco_amd.learn.vision import VisionOnPolicyRunner
    env = _env(5)
    cam = env.add_sensor("depth", _camera(env))
    m = cam.attach_map(sensors.ElevationMap(size=32, source="noisy"))
    tc = train_cfg_dict("aliengo")
    tc["runner"]["num_steps_per_env"] = 4
    torch.manual_seed(5)
    run = VisionOnPolicyRunner(env, tc, sensor="depth", encoder=DepthEncoder(48, 64, 2), device=DEV)
    path = str(tmp_path / "model.pt")
    run.save(path)
    record = torch.load(path, map_location="cpu", weights_only=False)["vision"]["sensor"]
    assert record["map"] == m.record() and record == cam.spec()
    env2 = _env(9)
    cam2 = env2.add_sensor("depth", sensors.from_spec(env2, record))          # as the command line builds it
    assert cam2.map == m
    named = ("scan_error", "map_scan_error", "map_coverage")
    res = evaluate(env2, path, 20, commands=(0.8, 0.0, 0.0), vision_metrics=named).result()
    torch.cuda.synchronize()
    cols = res["total"]["columns"]
    assert list(cols) == list(named) and all(c["nonfinite"] == 0 and np.isfinite(c["mean"]) for c in cols.values())
    assert 0.0 < cols["map_coverage"]["mean"] <= 1.0 and cols["map_scan_error"]["mean"] >= 0.0
    print("evaluate with a map:", {k: round(v["mean"], 5) for k, v in cols.items()})
    res = evaluate(_env_with(record, 11), path, 5, commands=(0.8, 0.0, 0.0)).result()
    assert list(res["total"]["columns"]) == ["depth_influence", "scan_error"], "the defaults stay as they are"


def _env_with(record, seed):
    from isaacgymloco_amd.envs import sensors
    env = _env(seed)
    env.add_sensor("depth", sensors.from_spec(env, record))
    return env
