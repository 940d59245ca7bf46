"""GPU: the fused elevation map through envs/sensors.py on a full LeggedRobot -- 64 Aliengo envs on stairs with a 64 x 48 camera and a
"clean" map with a fusion, held to the terrain's own height grid as the plain map is -- and learn/evaluate.py's two columns."""
import numpy as np
import pytest
import torch

from test_gpu_elevation_map_chain import DEV, N, _camera, _env, envelope_violations

pytestmark = pytest.mark.gpu


def test_on_stairs_every_known_fused_height_lies_inside_the_envelope_and_every_variance_inside_its_clamps():
    """a cell's mean is a convex combination of points on the surface inside the cell, and a fusion one of such means: the plain map's
    envelope holds for the fused map unchanged"""
    from isaacgymloco_amd.envs import sensors
    env = _env(5)
    cam = env.add_sensor("depth", _camera(env))
    f = sensors.MapFusion()
    cam.attach_map(sensors.ElevationMap(size=32, source="clean", fusion=f))
    assert list(cam.chain())[-1] == "lsim_elevation_map_fused"
    rows = cam.attach_map_rows(("height", "confidence"))
    g = torch.Generator().manual_seed(2)
    for step in range(30):
        env.step_device((torch.randn(N, 12, generator=g) * 0.3).to(DEV))
    torch.cuda.synchronize()
    bad, checked = envelope_violations(env, cam)
    var, known = cam.map_variance(), cam.map_known().bool()
    print(f"fused map on stairs: {checked} known scan points of {N * 187}, {bad} outside the envelope; variance {float(var[known].min()):.3g} .. {float(var[known].max()):.3g}")
    assert checked > N * 10 and bad == 0
    assert bool((var >= np.float32(f.var_floor)).all()) and bool((var <= np.float32(f.var_max)).all()) and bool((var[~known] == f.var_max).all())
    assert int(cam.map_nonfinite) == 0 and bool(torch.isfinite(cam.map_scan()).all()) and len(cam.map_state()) == 4
    conf = rows[:, 187:]
    assert bool((conf[known] > 0).all()) and bool((conf[known] <= 1).all()) and bool((conf[~known] == 0).all())
    ref = torch.full((), 16 * f.var_floor, dtype=torch.float32, device=DEV)
    want = ref / (ref + var)
    assert bool((conf[known] == want[known]).all()), "one correctly rounded quotient"


def test_evaluate_with_the_fusions_columns():
    from isaacgymloco_amd.envs import sensors
    from isaacgymloco_amd.learn.bench_train import train_cfg_dict
    from isaacgymloco_amd.learn.depth_encoder import DepthEncoder
    from isaacgymloco_amd.learn.evaluate import evaluate
    from isaacgymloco_amd.learn.vision import VisionOnPolicyRunner
    env = _env(5)
    model = sensors.SensorModel(period=2, stagger=True, latency=1, frames=2, noise=(0.01, 0.002))
    cam = env.add_sensor("depth", _camera(env, model=model))
    cam.attach_map(sensors.ElevationMap(size=32, source="noisy", fusion=sensors.MapFusion()))
    tc = train_cfg_dict("aliengo")
    tc["runner"]["num_steps_per_env"] = 4
    torch.manual_seed(5)
    run = VisionOnPolicyRunner(env, tc, sensor="depth", encoder=DepthEncoder(48, 64, 2), device=DEV)
    named = ("map_scan_error", "map_coverage", "map_variance", "map_z2")
    cols = evaluate(env, run, 20, commands=(0.8, 0.0, 0.0), vision_metrics=named).result()["total"]["columns"]
    torch.cuda.synchronize()
    assert list(cols) == list(named) and all(c["nonfinite"] == 0 and np.isfinite(c["mean"]) for c in cols.values())
    assert 2.5e-5 <= cols["map_variance"]["mean"] <= 0.25 and cols["map_z2"]["mean"] > 0.0
    print("evaluate with a fused map:", {k: round(v["mean"], 6) for k, v in cols.items()})
