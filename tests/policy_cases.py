"""TEST INFRASTRUCTURE -- one runner of every kind of policy checkpoint (HIM; vision, with a depth memory, with end_to_end; distilled; map;
scan) on the emulated LeggedRobot at the size tests/test_vision_deploy.py and tests/test_map_policy_chain.py use: 8 envs, a 16 x 12 camera,
4 rollout steps, every launch through the CPU builds of the kernel sources.  `build(case)` is deterministic: two calls give runners whose
weights, envs and sensors are bit-identical."""
import numpy as np
import torch

import emu_binding
from helpers import C
from isaacgymloco_amd.envs import sensors

CASES = ("him", "vision", "vision_memory", "vision_e2e", "distill", "map", "scan")
N, T, L, H = 8, 4, 10, 16
ENC = dict(c1=4, k1=3, s1=2, c2=8, k2=3, s2=1, latent_dim=L)
MODEL = dict(period=2, stagger=True, latency=1, frames=2, clip=(0.1, 3.0), normalise=True)
ODO = sensors.OdometryError(scale=0.02, yaw_per_m=0.05, z_per_m=0.02, noise=(0.005, 0.002, 0.002))
GRID = [[x, y] for x in np.linspace(-0.5, 0.5, 11) for y in np.linspace(-0.4, 0.4, 9)]          # 99 points: two channels fit the fused launch


def api():
    """the shims of every launch a sensor of these cases makes, for envs.sensors.RaySensor(api=...)"""
    return emu_binding.api("raycast", "raycast_bodies", "sensor_model", "depth_encoder", "depth_memory", "frames_log", "elevation_map", "odometry", "map_rows")


def env(seed=3):
    from emu_env import EmuLeggedRobot
    from isaacgymloco_amd.learn.evaluate import play_cfg
    cfg = play_cfg(C.aliengo_cfg())
    cfg.env.num_envs = N
    cfg.terrain.num_rows, cfg.terrain.num_cols = 2, 2
    cfg.terrain.terrain_proportions = [0.0, 0.0, 0.0, 0.0, 0.5, 0.5]
    e = EmuLeggedRobot(cfg, seed=seed)
    e.reset()
    return e


def camera(e, with_map=False):
    cam = e.add_sensor("depth", sensors.depth_camera(e, 16, 12, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, near=0.05, far=5.0, api=api(),
                                                     model=sensors.SensorModel(**MODEL)))
    if with_map:
        cam.attach_map(sensors.ElevationMap(size=32, source="clean", points=GRID), odometry=ODO)
    return cam


def train_cfg():
    from isaacgymloco_amd.learn.bench_train import train_cfg_dict
    tc = train_cfg_dict("aliengo")
    tc["runner"]["num_steps_per_env"] = T
    tc["algorithm"].update(num_learning_epochs=2, num_mini_batches=2)
    return tc


def build(case, seed=7):
    """(env, runner) of `case`, the env holding the runner's sensor as "depth" where the kind has one"""
    from isaacgymloco_amd.learn.depth_encoder import DepthEncoder
    from isaacgymloco_amd.learn.depth_memory import DepthMemory
    from isaacgymloco_amd.learn.distill import DistillRunner
    from isaacgymloco_amd.learn.map_policy import MapOnPolicyRunner
    from isaacgymloco_amd.learn.runner import HIMOnPolicyRunner
    from isaacgymloco_amd.learn.scan_policy import ScanOnPolicyRunner
    from isaacgymloco_amd.learn.vision import VisionOnPolicyRunner
    e = env()
    torch.manual_seed(seed)
    if case == "him":
        return e, HIMOnPolicyRunner(e, train_cfg(), device="cpu")
    if case == "scan":
        return e, ScanOnPolicyRunner(e, train_cfg(), device="cpu")
    if case == "map":
        return e, MapOnPolicyRunner(e, train_cfg(), sensor=camera(e, with_map=True), channels=("height", "known"), device="cpu")
    if case == "distill":
        teacher = ScanOnPolicyRunner(e, train_cfg(), device="cpu")
        return e, DistillRunner(e, train_cfg(), teacher=teacher, sensor=camera(e), encoder=DepthEncoder(12, 16, 2, **ENC), device="cpu")
    more = {"vision": {}, "vision_memory": {"memory": DepthMemory(L, 5, H)}, "vision_e2e": {"end_to_end": True}}[case]
    return e, VisionOnPolicyRunner(e, train_cfg(), sensor=camera(e), encoder=DepthEncoder(12, 16, 2, **ENC), device="cpu", **more)


def key_sets(d):
    """{"": top-level keys, record: its keys, record.sub: ...} of a checkpoint dict: the records a runner adds beside the reference's keys and
    the plain dicts inside them -- not a sensor's own record (envs/sensors.py's) and no state dict"""
    out = {"": sorted(d)}
    for name in ("vision", "map_policy", "scan_policy", "distill"):
        if name in d:
            out[name] = sorted(d[name])
            for sub, v in d[name].items():
                if isinstance(v, dict) and sub != "sensor" and not sub.endswith("state_dict"):
                    out[f"{name}.{sub}"] = sorted(v)
    return out
