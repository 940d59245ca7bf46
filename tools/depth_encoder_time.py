#!/usr/bin/env python3
"""HIP-event time of the depth-encoder launch (lsim_depth_encode) next to the torch forward it stands in for.

    timeout -k 10 600 python tools/depth_encoder_time.py [--num-envs 4096] [--iters 100] [--warmup 10] [--out profiles/depth_encoder_time.json]

One process; run it under a time limit of its own as above, and after a fault do not run it again before the cause is known.
N envs (Aliengo on the default terrain), a 64 x 48 depth camera with SensorModel(period=5, stagger=True, latency=1, frames=2, normalise=True),
the default DepthEncoder.  HIP events over `iters` launches each:
  encode_all_us        lsim_depth_encode with every env due (LSIM_SENSOR_FILL_ALL)
  encode_staggered_us  lsim_depth_encode at period 5 staggered, the tick advancing by one per launch: 1 env in 5 is due
  torch_forward_us     DepthEncoder.forward on sensor.frame_images() under torch.no_grad() on the same device: the baseline, torch's own kernels
                       (torch_forward_contiguous_us: the same on a contiguous copy made outside the timed region)
  capture_all_us / capture_staggered_us   lsim_sensor_capture alone, for scale
  kernel_a_us          kernel A from the library's own events (lsim_read_profile), for scale
and max_abs_diff, the largest difference between the launch and the torch forward on the same frames.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from isaacgymloco_amd import abi  # noqa: E402
from isaacgymloco_amd.envs import config as C, sensors  # noqa: E402
from isaacgymloco_amd.envs.legged_robot import LeggedRobot  # noqa: E402
from isaacgymloco_amd.learn.depth_encoder import DepthEncoder  # noqa: E402


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, dev = a.num_envs, "cuda:0"
    cfg = C.TASKS["aliengo"][0]()
    cfg.env.num_envs = n
    env = LeggedRobot(cfg, sim_device=dev, seed=1)
    env.reset()
    model = sensors.SensorModel(period=5, stagger=True, latency=1, frames=2, normalise=True)
    cam = env.add_sensor("depth", sensors.depth_camera(env, 64, 48, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, near=0.05, far=5.0, model=model))
    torch.manual_seed(0)
    enc = DepthEncoder(48, 64, 2).to(dev)
    fill = abi.DEFINES["LSIM_SENSOR_FILL_ALL"]
    res = {"tool": "depth_encoder_time", "device": torch.cuda.get_device_name(0), "num_envs": n, "iters": a.iters, "warmup": a.warmup,
           "image": [48, 64], "frames": 2, "network": "c1=16 k1=5 s1=2, c2=32 k2=3 s2=2, latent 64", "lds_bytes": enc.lds_bytes(env._L)}
    actions = torch.zeros(n, 12, device=dev)
    for _ in range(3):                              # episode_length > 0 everywhere: the staggered launches see no reset env
        env.step_device(actions)
    tick = [int(env.common_step_counter)]

    def staggered(fn):
        def run():
            tick[0] += 1
            fn(tick[0])
        return run

    res["capture_all_us"] = timed(lambda: cam.update(tick=tick[0], flags=fill), a.iters, a.warmup)
    res["capture_staggered_us"] = timed(staggered(lambda t: cam.update(tick=t)), a.iters, a.warmup)
    cam.refresh(tick=tick[0])
    res["encode_all_us"] = timed(lambda: enc.encode_device(cam, tick[0], fill), a.iters, a.warmup)
    res["encode_staggered_us"] = timed(staggered(lambda t: enc.encode_device(cam, t)), a.iters, a.warmup)
    z = enc.encode_device(cam, tick[0], fill)
    x = cam.frame_images()
    xc = x.contiguous()
    with torch.no_grad():
        res["torch_forward_us"] = timed(lambda: enc(x), a.iters, a.warmup)
        res["torch_forward_contiguous_us"] = timed(lambda: enc(xc), a.iters, a.warmup)
        res["max_abs_diff"] = float((enc(x) - z).abs().max().item())
    L = env._L
    L.lsim_set_profiling(env._h, a.iters)
    timed(lambda: env.step_device(actions), a.iters, 0)
    ms_a, ms_b, cnt = (ctypes.c_float * a.iters)(), (ctypes.c_float * a.iters)(), ctypes.c_int(a.iters)
    L.lsim_read_profile(env._h, ms_a, ms_b, ctypes.byref(cnt))
    L.lsim_set_profiling(env._h, 0)
    res["kernel_a_us"] = 1000.0 * sum(ms_a[:cnt.value]) / max(cnt.value, 1)
    res["torch_over_encode_all"] = res["torch_forward_us"] / res["encode_all_us"]
    res["encode_all_over_staggered"] = res["encode_all_us"] / res["encode_staggered_us"]
    res["nonfinite_rays"] = int(cam.nonfinite_rays)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
