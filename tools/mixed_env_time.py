"""The environment step alone on a mixed-robot instance (config.mixed_cfg), for kernel-A timing under rocprofv3 --kernel-trace --stats.
The loop is bench.py --mode env's: reset, episode lengths spread, N(0,1) actions, warm-up steps, then timed LeggedRobot.step_device calls.
usage: python tools/mixed_env_time.py --robots aliengo=0.5,go2=0.5 [--task aliengo] [--envs 4096] [--steps 200] [--warmup 50]
       (--robots go2=1 times one robot through the same path; prints one JSON line: wall time per step and the kernel-A / B means)"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from isaacgymloco_amd.envs import config as C  # noqa: E402
from isaacgymloco_amd.envs.legged_robot import LeggedRobot  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", default="aliengo=0.5,go2=0.5", help="name=fraction,... (single-robot task names)")
    ap.add_argument("--task", default="aliengo", help="base task: everything outside the robot-specific set")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    args = ap.parse_args()
    robots = {k: float(v) for k, v in (item.split("=") for item in args.robots.split(","))}
    cfg, _ = C.mixed_cfg(args.task, robots)
    cfg.env.num_envs = N = args.envs
    dev = torch.device("cuda:0")
    env = LeggedRobot(cfg, sim_device="cuda:0", seed=1)
    env.reset()
    env.episode_length_buf = torch.randint_like(env.episode_length_buf, high=int(env.max_episode_length))
    g = torch.Generator(device=dev).manual_seed(1)
    acts = [torch.randn(N, 12, device=dev, generator=g) for _ in range(16)]
    for i in range(args.warmup):
        env.step_device(acts[i % 16])
    env._L.lsim_set_profiling(env._h, args.steps)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(args.steps):
        env.step_device(acts[i % 16])
    torch.cuda.synchronize(dev)
    elapsed = time.perf_counter() - t0
    K = args.steps
    ms_a, ms_b, n = (ctypes.c_float * K)(), (ctypes.c_float * K)(), ctypes.c_int(K)
    env._L.lsim_read_profile(env._h, ms_a, ms_b, ctypes.byref(n))
    print(json.dumps({"robots": robots, "envs": N, "steps": K, "ms_per_step": 1e3 * elapsed / K,
                      "kernel_a_ms": sum(ms_a[i] for i in range(n.value)) / max(n.value, 1),
                      "kernel_b_ms": sum(ms_b[i] for i in range(n.value)) / max(n.value, 1),
                      "nonfinite_envs": int(env.nonfinite_envs)}))
    env.close()


if __name__ == "__main__":
    main()
