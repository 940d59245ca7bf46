#!/usr/bin/env python3
"""HIP-event time of the evaluator launch (lsim_eval_accumulate), alone and inside the evaluation step.

    python tools/eval_time.py [--sizes 4096,262144] [--terrains flat,stairs] [--iters 200] [--warmup 20] [--out profiles/eval_time.json]

Per (size, terrain), Aliengo + Go2 half and half, untrained seeded policy, play_cfg: `accumulate_us` = the launch alone on settled buffers;
`step_us` / `step_eval_us` = {lsim_policy_forward + lsim_step} without / with it; `kernel_a_us` = kernel A from the library's own events
(lsim_read_profile) in the same process; `torch_ops_us` = the same sums with torch index_add_ ops on the same buffers (what the launch
replaces).  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from isaacgymloco_amd.envs import config as C  # noqa: E402
from isaacgymloco_amd.envs.legged_robot import LeggedRobot  # noqa: E402
from isaacgymloco_amd.learn.evaluate import Evaluator, play_cfg  # noqa: E402
from isaacgymloco_amd.learn.fused_policy import PackedHimPolicy  # noqa: E402
from isaacgymloco_amd.learn.modules import HIMActorCritic  # noqa: E402


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


def torch_ops(env, ev, acc):
    """the step sample of lsim.h with torch ops: float index_add_ per metric into acc [groups, 8] (order-dependent sums)"""
    live = ~env.reset_buf
    g = (ev._const.get("robot_ids", torch.zeros_like(env.terrain_types)).long() * ev.num_types + env.terrain_types) * ev.num_levels + env.terrain_levels
    d = env.commands[:, :2] - env.base_lin_vel[:, :2]
    e2 = (d * d).sum(1)
    yaw = (env.commands[:, 2] - env.base_ang_vel[:, 2]).abs()
    tau = env.torques
    cols = torch.stack((live.float(), e2.sqrt(), e2, yaw, yaw * yaw, (tau * env.dof_vel).abs().sum(1), (tau * tau).sum(1),
                        ((env.actions - env.last_actions) ** 2).sum(1)), dim=1) * live.unsqueeze(1)
    acc.index_add_(0, g, cols)


def measure(n, terrain, iters, warmup):
    cfg = play_cfg(C.mixed_cfg("aliengo", {"aliengo": 0.5, "go2": 0.5})[0])
    cfg.env.num_envs = n
    cfg.terrain.terrain_proportions = [1.0, 0.0, 0.0, 0.0, 0.0, 0.0] if terrain == "flat" else [0.0, 0.0, 0.0, 0.0, 0.5, 0.5]
    env = LeggedRobot(cfg, sim_device="cuda:0", seed=1)
    env.reset()
    torch.manual_seed(0)
    ac = HIMActorCritic(env.num_obs, env.num_privileged_obs, env.num_one_step_obs, env.num_actions).to("cuda:0")
    packed = PackedHimPolicy(ac)
    mean, values = torch.empty(n, 12, device="cuda:0"), torch.empty(n, 1, device="cuda:0")
    ev = Evaluator(env, trace_envs=(0, 1), trace_capacity=64)

    def step():
        packed.forward(env.obs_buf, env.privileged_obs_buf, mean, values)
        env.step_device(mean)

    def step_eval():
        step()
        ev.accumulate()

    L = env._L
    out = {"num_envs": n, "terrain": terrain, "groups": ev.num_groups}
    out["step_us"] = timed(step, iters, warmup)
    L.lsim_set_profiling(env._h, iters)
    timed(step_eval, iters, 0)
    ms_a, ms_b, cnt = (ctypes.c_float * iters)(), (ctypes.c_float * iters)(), ctypes.c_int(iters)
    L.lsim_read_profile(env._h, ms_a, ms_b, ctypes.byref(cnt))
    L.lsim_set_profiling(env._h, 0)
    out["kernel_a_us"] = 1000.0 * sum(ms_a[:cnt.value]) / max(cnt.value, 1)
    out["step_eval_us"] = timed(step_eval, iters, warmup)
    out["accumulate_us"] = timed(ev.accumulate, iters, warmup)
    acc = torch.zeros(ev.num_groups, 8, device="cuda:0")
    out["torch_ops_us"] = timed(lambda: torch_ops(env, ev, acc), iters, warmup)
    out["accumulate_over_kernel_a"] = out["accumulate_us"] / out["kernel_a_us"]
    out["torch_ops_over_accumulate"] = out["torch_ops_us"] / out["accumulate_us"]
    out["nonfinite_addends"] = int(ev.table[:, 17].sum().item())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default="4096,262144")
    ap.add_argument("--terrains", default="flat,stairs")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"tool": "eval_time", "iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "cases": [measure(int(n), t, a.iters, a.warmup) for n in a.sizes.split(",") for t in a.terrains.split(",")]}
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
