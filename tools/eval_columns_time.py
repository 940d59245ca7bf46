#!/usr/bin/env python3
"""HIP-event times of the evaluator's columns launch (lsim_eval_columns_accumulate) and of the evaluation step of a vision policy.

    python tools/eval_columns_time.py --part launch   [--envs 4096] [--iters 200] [--rounds 5] [--out profiles/x.json]
    python tools/eval_columns_time.py --part evaluate [--envs 4096] [--steps 200] [--rounds 3]
    python tools/eval_columns_time.py --part him      [--envs 4096] [--steps 200] [--rounds 3]

`launch`: Aliengo on the default 10 x 20 terrain grid (200 groups by type x level), play_cfg, settled buffers after 30 steps of a seeded
untrained policy; per round, alternating, `iters` launches each of lsim_eval_accumulate, the columns launch with 2 columns and with 6.
`evaluate`: learn.evaluate.evaluate() per step for the HIM policy, for its vision twin (64 x 48 camera, period 5, staggered, 2 frames, default
encoder) without metrics and with both, alternating over the rounds.  `him`: the HIM case alone, written against the evaluator as it was
before the columns existed, so that the same file times an older tree.  Every figure: median, min and max over the rounds, microseconds.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from isaacgymloco_amd import abi  # noqa: E402
from isaacgymloco_amd.envs import config as C  # noqa: E402
from isaacgymloco_amd.envs.legged_robot import LeggedRobot  # noqa: E402
from isaacgymloco_amd.learn.evaluate import Evaluator, evaluate, play_cfg  # noqa: E402
from isaacgymloco_amd.learn.modules import HIMActorCritic  # noqa: E402

DEV = "cuda:0"


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


def spread(xs):
    return {"median_us": statistics.median(xs), "min_us": min(xs), "max_us": max(xs), "rounds": len(xs)}


def make_env(n, seed=1):
    cfg = play_cfg(C.aliengo_cfg())
    cfg.env.num_envs = n
    env = LeggedRobot(cfg, sim_device=DEV, seed=seed)
    env.reset()
    return env


def him_policy(env):
    torch.manual_seed(0)
    return HIMActorCritic(env.num_obs, env.num_privileged_obs, env.num_one_step_obs, env.num_actions).to(DEV)


def part_launch(a):
    env = make_env(a.envs)
    ac = him_policy(env)
    evs = {"eval_accumulate": Evaluator(env, group_by=("type", "level"))}
    for name, k in (("columns_2", 2), ("columns_6", 6)):
        evs[name] = Evaluator(env, group_by=("type", "level"))
        evs[name].add_columns([f"c{i}" for i in range(k)])
        evs[name].columns.copy_(torch.randn(a.envs, k, device=DEV))
    with torch.no_grad():
        for _ in range(30):
            env.step_device(ac.act_inference(env.get_observations()))
            for ev in evs.values():
                ev.accumulate()
    fns = {"eval_accumulate": evs["eval_accumulate"].accumulate, "columns_2": evs["columns_2"].accumulate_columns, "columns_6": evs["columns_6"].accumulate_columns}
    times = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            times[k].append(timed(fn, a.iters, 20))
    out = {k: spread(v) for k, v in times.items()}
    out["groups"] = evs["eval_accumulate"].num_groups
    out["groups_with_samples"] = int((evs["eval_accumulate"].table[:, 0] > 0).sum().item())
    return out


def time_evaluate(env, policy, ev, steps, **kw):
    ev.clear()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    evaluate(env, policy, steps, commands=(1.0, 0.0, 0.0), evaluator=ev, **kw)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / steps


def part_him(a):
    env = make_env(a.envs)
    ac = him_policy(env)
    ev = Evaluator(env, group_by=("type", "level"))
    time_evaluate(env, ac, ev, 20)
    return {"him": spread([time_evaluate(env, ac, ev, a.steps) for _ in range(a.rounds)])}


def part_evaluate(a):
    from isaacgymloco_amd.envs import sensors
    from isaacgymloco_amd.learn.depth_encoder import DepthEncoder
    from isaacgymloco_amd.learn.vision import VisionActorCritic
    env_h, env_v = make_env(a.envs), make_env(a.envs)
    cam = env_v.add_sensor("depth", sensors.depth_camera(env_v, 64, 48, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0,
                                                         model=sensors.SensorModel(period=5, stagger=True, latency=1, frames=2, normalise=True)))
    him = him_policy(env_h)
    torch.manual_seed(0)
    enc = DepthEncoder(48, 64, 2).to(DEV)
    vis = VisionActorCritic(env_v.num_obs, env_v.num_privileged_obs, env_v.num_one_step_obs, env_v.num_actions, depth_latent_dim=enc.latent_dim).to(DEV)
    head = torch.nn.Linear(enc.latent_dim, abi.DEFINES["LSIM_NUM_HEIGHT_PTS"]).to(DEV)
    cases = {"him": (env_h, him, Evaluator(env_h, group_by=("type", "level")), {}),
             "vision_no_metrics": (env_v, vis, Evaluator(env_v, group_by=("type", "level")), dict(sensor=cam, encoder=enc, vision_metrics=())),
             "vision_both_metrics": (env_v, vis, Evaluator(env_v, group_by=("type", "level")), dict(sensor=cam, encoder=enc, depth_head=head))}
    times = {k: [] for k in cases}
    for env, pol, ev, kw in cases.values():
        time_evaluate(env, pol, ev, 20, **kw)
    for _ in range(a.rounds):
        for k, (env, pol, ev, kw) in cases.items():
            times[k].append(time_evaluate(env, pol, ev, a.steps, **kw))
    out = {k: spread(v) for k, v in times.items()}
    out["columns"] = list(cases["vision_both_metrics"][2].column_names)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--part", required=True, choices=("launch", "evaluate", "him"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"tool": "eval_columns_time", "part": a.part, "num_envs": a.envs, "iters": a.iters, "steps": a.steps, "device": torch.cuda.get_device_name(0)}
    res.update({"launch": part_launch, "evaluate": part_evaluate, "him": part_him}[a.part](a))
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
