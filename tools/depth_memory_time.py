#!/usr/bin/env python3
"""HIP-event time of the depth-memory launches next to what they stand beside or in for.

    timeout -k 10 600 python tools/depth_memory_time.py [--num-envs 4096] [--samples 9] [--out profiles/depth_memory_time.json]

One process; run it under a time limit of its own as above, and after a fault do not run it again before the cause is known.
Samples ALTERNATE between the variants of a comparison (A B A B ...), each sample a HIP-event pair around `--repeat` back-to-back calls, and
the median per variant is reported with the smallest and largest sample, so clock drift and a busy neighbour fall on both sides alike.
  step_us / kernel_a_us          lsim_depth_memory_step at N envs (L = 64, P = 45, H = 64) on an Aliengo env with the default camera and
                                 encoder attached, next to kernel A from the library's own events (lsim_read_profile)
  sequence[n].device_ms          DepthMemory.sequence_device forward + backward (input GEMM, the two serial kernels, the parameter-gradient
                                 GEMMs) at T = 99 and n = 1024, 4096;  .forward_kernel_ms / .backward_kernel_ms the serial kernels alone
  sequence[n].torch_loop_ms      the same forward + backward through DepthMemory.sequence (the nn.GRUCell loop under autograd) on the device
  sequence[n].saved_bytes        what the forward keeps for the backward (hs + save = 5 H floats per row) next to the 4 H of save alone
Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from isaacgymloco_amd import abi, lib  # noqa: E402
from isaacgymloco_amd.learn.depth_memory import DepthMemory  # noqa: E402

DEV = "cuda:0"


def alternate(fns, samples, repeat, warmup=2):
    """{name: (median, min, max)} in ms per call; the variants take turns sample by sample"""
    out = {k: [] for k in fns}
    for k, fn in fns.items():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(samples):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(repeat):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[k].append(a.elapsed_time(b) / repeat)
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in out.items()}


def step_time(n, samples):
    from isaacgymloco_amd.envs import config as C, sensors
    from isaacgymloco_amd.envs.legged_robot import LeggedRobot
    from isaacgymloco_amd.learn.depth_encoder import DepthEncoder
    cfg = C.TASKS["aliengo"][0]()
    cfg.env.num_envs = n
    env = LeggedRobot(cfg, sim_device=DEV, seed=1)
    env.reset()
    model = sensors.SensorModel(period=5, stagger=True, latency=1, frames=2, normalise=True)
    cam = env.add_sensor("depth", sensors.depth_camera(env, 64, 48, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, model=model))
    torch.manual_seed(0)
    cam.attach_encoder(DepthEncoder(48, 64, 2).to(DEV))
    mem = DepthMemory(64, env.num_one_step_obs, 64).to(DEV)
    actions = torch.zeros(n, 12, device=DEV)
    iters = 50
    L = env._L

    def kernel_a():
        L.lsim_set_profiling(env._h, iters)
        for _ in range(iters):
            env.step_device(actions)
        torch.cuda.synchronize()
        ms_a, ms_b, cnt = (ctypes.c_float * iters)(), (ctypes.c_float * iters)(), ctypes.c_int(iters)
        L.lsim_read_profile(env._h, ms_a, ms_b, ctypes.byref(cnt))
        L.lsim_set_profiling(env._h, 0)
        return 1000.0 * sorted(ms_a[:cnt.value])[cnt.value // 2]
    a_before = kernel_a()                               # without the memory attached
    cam.attach_memory(mem)                              # h and the rows are the sensor's; steps every env once from h = 0
    t = alternate({"step": lambda: mem.step_device(cam), "encode_staggered": lambda: cam.stage("encoder").launch(1, 0)}, samples, iters)
    a_after = kernel_a()
    return {"num_envs": n, "cell": {"latent_dim": 64, "proprio_dim": env.num_one_step_obs, "hidden": 64}, "lds_bytes": list(mem.lds_bytes(L)),
            "step_us": [1000.0 * v for v in t["step"]], "encode_staggered_us": [1000.0 * v for v in t["encode_staggered"]],
            "kernel_a_us": [a_before, a_after], "step_over_kernel_a": 1000.0 * t["step"][0] / a_after}


def sequence_time(n, T, samples):
    torch.manual_seed(1)
    mem = DepthMemory(64, 45, 64).to(DEV)
    x = torch.randn(T, n, 109, device=DEV)
    h0 = 0.3 * torch.randn(n, 64, device=DEV)
    reset = (torch.rand(T, n, device=DEV) < 0.01).to(torch.uint8)
    head = torch.randn(T, n, 64, device=DEV)
    Lb = lib.load()

    def both(fn):
        def run():
            mem.zero_grad(set_to_none=True)
            (fn(x, h0, reset) * head).sum().backward()
        return run
    # the serial kernels alone, on buffers of their own
    gi = torch.randn(T, n, 192, device=DEV)
    hs, save = torch.empty(T, n, 64, device=DEV), torch.empty(T, n, 256, device=DEV)
    dgi, dghn, dh0 = torch.empty(T, n, 192, device=DEV), torch.empty(T, n, 64, device=DEV), torch.empty(n, 64, device=DEV)
    gs = abi.STRUCTS["lsim_gru_sequence_t"]()
    gs.gi, gs.h0, gs.reset, gs.weight_hh, gs.bias_hh = gi.data_ptr(), h0.data_ptr(), reset.data_ptr(), mem.cell.weight_hh.data_ptr(), mem.cell.bias_hh.data_ptr()
    gs.hs, gs.save, gs.dhs, gs.dgi, gs.dghn, gs.dh0 = hs.data_ptr(), save.data_ptr(), head.data_ptr(), dgi.data_ptr(), dghn.data_ptr(), dh0.data_ptr()
    gs.steps, gs.num_envs, gs.hidden = T, n, 64
    stream = lambda: torch.cuda.current_stream().cuda_stream
    t = alternate({"device": both(mem.sequence_device), "torch_loop": both(mem.sequence),
                   "forward_kernel": lambda: lib.check(Lb.lsim_gru_sequence_forward(ctypes.byref(gs), stream())),
                   "backward_kernel": lambda: lib.check(Lb.lsim_gru_sequence_backward(ctypes.byref(gs), stream()))}, samples, 1)
    mem.zero_grad(set_to_none=True)
    (mem.sequence_device(x, h0, reset) * head).sum().backward()
    g_dev = [p.grad.clone() for p in mem.parameters()]
    mem.zero_grad(set_to_none=True)
    (mem.sequence(x, h0, reset) * head).sum().backward()
    diff = max(float((a - p.grad).abs().max() / p.grad.abs().max()) for a, p in zip(g_dev, mem.parameters()))
    out = {"n": n, "T": T, "workgroups": (n + 15) // 16, "saved_bytes": 4 * T * n * 5 * 64, "save_bytes": 4 * T * n * 4 * 64,
           "max_relative_gradient_difference": diff}
    out.update({k + "_ms": list(v) for k, v in t.items()})
    out["forward_us_per_step"] = 1000.0 * t["forward_kernel"][0] / T
    out["backward_us_per_step"] = 1000.0 * t["backward_kernel"][0] / T
    out["torch_loop_over_device"] = t["torch_loop"][0] / t["device"][0]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=99)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("depth_memory_time.py needs a GPU: there is no CPU form of this measurement")
    res = {"tool": "depth_memory_time", "device": torch.cuda.get_device_name(0), "samples": a.samples,
           "what": "[median, min, max] over alternating samples", "step": step_time(a.num_envs, a.samples),
           "sequence": [sequence_time(n, a.steps, a.samples) for n in sorted({min(1024, a.num_envs), a.num_envs})]}
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
