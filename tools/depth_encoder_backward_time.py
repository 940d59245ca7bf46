#!/usr/bin/env python3
"""HIP-event time and peak device memory of training the depth encoder through its fused launches (DepthEncoder.forward_device, whose backward
is lsim_depth_encode_backward) next to torch's own autograd through DepthEncoder.forward on the same device and frames.

    timeout -k 10 900 python tools/depth_encoder_backward_time.py [--rows 4096,minibatch] [--iters 100] [--warmup 10] [--out profiles/depth_encoder_backward_time.json]

One process; run it under a time limit of its own as above, and after a fault do not run it again before the cause is known.
The default DepthEncoder on a 64 x 48 camera with 2 frames, uniform random frames, at B = 4096 and at the rows of one minibatch of the default
Aliengo training configuration (num_envs * num_steps_per_env / num_mini_batches).  Per B, HIP events over `iters` repetitions after `warmup`:
  device_fwd_bwd_us   forward_device(frames).square().sum().backward()                       (1)
  torch_fwd_bwd_us    forward(frames).square().sum().backward(), torch's kernels             (2)
  device_fwd_us / backward_entry_us   lsim_depth_encode over the batch / lsim_depth_encode_backward alone (3), raw calls on fixed buffers
  *_peak_bytes        torch.cuda.max_memory_allocated over one repetition of (1) / (2), above what was allocated before it (frames, parameters)
  workspace_bytes, a1_bytes   what lsim_depth_encode_backward_sizes reports / what a buffer of a1's size would take at this B
and max_rel_diff, the largest |difference| / rms between the six gradients of (1) and (2).  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from isaacgymloco_amd import abi, lib  # noqa: E402
from isaacgymloco_amd.envs import config as C  # noqa: E402
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


def peak(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def minibatch_rows():
    env_cfg, train_cfg = (f() for f in C.TASKS["aliengo"][:2])
    return env_cfg.env.num_envs * train_cfg.runner.num_steps_per_env // train_cfg.algorithm.num_mini_batches


def measure(B, iters, warmup, dev):
    torch.manual_seed(0)
    enc = DepthEncoder(48, 64, 2).to(dev)
    frames = torch.rand(B, 2, 48, 64, device=dev)
    L = lib.load()
    res = {"rows": B}

    def clear():
        for p in enc.parameters():
            p.grad = None

    def device_step():
        clear()
        enc.forward_device(frames).square().sum().backward()

    def torch_step():
        clear()
        enc(frames).square().sum().backward()

    device_step()
    g_dev = [p.grad.clone() for p in enc.device_params()]
    torch_step()
    g_ref = [p.grad.clone() for p in enc.device_params()]
    res["max_rel_diff"] = max(float(((a - b).abs().max() / b.square().mean().sqrt()).item()) for a, b in zip(g_dev, g_ref))
    res["device_fwd_bwd_us"] = timed(device_step, iters, warmup)
    res["torch_fwd_bwd_us"] = timed(torch_step, iters, warmup)
    clear()
    res["device_peak_bytes"] = peak(device_step)
    clear()
    res["torch_peak_bytes"] = peak(torch_step)
    clear()
    # the two entries alone, on fixed buffers
    with torch.no_grad():
        latent = enc.forward_device(frames).contiguous()
        res["device_fwd_us"] = timed(lambda: enc.forward_device(frames), iters, warmup)
    g = 2.0 * latent
    db = abi.LsimDepthEncoderBwd()
    for k in ("height", "width", "frames", "c1", "k1", "s1", "c2", "k2", "s2", "latent_dim"):
        setattr(db, k, getattr(enc._extents, k))
    db.hist, db.hist_stride, db.hist_slots, db.batch, db.final_act = frames.data_ptr(), 48 * 64, 2, B, 1
    db.g, db.g_stride, db.latent, db.latent_stride = g.data_ptr(), g.stride(0), latent.data_ptr(), latent.stride(0)
    lds, need = ctypes.c_size_t(), ctypes.c_size_t()
    lib.check(L.lsim_depth_encode_backward_sizes(ctypes.byref(db), ctypes.byref(lds), ctypes.byref(need)), what="lsim_depth_encode_backward_sizes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    outs = [torch.empty_like(p) for p in enc.device_params()]
    for name, p, o in zip(("w1", "b1", "w2", "b2", "w3", "b3"), enc.device_params(), outs):
        setattr(db, name, p.data_ptr())
        setattr(db, "g" + name, o.data_ptr())
    db.workspace, db.workspace_bytes = ws.data_ptr(), need.value
    stream = torch.cuda.current_stream().cuda_stream
    res["backward_entry_us"] = timed(lambda: lib.check(L.lsim_depth_encode_backward(ctypes.byref(db), stream), what="lsim_depth_encode_backward"), iters, warmup)
    res["backward_lds_bytes"], res["workspace_bytes"] = lds.value, need.value
    res["a1_bytes"] = 4 * B * 16 * 22 * 30
    res["torch_over_device"] = res["torch_fwd_bwd_us"] / res["device_fwd_bwd_us"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", default="4096,minibatch")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    rows = [minibatch_rows() if r == "minibatch" else int(r) for r in a.rows.split(",")]
    res = {"tool": "depth_encoder_backward_time", "device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "image": [48, 64], "frames": 2,
           "network": "c1=16 k1=5 s1=2, c2=32 k2=3 s2=2, latent 64", "minibatch_rows": minibatch_rows(), "runs": [measure(B, a.iters, a.warmup, dev) for B in rows]}
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
