"""Time of the fused rollout-time policy launch (include/lsim.h, lsim_policy_forward) at N = 4096, HIP events.

    python tools/policy_time.py            # the plain launch, one line
    python tools/policy_time.py --ext      # the launch with the extra actor-input segment (L = 64, learn/vision.py) against the plain launch in
                                           # the same process, alternating, forward and act forms -> profiles/policy_ext_time.json"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from isaacgymloco_amd.learn.modules import HIMActorCritic
from isaacgymloco_amd.learn.fused_policy import PackedHimPolicy
N = 4096
DEV = "cuda:0"


def timed(fn, reps):
    """microseconds per call: HIP events around `reps` calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def plain():
    torch.manual_seed(0)
    ac = HIMActorCritic(270, 238, 45, 12).to(DEV)
    pk = PackedHimPolicy(ac)
    obs, priv = torch.randn(N, 270, device=DEV), torch.randn(N, 238, device=DEV)
    mean, val = torch.empty(N, 12, device=DEV), torch.empty(N, 1, device=DEV)
    for _ in range(30): pk.forward(obs, priv, mean, val)
    torch.cuda.synchronize()
    print("policy forward us:", timed(lambda: pk.forward(obs, priv, mean, val), 200))


def ext(L, reps, rounds, out):
    from isaacgymloco_amd.learn.storage import HIMRolloutStorage
    from isaacgymloco_amd.learn.vision import PackedVisionPolicy, VisionActorCritic
    torch.manual_seed(0)
    him = HIMActorCritic(270, 238, 45, 12).to(DEV)
    vis = VisionActorCritic(270, 238, 45, 12, depth_latent_dim=L).to(DEV)
    pk_h, pk_v = PackedHimPolicy(him), PackedVisionPolicy(vis)
    obs, priv, rows = torch.randn(N, 270, device=DEV), torch.randn(N, 238, device=DEV), torch.randn(N, L, device=DEV)
    std = torch.ones(12, device=DEV)
    mean, val, act = torch.empty(N, 12, device=DEV), torch.empty(N, 1, device=DEV), torch.empty(N, 12, device=DEV)
    T = 4
    S = HIMRolloutStorage(N, T, [270], [238], [12], DEV).c_struct()
    store = torch.zeros(T, N, L, device=DEV)
    calls = {"forward_plain": lambda: pk_h.forward(obs, priv, mean, val),
             "forward_ext": lambda: pk_v.forward(obs, priv, mean, val, rows=rows),
             "act_plain": lambda: pk_h.forward_act(S, 1, 0, obs, priv, std, 1, 0, mean, val, act),
             "act_ext": lambda: pk_v.forward_act(S, 1, 0, obs, priv, std, 1, 0, mean, val, act, rows=rows, store=store)}
    for fn in calls.values():
        for _ in range(30): fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in calls}
    for _ in range(rounds):                 # alternate the four, so that a drift of the clocks lands on all of them
        for k, fn in calls.items():
            samples[k].append(timed(fn, reps))
    med = {k: sorted(v)[len(v) // 2] for k, v in samples.items()}
    res = {"what": "lsim_policy_forward_ext / lsim_policy_act_post_at_ext against the plain launches, same process, HIP events", "num_envs": N,
           "extra_dim": L, "reps_per_sample": reps, "rounds": rounds, "device": torch.cuda.get_device_name(0),
           "median_us": med, "min_us": {k: min(v) for k, v in samples.items()}, "max_us": {k: max(v) for k, v in samples.items()},
           "ext_over_plain": {"forward": med["forward_ext"] / med["forward_plain"], "act": med["act_ext"] / med["act_plain"]}}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ext", action="store_true", help="time the launch with the extra actor-input segment against the plain one")
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "policy_ext_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("policy_time.py needs a GPU: there is no CPU form of this measurement")
    ext(a.dim, a.reps, a.rounds, a.out) if a.ext else plain()
