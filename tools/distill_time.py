"""Times of vision distillation (learn/distill.py) at a user's shapes: the labelling pass, one lsim_distill_loss launch and
the whole distillation update, and -- as context, no pass bar -- the update of VisionOnPolicyRunner(end_to_end=True) on the same shapes.

    python tools/distill_time.py [--envs 4096] [--steps 24] [--iters 6] [--warmup 2] [--skip-distill] [--out profiles/distill_time.json]

--skip-distill measures the end-to-end PPO update alone and needs nothing of this feature: it runs unchanged on a checkout of the commit
before it, which is how the "parent" entry of profiles/distill_time.json was taken (same machine, same call).

Wall clock around device synchronisations for the updates (the runner's own last_perf); HIP events for the labelling pass inside the
update and for a train of lsim_distill_loss launches on the update's own minibatch shape."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

DEV = "cuda:0"


def make_env(a, seed=1):
    from isaacgymloco_amd.envs import config as C, sensors
    from isaacgymloco_amd.envs.legged_robot import LeggedRobot
    cfg = C.aliengo_cfg()
    cfg.env.num_envs = a.envs
    env = LeggedRobot(cfg, sim_device=DEV, seed=seed)
    env.add_sensor("depth", sensors.depth_camera(env, a.width, a.height, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0,
                                                 model=sensors.SensorModel(period=5, stagger=True, latency=1, frames=2, normalise=True)))
    return env


def train_cfg(a):
    from isaacgymloco_amd.learn.bench_train import train_cfg_dict
    tc = train_cfg_dict("aliengo")
    tc["runner"]["num_steps_per_env"] = a.steps
    return tc


def med(v):
    return sorted(v)[len(v) // 2]


def iterate(run, a):
    rows = []
    for it in range(a.warmup + a.iters):
        run.learn(1)
        if it >= a.warmup:
            rows.append((run.last_perf["collection_time"], run.last_perf["learn_time"]))
    torch.cuda.synchronize()
    return {"collection_s": med([r[0] for r in rows]), "update_s": med([r[1] for r in rows]), "iterations": len(rows),
            "collection_s_all": [r[0] for r in rows], "update_s_all": [r[1] for r in rows]}


def measure_e2e(a):
    from isaacgymloco_amd.learn.vision import VisionOnPolicyRunner
    torch.manual_seed(0)
    run = VisionOnPolicyRunner(make_env(a), train_cfg(a), sensor="depth", device=DEV, end_to_end=True)
    assert run.enable_graphs()
    out = iterate(run, a)
    out.update(minibatches=run.alg.num_learning_epochs * run.alg.num_mini_batches, e2e_minibatches=run.alg.e2e_epochs * run.alg.num_mini_batches)
    del run
    torch.cuda.empty_cache()
    return out


def measure_distill(a):
    import ctypes
    from isaacgymloco_amd import abi, lib
    from isaacgymloco_amd.learn.distill import DistillRunner
    from isaacgymloco_amd.learn.scan_policy import ScanOnPolicyRunner
    torch.manual_seed(0)
    teacher = ScanOnPolicyRunner(make_env(a, seed=2), train_cfg(a), device=DEV)     # untrained: the times do not depend on its weights
    with torch.no_grad():
        w = teacher.alg.actor_critic.actor[0].weight
        w[:, -187:] = 0.05 * torch.randn(w.shape[0], 187, device=DEV)
    run = DistillRunner(make_env(a), train_cfg(a), teacher=teacher, sensor="depth", device=DEV)
    del teacher
    assert run.enable_graphs()
    alg = run.alg
    label_ms, label = [], alg.label_rollout

    def timed_label():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = label(); e1.record()
        label_ms.append((e0, e1))
        return out
    alg.label_rollout = timed_label
    out = iterate(run, a)
    out["label_s"] = med([e0.elapsed_time(e1) * 1e-3 for e0, e1 in label_ms[a.warmup:]])
    out.update(distill_loss=alg.last_distill_loss, minibatches=alg.distill_epochs * alg.num_mini_batches, logged_images=int(alg._e2e_rows),
               transitions=a.steps * a.envs, label_rows=int(alg.teacher_means.shape[0]))
    # one lsim_distill_loss launch on the update's minibatch shape: a train of launches between two events, after a warm-up
    B, A = a.steps * a.envs // alg.num_mini_batches, run.env.num_actions
    mu, g = torch.randn(B, A, device=DEV), torch.empty(B, A, device=DEV)
    index = torch.randperm(a.steps * a.envs, device=DEV)[:B].to(torch.int32)
    partial = torch.empty(abi.DEFINES["LSIM_DISTILL_PARTIALS"], device=DEV)
    dl = abi.LsimDistillLoss()
    dl.mu, dl.target, dl.index, dl.g, dl.partial = mu.data_ptr(), alg.teacher_means.data_ptr(), index.data_ptr(), g.data_ptr(), partial.data_ptr()
    dl.batch, dl.actions, dl.target_rows, dl.mu_stride, dl.target_stride, dl.g_stride, dl.scale = B, A, alg.teacher_means.shape[0], A, A, A, 2.0 / (B * A)
    L, s = lib.load(), torch.cuda.current_stream().cuda_stream
    for _ in range(20):
        lib.check(L.lsim_distill_loss(ctypes.byref(dl), s))
    trains = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            L.lsim_distill_loss(ctypes.byref(dl), s)
        e1.record()
        torch.cuda.synchronize()
        trains.append(e0.elapsed_time(e1) * 1e-3 / a.launches)
    out.update(distill_loss_launch_s=med(trains), distill_loss_launch_s_all=trains, launches_per_train=a.launches, minibatch_rows=B,
               distill_loss_bytes=B * A * 4 * 3 + B * 4)
    del run
    torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--height", type=int, default=48)
    ap.add_argument("--steps", type=int, default=24, help="env steps per rollout")
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=200, help="lsim_distill_loss launches per timed train")
    ap.add_argument("--skip-distill", action="store_true", help="only the end-to-end PPO update (runs on a checkout without this feature)")
    ap.add_argument("--parent", default=None, help="a JSON file written with --skip-distill on the commit before this feature: copied into the result as 'parent'")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "distill_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("distill_time.py needs a GPU: there is no CPU form of this measurement")
    res = {"what": "seconds, medians over the iterations: label_s = the labelling pass (one lsim_policy_forward_ext over all stored transitions, inside "
                   "update_s), distill_loss_launch_s = one lsim_distill_loss launch in a train of back-to-back launches, update_s = the whole update; "
                   "e2e_ppo = VisionOnPolicyRunner(end_to_end=True) on the same shapes in this tree, parent = the same at the commit before the feature",
           "num_envs": a.envs, "steps": a.steps, "camera": [a.width, a.height, "period 5"], "device": torch.cuda.get_device_name(0)}
    res["e2e_ppo"] = measure_e2e(a)
    if not a.skip_distill:
        res["distill"] = measure_distill(a)
    if a.parent:
        res["parent"] = json.load(open(a.parent))["e2e_ppo"]
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
