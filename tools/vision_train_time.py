"""Collection and update time per iteration of VisionOnPolicyRunner next to HIMOnPolicyRunner on the same env configuration, both with the
depth camera attached (the HIM runner merely does not read it), and the encoder's own step separately.

    python tools/vision_train_time.py [--envs 4096] [--steps T] [--iters 6] [--warmup 2] [--memory] [--e2e] [--mount-jitter POS,ROT_DEG] [--instrument RANGES] [--out profiles/vision_train_time.json]

--e2e: also the vision runner with end_to_end=True (the PPO gradient into the encoder): collection and update time, the
frame log's launches per iteration with HIP events, the logged images and the log's bytes.

Wall clock around device synchronisations, as the runners' own last_perf; the encoder step with HIP events inside VisionPPO.update()."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

DEV = "cuda:0"
VISION_KINDS = ("vision", "vision_jitter", "vision_instrument", "memory", "e2e")


def make(kind, a):
    from isaacgymloco_amd.envs import config as C, sensors
    from isaacgymloco_amd.envs.legged_robot import LeggedRobot
    from isaacgymloco_amd.learn.bench_train import train_cfg_dict
    from isaacgymloco_amd.learn.runner import HIMOnPolicyRunner
    from isaacgymloco_amd.learn.vision import VisionOnPolicyRunner
    cfg = C.aliengo_cfg()
    cfg.env.num_envs = a.envs
    env = LeggedRobot(cfg, sim_device=DEV, seed=1)
    cam = env.add_sensor("depth", sensors.depth_camera(env, a.width, a.height, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0,
                                                       model=sensors.SensorModel(period=5, stagger=True, latency=1, frames=2, normalise=True),
                                                       mount_jitter=a.jitter if kind == "vision_jitter" else None,
                                                       instrument=a.inst if kind == "vision_instrument" else None))
    tc = train_cfg_dict("aliengo")
    if a.steps:
        tc["runner"]["num_steps_per_env"] = a.steps
    torch.manual_seed(0)
    if kind in VISION_KINDS:
        run = VisionOnPolicyRunner(env, tc, sensor="depth", device=DEV, memory=True if kind == "memory" else None, end_to_end=kind == "e2e")
    else:
        from isaacgymloco_amd.learn.depth_encoder import DepthEncoder
        cam.attach_encoder(DepthEncoder(a.height, a.width, 2).to(DEV))      # the same launches per step; nobody reads the latent
        run = HIMOnPolicyRunner(env, tc, log_dir=None, device=DEV)
    assert run.enable_graphs()
    return run


def measure(kind, a):
    run = make(kind, a)
    enc_ms, mem_ms = [], []
    if kind == "memory":
        mstep = run.alg.memory_step

        def timed_memory_step():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); out = mstep(); e1.record()
            mem_ms.append((e0, e1))
            return out
        run.alg.memory_step = timed_memory_step
    log_ms = []
    if kind == "e2e":
        stage = run.sensor.stage("frames_log")
        launch = stage.launch

        def timed_launch(tick, flags, stream=None):
            if stage.step is None:
                return launch(tick, flags, stream)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); out = launch(tick, flags, stream); e1.record()
            log_ms.append((e0, e1))
            return out
        stage.launch = timed_launch
    if kind in VISION_KINDS:
        alg, step = run.alg, run.alg.encoder_step

        def timed_step():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); out = step(); e1.record()
            enc_ms.append((e0, e1))
            return out
        alg.encoder_step = timed_step
    rows = []
    for it in range(a.warmup + a.iters):
        run.learn(1)
        if it >= a.warmup:
            rows.append((run.last_perf["collection_time"], run.last_perf["learn_time"]))
    torch.cuda.synchronize()
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"collection_s": med([r[0] for r in rows]), "update_s": med([r[1] for r in rows]), "iterations": len(rows),
           "collection_s_all": [r[0] for r in rows], "update_s_all": [r[1] for r in rows]}
    if enc_ms:
        out["encoder_step_s"] = med([e0.elapsed_time(e1) * 1e-3 for e0, e1 in enc_ms[a.warmup:]])
        out["aux_loss"] = run.alg.last_aux_loss
    if log_ms:
        T = run.num_steps_per_env           # per rollout: the FILL_ALL launch of its start, then one behind every env step but the last
        per_it = [sum(e0.elapsed_time(e1) for e0, e1 in log_ms[i * T:(i + 1) * T]) * 1e-3 for i in range(a.warmup, a.warmup + a.iters)]
        first = [log_ms[i * T][0].elapsed_time(log_ms[i * T][1]) * 1e-3 for i in range(a.warmup, a.warmup + a.iters)]
        cam = run.sensor
        out.update(frames_log_s=med(per_it), frames_log_start_s=med(first), logged_images=int(cam.frames_log_state()[0]),
                   log_overflow=int(run.alg.last_e2e_overflow), log_capacity=int(cam.frames_log().shape[0]),
                   log_bytes=int(cam.frames_log().numel() * 4), e2e_epochs=run.alg.e2e_epochs, transitions=T * a.envs)
    if mem_ms:
        out["memory_step_s"] = med([e0.elapsed_time(e1) * 1e-3 for e0, e1 in mem_ms[a.warmup:]])
        out["memory_loss"] = run.alg.last_memory_loss
    del run
    torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--height", type=int, default=48)
    ap.add_argument("--steps", type=int, default=0, help="env steps per rollout (default: the task's num_steps_per_env)")
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "vision_train_time.json"))
    ap.add_argument("--memory", action="store_true", help="also the vision runner with a depth memory (memory=True): collection, update and memory-step time")
    ap.add_argument("--e2e", action="store_true", help="also the vision runner with end_to_end=True: collection, update and frame-log time, the log's size")
    ap.add_argument("--mount-jitter", default=None, help="POS,ROT_DEG (metres, degrees): also the vision runner with sensors.MountJitter(pos, rot_deg) on its camera")
    ap.add_argument("--instrument", default=None, help="latency=LO:HI,noise_gain=LO:HI,depth_scale=S,depth_quad=Q,fov=F (evaluate's --camera-instrument): also the "
                    "vision runner with that sensors.InstrumentError on its camera")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vision_train_time.py needs a GPU: there is no CPU form of this measurement")
    res = {"what": "seconds per PPO iteration, median; update_s of the vision runner includes encoder_step_s", "num_envs": a.envs,
           "steps": a.steps or "the task's num_steps_per_env",
           "camera": [a.width, a.height], "device": torch.cuda.get_device_name(0), "him": measure("him", a), "vision": measure("vision", a)}
    if a.mount_jitter:
        from isaacgymloco_amd.envs.sensors import MountJitter
        pos, rot = (float(v) for v in a.mount_jitter.split(","))
        a.jitter = MountJitter(pos=pos, rot_deg=rot)
        res["vision_jitter"] = measure("vision_jitter", a)      # one more launch per step in the collection; the update is the same
        res["mount_jitter"] = a.jitter.record()
    if a.instrument:
        from isaacgymloco_amd.learn.evaluate import parse_camera_instrument
        a.inst = parse_camera_instrument(a.instrument)
        res["vision_instrument"] = measure("vision_instrument", a)      # one more launch per step and the other capture kernel in the collection
        res["instrument"] = a.inst.record()
    if a.e2e:
        res["e2e"] = measure("e2e", a)                # collection_s includes frames_log_s; update_s includes the encoder passes of the end-to-end epochs
    if a.memory:
        res["memory"] = measure("memory", a)          # update_s includes encoder_step_s and memory_step_s
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
