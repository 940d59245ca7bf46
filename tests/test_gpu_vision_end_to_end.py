"""GPU: the PPO gradient into the depth encoder (learn/vision.py, end_to_end=True) on a real device -- 64 Aliengo envs on
stairs, a 16 x 12 camera of period 3, rollouts of 6 steps through the fused rollout, aux_snapshots = 0 so that only the new path can move
the encoder: it moves, its gradient through frame log, lsim_latent_rows_grad and lsim_depth_encode_backward is as accurate as the
per-transition device path, the latent recomputed from the log is the stored one, the checkpoint follows, and off means off."""
import copy

import numpy as np
import pytest
import torch

import depth_encoder_emu_binding as DB
import depth_encoder_reference as ER
from test_gpu_sensor_chain import Logged

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, L, T, PERIOD = 64, 10, 6, 3
ENC = dict(c1=4, k1=3, s1=2, c2=8, k2=3, s2=1, latent_dim=L)
SENSOR_ENTRIES = ("lsim_sensor_capture", "lsim_sensor_frames_log", "lsim_depth_encode")
NEW_ENTRIES = ("lsim_sensor_frames_log", "lsim_latent_rows_grad")


def _make(seed, end_to_end, logged=None, **alg_keys):
    """(env, camera, runner): `logged`: a Logged library the camera launches through"""
    from isaacgymloco_amd.envs import config as C
    from isaacgymloco_amd.envs import sensors
    from isaacgymloco_amd.envs.legged_robot import LeggedRobot
    from isaacgymloco_amd.learn.bench_train import train_cfg_dict
    from isaacgymloco_amd.learn.depth_encoder import DepthEncoder
    from isaacgymloco_amd.learn.vision import VisionOnPolicyRunner
    cfg = C.aliengo_cfg()
    cfg.env.num_envs = N
    cfg.terrain.terrain_proportions = [0.0, 0.0, 0.0, 0.0, 0.5, 0.5]
    env = LeggedRobot(cfg, sim_device=DEV, seed=seed)
    cam = env.add_sensor("depth", sensors.depth_camera(env, 16, 12, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, api=logged,
                                                       model=sensors.SensorModel(period=PERIOD, stagger=True, latency=1, frames=2, normalise=True)))
    tc = train_cfg_dict("aliengo")
    tc["runner"]["num_steps_per_env"] = T
    tc["algorithm"].update(aux_snapshots=0, num_learning_epochs=2, **alg_keys)
    torch.manual_seed(seed)
    run = VisionOnPolicyRunner(env, tc, sensor="depth", encoder=DepthEncoder(12, 16, 2, **ENC), device=DEV, end_to_end=end_to_end)
    assert run.enable_graphs()
    return env, cam, run


def test_the_encoder_moves_only_with_the_switch_on_and_the_checkpoint_follows(tmp_path):
    from isaacgymloco_amd.learn.vision import VisionRollout
    moved = {}
    for on in (True, False):
        env, cam, run = _make(5, on)
        alg = run.alg
        assert isinstance(run.graphs, VisionRollout)
        start = [p.detach().clone() for p in alg.encoder.parameters()]
        env.episode_length_buf[:5] = int(env.max_episode_length) - 3         # these time out, and reset, inside the rollout
        run.learn(1)
        moved[on] = [bool((p != q).any()) for p, q in zip(alg.encoder.parameters(), start)]
        assert all(bool(torch.isfinite(p).all()) for p in alg.encoder.parameters()) and all(p.grad is None for p in alg.encoder.parameters())
        path = str(tmp_path / f"vision_{on}.pt")
        run.save(path)
        d = torch.load(path, map_location="cpu", weights_only=False)
        if not on:
            assert "depth_e2e_optimizer_state_dict" not in d and "end_to_end" not in d["vision"] and alg.storage.frame_row is None
            continue
        rows, overflow = cam.frames_log_state()[:2].tolist()
        print("logged images", rows, "of", T * N, "transitions; capacity", cam.frames_log().shape[0], "overflow", overflow)
        assert N + (T - 1) * (N // PERIOD) <= rows < cam.frames_log().shape[0] and overflow == 0 and alg.last_e2e_overflow == 0
        assert d["vision"]["end_to_end"] == {"epochs": 1, "learning_rate": alg.aux_learning_rate, "capacity": N * 5}
        assert len(d["depth_e2e_optimizer_state_dict"]["state"]) == 6
        env2, cam2, run2 = _make(6, True)
        run2.load(path)
        for a, b in zip(alg.encoder.parameters(), run2.alg.encoder.parameters()):
            assert torch.equal(a, b)
        sa, sb = alg.e2e_optimizer.state_dict()["state"], run2.alg.e2e_optimizer.state_dict()["state"]
        assert all(torch.equal(sa[k]["exp_avg"], sb[k]["exp_avg"]) and torch.equal(sa[k]["exp_avg_sq"], sb[k]["exp_avg_sq"]) for k in sa)
        loaded = [p.detach().clone() for p in run2.alg.encoder.parameters()]
        run2.learn(1)
        assert all(bool(torch.isfinite(p).all()) for p in run2.alg.encoder.parameters()) and int(env2.nonfinite_envs) == 0
        assert all(bool((p != q).any()) for p, q in zip(run2.alg.encoder.parameters(), loaded))
    assert moved[True] == [True] * 6, "end_to_end=True: the PPO loss moves the encoder"
    assert moved[False] == [False] * 6, "aux_snapshots = 0 and no end-to-end gradient: nothing moves the encoder"


def _relative(got, want):
    """max over the six parameters of max |got - want| / max |want|, and the six figures"""
    each = [float((g.detach().double().cpu() - w).abs().max() / w.abs().max()) for g, w in zip(got, want)]
    return max(each), each


def test_the_gradient_through_the_log_is_as_accurate_as_the_per_transition_path_and_the_latent_is_the_stored_one():
    """One recorded rollout.  (a) The latent of every logged image under the rollout's weights against the rows the rollout stored: both
    are lsim_depth_encode's, each within the forward's derived bound of the fp64 reference (tests/depth_encoder_reference.py), so they
    differ by at most twice that bound.  (b) The encoder gradient of the first minibatch's PPO loss: fp64 per transition on the CPU
    (the construction of tests/test_vision_end_to_end.py) is the reference; the device's own per-transition path (forward_device on the
    un-deduplicated frames) has some error against it, and the log path -- one short sum per row more, the batch sums in another order,
    no new arithmetic -- may have at most 4 x that."""
    from isaacgymloco_amd.learn.him_ppo import HIMPPO
    env, cam, run = _make(7, True)
    alg, ac, enc, st = run.alg, run.alg.actor_critic, run.alg.encoder, run.alg.storage
    from isaacgymloco_amd.learn.depth_encoder import DepthEncoder
    ac64, enc64 = copy.deepcopy(ac).double().cpu(), DepthEncoder(**enc.config()).double()       # nothing below changes a weight
    enc64.load_state_dict({k: v.detach().double().cpu() for k, v in enc.state_dict().items()})
    env.episode_length_buf[:5] = int(env.max_episode_length) - 3
    frames = torch.zeros(T, N, 2, 12, 16, device=DEV)
    with torch.inference_mode():
        for t in range(T):
            frames[t] = cam.frame_images()
            run.graphs.step()
        run.graphs.flush()
        alg.compute_returns(env.privileged_obs_buf)
    run.graphs.end_iteration()
    torch.cuda.synchronize()
    assert int(st.dones.sum()) >= 5
    gen = alg._sample_stream()
    batch, _ = next(gen)
    rows = alg._e2e_rows
    assert len(batch) == 12 and alg._e2e_minibatch == 0 and N < rows < T * N and bool((st.frame_row >= 0).all())
    log = cam.frames_log()[:rows]
    assert torch.equal(log[st.frame_row.long()].unflatten(3, (12, 16)), frames), "every transition finds its own frames in the log"
    # (a)
    with torch.no_grad():
        z = enc.forward_device_rows(log)
    again = z[st.frame_row.flatten().long()].cpu().numpy()
    stored = st.depth_latent.flatten(0, 1).cpu().numpy()
    want, bound = ER.encode(log.unflatten(2, (12, 16)).cpu().numpy().astype(np.float64), DB.params_of(enc), 2, 1, True)
    bound = bound[st.frame_row.flatten().long().cpu().numpy()]
    worst = float((np.abs(again - stored) / (2.0 * bound)).max())
    same = bool(np.array_equal(again.view(np.uint32), stored.view(np.uint32)))
    print(f"latent recomputed from the log vs stored: worst |difference| / (2 x bound) = {worst:.3e}, max |difference| = {np.abs(again - stored).max():.3e}, bit-equal: {same}")
    assert worst <= 1.0
    # (b)
    B = batch[0].shape[0]
    picked = st.last_perm[:B]
    params = list(enc.parameters())
    mb = alg._mb_forward(ac, batch, False)
    g_log = torch.autograd.grad(mb.loss, params)
    per_transition = enc.forward_device(frames.flatten(0, 1)[picked].contiguous())
    with ac.bound_latent(per_transition, live=True):
        mb_dev = HIMPPO._mb_forward(alg, ac, batch[:10], False)
    g_dev = torch.autograd.grad(mb_dev.loss, params)
    batch64 = tuple(b.detach().double().cpu() for b in batch[:10])
    naive = enc64(frames.flatten(0, 1)[picked].double().cpu())
    with ac64.bound_latent(naive, live=True):
        mb64 = HIMPPO._mb_forward(alg, ac64, batch64, False)
    g64 = torch.autograd.grad(mb64.loss, list(enc64.parameters()))
    gen.close()
    e_dev, each_dev = _relative(g_dev, g64)
    e_log, each_log = _relative(g_log, g64)
    print("encoder gradient, max |device - fp64| / max |fp64| per parameter (w1 b1 w2 b2 w3 b3):")
    print("  per-transition device path:", " ".join(f"{v:.3e}" for v in each_dev), "-> error", f"{e_dev:.3e}")
    print("  frame-log path:            ", " ".join(f"{v:.3e}" for v in each_log), "-> error", f"{e_log:.3e}")
    print("  losses: fp64", float(mb64.loss.detach()), "device", float(mb_dev.loss.detach()), "log path", float(mb.loss.detach()))
    assert all(float(g.abs().max()) > 0.0 for g in g64) and e_dev > 0.0
    assert e_log <= 4.0 * e_dev, (e_log, e_dev)


def test_off_means_off(monkeypatch):
    """end_to_end=False: the chain, the record and the storage are the parent's, and over two iterations the library sees the parent's
    launches; with it on, the same wrapper sees the two new entry points"""
    from isaacgymloco_amd import lib
    seen = {}
    for on in (False, True):
        logged = Logged(lib.load(), SENSOR_ENTRIES + ("lsim_latent_rows_grad",))
        with monkeypatch.context() as m:
            m.setattr(lib, "load", lambda logged=logged: logged)
            env, cam, run = _make(9, on, logged=logged)
            spec = cam.spec()
            del logged.log[:]
            run.learn(2)
            seen[on] = list(logged.log)
        assert cam.spec() == spec and "frames_log" not in str(sorted(spec))
        if not on:
            assert cam.chain() == ("lsim_sensor_capture", "lsim_depth_encode") and cam.stage("frames_log") is None
            assert run.alg.storage.frame_row is None and len(run.alg.storage._extra_fields()) == 1
    assert seen[False] == ["lsim_sensor_capture", "lsim_depth_encode"] * (2 * T), "the parent's launches: the capture and the encoder behind every env step"
    assert not set(seen[False]) & set(NEW_ENTRIES)
    per_rollout = ["lsim_sensor_frames_log"] + ["lsim_sensor_capture", "lsim_sensor_frames_log", "lsim_depth_encode"] * (T - 1) + ["lsim_sensor_capture", "lsim_depth_encode"]
    minibatches = run.alg.e2e_epochs * run.alg.num_mini_batches
    update = ["lsim_depth_encode", "lsim_latent_rows_grad"] * minibatches
    assert seen[True] == (per_rollout + update) * 2, "one log launch per rollout start and per env step but the last; one re-encoding and one gradient launch per end-to-end minibatch"
