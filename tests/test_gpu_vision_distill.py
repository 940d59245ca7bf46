"""GPU: vision distillation (learn/distill.py, learn/scan_policy.py) on a real device -- 64 Aliengo envs on stairs, a
16 x 12 camera of period 3, rollouts of 6 steps through the fused rollout: the labelling pass against its fp32 twin, the gradient through
the whole device path against the device's own per-transition path, what one iteration moves and what it leaves, the launches it makes,
the checkpoints, and the scan-reading teacher."""
import copy

import pytest
import torch

from test_gpu_sensor_chain import Logged

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, L, T, PERIOD, SCAN = 64, 10, 6, 3, 187
ENC = dict(c1=4, k1=3, s1=2, c2=8, k2=3, s2=1, latent_dim=L)
CAPTURE, LOG, ENCODE, ACT = "lsim_sensor_capture", "lsim_sensor_frames_log", "lsim_depth_encode", "lsim_policy_act_post_at_ext"
LABEL, LOSS, ROWS_GRAD = "lsim_policy_forward_ext", "lsim_distill_loss", "lsim_latent_rows_grad"
AUDITED = (CAPTURE, LOG, ENCODE, ACT, LABEL, LOSS, ROWS_GRAD)


def _env(seed):
    from isaacgymloco_amd.envs import config as C
    from isaacgymloco_amd.envs.legged_robot import LeggedRobot
    cfg = C.aliengo_cfg()
    cfg.env.num_envs = N
    cfg.terrain.terrain_proportions = [0.0, 0.0, 0.0, 0.0, 0.5, 0.5]
    return LeggedRobot(cfg, sim_device=DEV, seed=seed)


def _train_cfg(**alg_keys):
    from isaacgymloco_amd.learn.bench_train import train_cfg_dict
    tc = train_cfg_dict("aliengo")
    tc["runner"]["num_steps_per_env"] = T
    tc["algorithm"].update(**alg_keys)
    return tc


def _camera(env, logged=None):
    from isaacgymloco_amd.envs import sensors
    return env.add_sensor("depth", sensors.depth_camera(env, 16, 12, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, api=logged,
                                                        model=sensors.SensorModel(period=PERIOD, stagger=True, latency=1, frames=2, normalise=True)))


@pytest.fixture(scope="module")
def teacher(tmp_path_factory):
    """a ScanOnPolicyRunner after one iteration through the fused rollout, its scan columns far from their initialisation, saved:
    (path, state dict, runner)"""
    from isaacgymloco_amd.learn.scan_policy import ScanOnPolicyRunner
    from isaacgymloco_amd.learn.vision import VisionRollout
    env = _env(3)
    torch.manual_seed(3)
    run = ScanOnPolicyRunner(env, _train_cfg(), device=DEV)
    assert run.enable_graphs() and isinstance(run.graphs, VisionRollout)
    with torch.no_grad():
        ac = run.alg.actor_critic
        ac.actor[0].weight[:, -SCAN:] = 0.05 * torch.randn(ac.actor[0].out_features, SCAN, device=DEV)
        ac.std.fill_(0.3)
    run.learn(1)
    path = str(tmp_path_factory.mktemp("distill") / "teacher.pt")
    run.save(path)
    return path, {k: v.detach().clone() for k, v in run.alg.actor_critic.state_dict().items()}, run


def _make(seed, teacher, logged=None, plain=None, **alg_keys):
    """(env, camera, runner): a DistillRunner on `teacher`, or with `plain` = True / False the parent with that end_to_end"""
    from isaacgymloco_amd.learn.depth_encoder import DepthEncoder
    from isaacgymloco_amd.learn.distill import DistillRunner
    from isaacgymloco_amd.learn.vision import VisionOnPolicyRunner
    env = _env(seed)
    cam = _camera(env, logged)
    torch.manual_seed(seed)
    enc = DepthEncoder(12, 16, 2, **ENC)
    if plain is None:
        run = DistillRunner(env, _train_cfg(aux_snapshots=0, **alg_keys), teacher=teacher, sensor="depth", encoder=enc, device=DEV)
    else:
        run = VisionOnPolicyRunner(env, _train_cfg(aux_snapshots=0, num_learning_epochs=2, **alg_keys), sensor="depth", encoder=enc, device=DEV, end_to_end=plain)
    assert run.enable_graphs()
    return env, cam, run


def _depth_columns(run, seed=0):
    """depth columns a student would have after some training: with the warm start's zeros no gradient reaches the encoder"""
    g = torch.Generator().manual_seed(seed)
    w = run.alg.actor_critic.actor[0].weight
    with torch.no_grad():
        w[:, -L:] = (0.3 * torch.randn(w.shape[0], L, generator=g)).to(DEV)


def _rollout(env, cam, run):
    """T steps of the fused rollout with resets inside -> the frames each transition's latent came from [T, N, 2, 12, 16]"""
    env.episode_length_buf[:5] = int(env.max_episode_length) - 3
    frames = torch.zeros(T, N, 2, 12, 16, device=DEV)
    with torch.inference_mode():
        for t in range(T):
            frames[t] = cam.frame_images()
            run.graphs.step()
        run.graphs.flush()
        run.alg.compute_returns(env.privileged_obs_buf)
    run.graphs.end_iteration()
    torch.cuda.synchronize()
    return frames


@pytest.fixture(scope="module")
def recorded(teacher):
    """one rollout of a student, labelled: (env, camera, runner, frames)"""
    env, cam, run = _make(7, teacher[0])
    _depth_columns(run)
    frames = _rollout(env, cam, run)
    run.alg.label_rollout()
    torch.cuda.synchronize()
    return env, cam, run, frames


def test_the_labels_are_as_accurate_as_the_teachers_fp32_twin(recorded):
    """reference: the teacher's act_inference in fp64 on the CPU over the stored rows; the device pass (one lsim_policy_forward_ext) may be
    at most 4 x as far from it as the teacher evaluated in fp32 torch on the CPU"""
    env, cam, run, _ = recorded
    alg, st = run.alg, run.alg.storage
    off, w = alg.teacher_scan
    assert alg._teacher_packed is not None and alg.teacher_means.shape == (T * N, env.num_actions) and int(st.dones.sum()) >= 5
    obs, priv = st.observations.flatten(0, 1).cpu(), st.privileged_observations.flatten(0, 1).cpu()
    t64, t32 = copy.deepcopy(alg.teacher).double().cpu(), copy.deepcopy(alg.teacher).cpu()
    with torch.no_grad():
        want = t64.act_inference(obs.double(), depth_latent=priv[:, off:off + w].double())
        twin = t32.act_inference(obs, depth_latent=priv[:, off:off + w].contiguous())
        flat = t64.act_inference(obs.double(), depth_latent=torch.zeros(T * N, w, dtype=torch.float64))
    e_dev = float((alg.teacher_means.cpu().double() - want).abs().max())
    e_twin = float((twin.double() - want).abs().max())
    print(f"labels: max |device - fp64| = {e_dev:.3e}, max |fp32 torch on the CPU - fp64| = {e_twin:.3e}, largest mean {float(want.abs().max()):.3e}, "
          f"the scan moves the means by up to {float((want - flat).abs().max()):.3e}")
    assert float((want - flat).abs().max()) > 100.0 * e_twin, "the labels depend on the scan"
    assert e_twin > 0.0 and e_dev <= 4.0 * e_twin, (e_dev, e_twin)


def _relative(got, want):
    each = [float((g.detach().double().cpu() - w).abs().max() / w.abs().max()) for g, w in zip(got, want)]
    return max(each), each


def test_the_gradient_through_the_device_path_is_as_accurate_as_the_per_transition_path(recorded):
    """reference: the fp64 per-transition gradient of the first minibatch's distillation loss on the CPU, labels included; the path
    through frame log, lsim_distill_loss, lsim_latent_rows_grad and lsim_depth_encode_backward may be at most 4 x as far from it as the
    device's own per-transition path (forward_device on the un-deduplicated frames)"""
    from isaacgymloco_amd.learn.depth_encoder import DepthEncoder
    from isaacgymloco_amd.learn.distill import distill_loss
    env, cam, run, frames = recorded
    alg, ac, enc, st = run.alg, run.alg.actor_critic, run.alg.encoder, run.alg.storage
    off, w = alg.teacher_scan
    ac64, t64, enc64 = copy.deepcopy(ac).double().cpu(), copy.deepcopy(alg.teacher).double().cpu(), DepthEncoder(**enc.config()).double()
    enc64.load_state_dict({k: v.detach().double().cpu() for k, v in enc.state_dict().items()})
    alg._e2e_rows = int(cam.frames_log_state()[0])
    assert N < alg._e2e_rows < T * N and bool((st.frame_row >= 0).all())
    gen = st.mini_batch_generator(alg.num_mini_batches, 1)
    batch = next(gen)
    B = batch[0].shape[0]
    picked = st.last_perm[:B]
    index = picked.to(torch.int32)
    params = list(enc.parameters()) + list(ac.actor.parameters())
    loss_log = alg.minibatch_loss(ac, batch, 0)
    g_log = torch.autograd.grad(loss_log, params)
    per_transition = enc.forward_device(frames.flatten(0, 1)[picked].contiguous())
    with ac.bound_latent(per_transition, live=True):
        loss_dev = distill_loss(ac.actor(ac._actor_input(batch[0])), alg.teacher_means, index)
    g_dev = torch.autograd.grad(loss_dev, params)
    obs_all, priv_all = st.observations.flatten(0, 1).double().cpu(), st.privileged_observations.flatten(0, 1).double().cpu()
    with torch.no_grad():
        means64 = t64.act_inference(obs_all, depth_latent=priv_all[:, off:off + w])
    naive = enc64(frames.flatten(0, 1)[picked].double().cpu())
    with ac64.bound_latent(naive, live=True):
        loss64 = distill_loss(ac64.actor(ac64._actor_input(batch[0].double().cpu())), means64, index.cpu())
    g64 = torch.autograd.grad(loss64, list(enc64.parameters()) + list(ac64.actor.parameters()))
    gen.close()
    e_dev, each_dev = _relative(g_dev, g64)
    e_log, each_log = _relative(g_log, g64)
    print("gradient of the distillation loss, max |device - fp64| / max |fp64| per parameter (encoder w1 b1 w2 b2 w3 b3, then the actor's):")
    print("  per-transition device path:", " ".join(f"{v:.3e}" for v in each_dev), "-> error", f"{e_dev:.3e}")
    print("  frame-log path:            ", " ".join(f"{v:.3e}" for v in each_log), "-> error", f"{e_log:.3e}")
    print("  losses: fp64", float(loss64.detach()), "device", float(loss_dev.detach()), "log path", float(loss_log.detach()))
    assert all(float(g.abs().max()) > 0.0 for g in g64) and e_dev > 0.0
    assert e_log <= 4.0 * e_dev, (e_log, e_dev)


@pytest.fixture(scope="module")
def distilled(teacher, tmp_path_factory):
    """one iteration of a DistillRunner, saved: (path, runner, env, the actor's and the encoder's parameters before it)"""
    env, cam, run = _make(5, teacher[0], distill_epochs=2)
    _depth_columns(run)
    start_actor = [p.detach().clone() for p in run.alg.actor_critic.actor.parameters()]
    start_enc = [p.detach().clone() for p in run.alg.encoder.parameters()]
    env.episode_length_buf[:5] = int(env.max_episode_length) - 3
    run.learn(1)
    path = str(tmp_path_factory.mktemp("distilled") / "student.pt")
    run.save(path)
    return path, run, env, start_actor, start_enc


def test_one_iteration_moves_the_actor_and_the_encoder_and_nothing_of_the_teachers(teacher, distilled):
    _, teacher_sd, _ = teacher
    path, run, env, start_actor, start_enc = distilled
    alg, ac = run.alg, run.alg.actor_critic
    loss, aux = run.last_update
    print("distillation loss of the first iteration", loss)
    assert loss > 0.0 and aux != aux and alg.last_e2e_overflow == 0
    assert [bool((p != q).any()) for p, q in zip(alg.encoder.parameters(), start_enc)] == [True] * 6
    assert all(bool((p != q).any()) for p, q in zip(ac.actor.parameters(), start_actor))
    assert all(bool(torch.isfinite(p).all()) for p in list(ac.parameters()) + list(alg.encoder.parameters()))
    frozen = [k for k in teacher_sd if not k.startswith("actor.")]
    assert "std" in frozen and len(frozen) > 10
    for k in frozen:
        assert torch.equal(ac.state_dict()[k], teacher_sd[k]), k
    assert int(env.nonfinite_envs) == 0


def test_the_launches_are_the_parents_rollout_one_labelling_pass_and_three_per_minibatch(teacher, monkeypatch):
    from isaacgymloco_amd import lib
    rollout = [LOG] + [ACT, CAPTURE, LOG, ENCODE] * (T - 1) + [ACT, CAPTURE, ENCODE]
    seen, minibatches = {}, {}
    for kind in ("distill", "parent", "plain"):
        logged = Logged(lib.load(), AUDITED)
        with monkeypatch.context() as m:
            m.setattr(lib, "load", lambda logged=logged: logged)
            plain = {"distill": None, "parent": True, "plain": False}[kind]
            env, cam, run = _make(9, teacher[0], logged=logged, plain=plain)
            del logged.log[:]
            run.learn(2)
            seen[kind] = list(logged.log)
        minibatches[kind] = run.alg.num_mini_batches * (run.alg.distill_epochs if kind == "distill" else run.alg.e2e_epochs)
    assert seen["parent"] == (rollout + [ENCODE, ROWS_GRAD] * minibatches["parent"]) * 2, "the end-to-end parent: nothing of the new entry"
    assert seen["distill"] == (rollout + [LABEL] + [ENCODE, LOSS, ROWS_GRAD] * minibatches["distill"]) * 2, \
        "the parent's rollout; per update one lsim_policy_forward_ext; per minibatch one re-encoding, one loss launch, one gradient-rows launch"
    assert seen["plain"] == [ACT, CAPTURE, ENCODE] * (2 * T) and not {LABEL, LOSS} & set(seen["plain"]) and not {LABEL, LOSS} & set(seen["parent"])


def test_the_checkpoint_is_an_ordinary_vision_checkpoint(teacher, distilled, tmp_path):
    from isaacgymloco_amd.envs import sensors
    from isaacgymloco_amd.learn.evaluate import evaluate
    path, run, _, _, _ = distilled
    alg = run.alg
    d = torch.load(path, map_location="cpu", weights_only=False)
    assert d["distill"]["teacher"] == {"offset": 238 - SCAN, "width": SCAN, "dim": SCAN} and d["distill"]["epochs"] == 2
    assert d["vision"]["latent_dim"] == L and d["vision"]["end_to_end"]["epochs"] == 1
    # a second DistillRunner: parameters and both optimisers' moments
    env2, cam2, run2 = _make(6, teacher[2], distill_epochs=2)
    run2.load(path)
    for a, b in zip(list(alg.actor_critic.parameters()) + list(alg.encoder.parameters()),
                    list(run2.alg.actor_critic.parameters()) + list(run2.alg.encoder.parameters())):
        assert torch.equal(a, b)
    for name in ("distill_optimizer", "e2e_optimizer"):
        sa, sb = getattr(alg, name).state_dict()["state"], getattr(run2.alg, name).state_dict()["state"]
        assert sa and all(torch.equal(sa[k]["exp_avg"], sb[k]["exp_avg"]) and torch.equal(sa[k]["exp_avg_sq"], sb[k]["exp_avg_sq"]) for k in sa)
    # a plain vision runner goes on with PPO from it, and exports it
    env3, cam3, plain = _make(8, None, plain=False)
    plain.load(path)
    assert torch.equal(plain.alg.actor_critic.actor[0].weight, alg.actor_critic.actor[0].weight)
    before = plain.alg.actor_critic.critic[0].weight.detach().clone()
    plain.learn(1)
    assert bool((plain.alg.actor_critic.critic[0].weight != before).any()) and int(env3.nonfinite_envs) == 0
    assert all(bool(torch.isfinite(p).all()) for p in plain.alg.actor_critic.parameters())
    plain.load(path)
    mod = torch.jit.load(plain.export(str(tmp_path / "exported")))
    with torch.no_grad():
        frames, obs = cam3.frame_images().cpu(), env3.get_observations().cpu()
        got = mod.act(obs, mod.encode(frames))
        want = plain.alg.actor_critic.cpu().act_inference(obs, depth_latent=plain.alg.encoder.cpu()(frames))
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6)
    # evaluate takes the file as it takes any vision checkpoint
    env4 = _env(4)
    env4.reset()
    env4.add_sensor("depth", sensors.from_spec(env4, d["vision"]["sensor"]))
    res = evaluate(env4, path, 5, commands=(0.5, 0.0, 0.0)).result()
    assert res["conventions"]["columns"] == ["depth_influence", "scan_error"] and res["total"]["samples"] > 0
    assert res["total"]["columns"]["depth_influence"]["mean"] > 0.0 and int(env4.nonfinite_envs) == 0


def test_the_teachers_storage_holds_the_scan_block_and_its_checkpoint_evaluates(teacher):
    from isaacgymloco_amd.learn.evaluate import evaluate
    from isaacgymloco_amd.learn.vision import PackedVisionPolicy, height_scan_block
    path, _, run = teacher
    env, st = run.env, run.alg.storage
    off, w = height_scan_block(env.cfg)
    assert (off, w) == (238 - SCAN, SCAN) and PackedVisionPolicy.supported(run.alg.actor_critic)
    env.episode_length_buf[:5] = int(env.max_episode_length) - 3
    with torch.inference_mode():
        for _ in range(T):
            run.graphs.step()
        run.graphs.flush()
    run.graphs.end_iteration()
    torch.cuda.synchronize()
    assert int(st.dones.sum()) >= 5 and float(st.depth_latent.abs().max()) > 0.0
    assert torch.equal(st.depth_latent, st.privileged_observations[:, :, off:off + w]), "the rows the actor read are the critic's scan block"
    st.clear()
    d = torch.load(path, map_location="cpu", weights_only=False)
    assert d["scan_policy"] == {"offset": off, "width": w, "dim": w}
    env2 = _env(12)
    env2.reset()
    for fused in (True, False):
        res = evaluate(env2, path, 5, commands=(0.5, 0.0, 0.0), fused=fused).result()
        assert res["total"]["samples"] > 0 and not res["total"].get("columns") and int(env2.nonfinite_envs) == 0
    with pytest.raises(ValueError, match="no sensor"):
        evaluate(env2, path, 1, vision_metrics=("scan_error",))
