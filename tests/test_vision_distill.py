"""CPU: vision distillation (learn/distill.py, learn/scan_policy.py) on the emulated env -- N = 8, T = 6, a 16 x 12 camera of
period 3, fp64 above the sensor where exactness is claimed: the exact fixed point, the gradient through log and join against the naive
per-transition construction, the parts that stay frozen, the scan policy's storage invariant, checkpoints and evaluate.
tests/test_gpu_vision_distill.py runs the device half."""
import copy

import pytest
import torch

import eval_columns_emu_binding as CB
import frames_log_emu_binding as FB
from isaacgymloco_amd.learn import vision as V
from isaacgymloco_amd.learn.depth_encoder import DepthEncoder
from isaacgymloco_amd.learn.distill import DistillRunner, VisionDistill, distill_loss
from isaacgymloco_amd.learn.modules import HIMActorCritic
from isaacgymloco_amd.learn.scan_policy import ScanOnPolicyRunner
from test_vision_end_to_end import A, ENC, L, N, N1, O, P, T, _camera, _env, _step, fp64  # noqa: F401  (fp64 is a fixture)

SCAN = 187


def _train_cfg(**alg_keys):
    from isaacgymloco_amd.learn.bench_train import train_cfg_dict
    tc = train_cfg_dict("aliengo")
    tc["runner"]["num_steps_per_env"] = T
    tc["algorithm"].update(num_learning_epochs=2, num_mini_batches=2, **alg_keys)
    return tc


def _teacher(generic):
    """a VisionActorCritic over the scan block: made by load_him_state_dict (its scan columns are zero), or with the scan columns random"""
    teacher = V.VisionActorCritic(O, P, N1, A, depth_latent_dim=SCAN)
    teacher.load_him_state_dict(HIMActorCritic(O, P, N1, A).state_dict())
    if generic:
        with torch.no_grad():
            teacher.actor[0].weight[:, -SCAN:].normal_(0.0, 0.05)
    return teacher


def _learner(env, generic, **alg_keys):
    """(camera, student, encoder, VisionDistill with storage, frame log and teacher attached), everything above the sensor in the default dtype"""
    cam = env.add_sensor("depth", _camera(env, FB.EmuApi()))
    cam.attach_encoder(DepthEncoder(12, 16, 2, **ENC).float())          # the sensor's own fp32 launch: the log stage needs one
    teacher = _teacher(generic)
    ac, enc = V.VisionActorCritic(O, P, N1, A, depth_latent_dim=L), DepthEncoder(12, 16, 2, **ENC)
    ac.load_scan_teacher_state_dict(teacher.state_dict(), SCAN)
    if generic:
        with torch.no_grad():
            ac.actor[0].weight[:, -L:].normal_(0.0, 0.3)                # the depth columns carry a gradient to the encoder
    dtype = enc.fc.weight.dtype
    alg = VisionDistill(ac, encoder=enc, latent_source=lambda: enc(cam.frame_images().to(dtype)), frames_source=cam.frame_images, aux_snapshots=0,
                        num_mini_batches=2, device="cpu", **alg_keys)
    alg.init_storage(N, T, [O], [P], [A])
    cam.attach_frames_log(T, row_of=alg.storage.frame_row)
    alg.attach_frame_log(cam)
    alg.attach_teacher(teacher, V.height_scan_block(env.cfg))
    return cam, ac, enc, alg


def _rollout(env, cam, alg):
    """T eager steps with a reset inside -> the frames every transition's latent came from [T, N, 2, 12, 16]"""
    dtype = next(alg.actor_critic.parameters()).dtype
    env.episode_length_buf[2] = int(env.max_episode_length) - 2
    frames = torch.zeros(T, N, 2, 12, 16, dtype=torch.float32)
    obs, crit = env.get_observations().to(dtype), env.get_privileged_observations().to(dtype)
    with torch.inference_mode():
        for t in range(T):
            frames[t] = cam.frame_images()
            obs, crit, _ = _step(env, alg, obs, crit)
        alg.compute_returns(crit)
    return frames


def test_the_student_warm_start_drops_the_scan_columns_and_zeroes_the_depth_columns():
    teacher = _teacher(True)
    ac = V.VisionActorCritic(O, P, N1, A, depth_latent_dim=L)
    ac.load_scan_teacher_state_dict(teacher.state_dict(), SCAN)
    k = N1 + 3 + 16
    assert torch.equal(ac.actor[0].weight[:, :k], teacher.actor[0].weight[:, :k]) and bool((ac.actor[0].weight[:, k:] == 0).all())
    for name, v in teacher.state_dict().items():
        if name != "actor.0.weight":
            assert torch.equal(ac.state_dict()[name], v), name
    with pytest.raises(ValueError, match="actor.0.weight"):
        ac.load_scan_teacher_state_dict(teacher.state_dict(), SCAN - 1)


def test_a_student_that_is_the_teacher_is_an_exact_fixed_point(fp64):
    """(a) the teacher is made by load_him_state_dict, so its scan columns are zero and the warm-started student computes its means: the
    loss is exactly 0.0 and update() moves no parameter of the actor or the encoder"""
    torch.manual_seed(0)
    env = _env()
    cam, ac, enc, alg = _learner(env, generic=False, distill_epochs=2)
    _rollout(env, cam, alg)
    before = [p.detach().clone() for p in list(ac.parameters()) + list(enc.parameters())]
    loss, aux = alg.update()
    assert loss == 0.0 and aux != aux, (loss, aux)                      # aux_snapshots = 0: no auxiliary loss, NaN
    assert alg._e2e_rows > N and alg.teacher_means.shape == (T * N, A) and float(alg.teacher_means.abs().max()) > 0.0
    for p, q in zip(list(ac.parameters()) + list(enc.parameters()), before):
        assert torch.equal(p, q)
    assert alg.storage.step == 0 and all(p.grad is None for p in enc.parameters())


def test_the_gradient_through_log_and_join_is_the_per_transition_one(fp64):
    """(b) a generic teacher: the gradient of the first minibatch's distillation loss with respect to the six encoder parameters and the
    actor's, through frame log + join, equals the naive construction encoder(frames[t, n]) per transition to 1e-9 of its largest entry"""
    torch.manual_seed(1)
    env = _env()
    cam, ac, enc, alg = _learner(env, generic=True)
    frames = _rollout(env, cam, alg)
    st = alg.storage
    means = alg.label_rollout()
    off, w = alg.teacher_scan
    want = alg.teacher.act_inference(st.observations.flatten(0, 1).double(), depth_latent=st.privileged_observations.flatten(0, 1)[:, off:off + w].double())
    assert torch.equal(means, want) and means.dtype == torch.float64
    alg._e2e_rows = int(cam.frames_log_state()[0])
    gen = st.mini_batch_generator(alg.num_mini_batches, 1)
    batch = next(gen)
    batch = tuple(b.double() if b.is_floating_point() else b for b in batch)
    B = batch[0].shape[0]
    picked = st.last_perm[:B]
    params = list(enc.parameters()) + list(ac.actor.parameters())
    loss = alg.minibatch_loss(ac, batch, 0)
    g_log = torch.autograd.grad(loss, params)
    naive = enc(frames.flatten(0, 1)[picked].double())
    with ac.bound_latent(naive, live=True):
        mu = ac.actor(ac._actor_input(batch[0]))
    loss2 = distill_loss(mu, means, picked.to(torch.int32))
    g_naive = torch.autograd.grad(loss2, params)
    loss, loss2 = float(loss.detach()), float(loss2.detach())
    assert loss > 0.0 and abs(loss - loss2) <= 1e-12 * loss2
    assert abs(loss2 - float((mu.detach() - means[picked]).square().mean())) <= 1e-12 * loss2, "the loss is the mean squared error"
    for i, (a, b) in enumerate(zip(g_log, g_naive)):
        scale, err = float(b.abs().max()), float((a - b).abs().max())
        print("parameter", i, "max |log path - per transition|", err, "largest entry", scale)
        assert scale > 0.0 and err <= 1e-9 * scale, (i, err, scale)
    gen.close()


def test_rows_outside_the_labels_carry_no_loss_in_the_torch_statement():
    mu = torch.randn(5, 3, dtype=torch.float64, requires_grad=True)
    target = torch.randn(7, 3, dtype=torch.float64)
    index = torch.tensor([2, -1, 6, 7, 0], dtype=torch.int32)
    with torch.no_grad():
        mu[1], mu[3] = float("nan"), float("nan")
    loss = distill_loss(mu, target, index)
    g, = torch.autograd.grad(loss, mu)
    keep = [0, 2, 4]
    d = mu.detach()[keep] - target[[2, 6, 0]]
    assert torch.allclose(loss, (d * d).sum() / 15.0) and torch.allclose(g[keep], d * (2.0 / 15.0)) and bool((g[[1, 3]] == 0).all())


def _runner(env, cam, teacher, **alg_keys):
    torch.manual_seed(7)
    return DistillRunner(env, _train_cfg(aux_snapshots=0, **alg_keys), teacher=teacher, sensor=cam, encoder=DepthEncoder(12, 16, 2, **ENC), device="cpu")


def _scan_runner(env, seed=11):
    torch.manual_seed(seed)
    return ScanOnPolicyRunner(env, _train_cfg(), device="cpu")


def test_the_scan_policys_storage_holds_the_scan_block_and_its_checkpoint_evaluates(tmp_path):
    """(d) storage.depth_latent[t] is storage.privileged_observations[t][:, off:off + w] exactly; the checkpoint carries the record,
    evaluates with the base columns only, and refuses vision metrics that are named"""
    from isaacgymloco_amd.learn.evaluate import Evaluator, evaluate
    env = _env()
    run = _scan_runner(env)
    alg, ac = run.alg, run.alg.actor_critic
    off, w = V.height_scan_block(env.cfg)
    assert (off, w) == (P - SCAN, SCAN) and ac.depth_latent_dim == SCAN and ac.actor[0].in_features == 251 and run.scan == (off, w)
    rows = alg.latent_source()
    assert rows.data_ptr() == env.privileged_obs_buf.data_ptr() + 4 * off and rows.stride() == (P, 1), "a column-slice view: nothing is copied"
    obs, crit = env.get_observations().clone(), env.get_privileged_observations().clone()
    with torch.inference_mode():
        for _ in range(T):
            obs, crit = run._rollout_step(obs, crit)[:2]
    st = alg.storage
    assert torch.equal(st.depth_latent, st.privileged_observations[:, :, off:off + w]) and float(st.depth_latent.abs().max()) > 0.0
    st.clear()
    run.learn(1)
    path = str(tmp_path / "teacher.pt")
    run.save(path)
    d = torch.load(path, weights_only=False)
    assert d["scan_policy"] == {"offset": off, "width": w, "dim": w} and "vision" not in d and "map_policy" not in d
    him = HIMActorCritic(O, P, N1, A)
    run.load_him_state_dict(him.state_dict())
    assert bool((ac.actor[0].weight[:, -w:] == 0).all()) and torch.equal(ac.actor[0].weight[:, :-w], him.actor[0].weight)
    ev = lambda policy, **kw: evaluate(env, policy, 3, commands=(0.5, 0.0, 0.0), evaluator=Evaluator(env, api=CB.EmuApi()), fused=False, **kw).result()
    for policy in (path, run):
        res = ev(policy)
        assert res["total"]["samples"] > 0 and not res["total"].get("columns")
    assert not ev(path, blind=True, vision_metrics=()).get("columns")
    with pytest.raises(ValueError, match="no vision\\s+metrics|no sensor"):
        ev(path, vision_metrics=("depth_influence",))
    flat = copy.deepcopy(env.cfg)
    flat.terrain.measure_heights = False
    env.cfg = flat
    with pytest.raises(ValueError, match="measure_heights"):
        _scan_runner(env)


def test_one_iteration_moves_actor_and_encoder_and_leaves_the_teachers_parts_and_the_checkpoint_is_a_vision_checkpoint(tmp_path):
    """(c) after learn(1): estimator, critic and std are bit-identical to the teacher's, the actor and all six encoder parameters
    moved; the checkpoint loads into a second DistillRunner with both optimisers' moments, and into a plain VisionOnPolicyRunner, which
    goes on with PPO"""
    env = _env()
    teacher_run = _scan_runner(env)
    with torch.no_grad():
        teacher_run.alg.actor_critic.std.fill_(0.3)
    teacher_path = str(tmp_path / "teacher.pt")
    teacher_run.save(teacher_path)
    teacher_sd = {k: v.clone() for k, v in teacher_run.alg.actor_critic.state_dict().items()}
    cam = env.add_sensor("depth", _camera(env, FB.EmuApi()))
    with pytest.raises(NotImplementedError, match="memory"):
        DistillRunner(env, _train_cfg(), teacher=teacher_path, sensor=cam, memory=True)
    with pytest.raises(ValueError, match="scan_policy"):
        DistillRunner(env, _train_cfg(), teacher={"model_state_dict": teacher_sd}, sensor=cam)
    run = _runner(env, cam, teacher_path, distill_epochs=2, distill_learning_rate=3e-4)
    alg, ac = run.alg, run.alg.actor_critic
    assert isinstance(alg, VisionDistill) and alg.end_to_end and alg.storage.frame_row is not None
    assert bool((ac.actor[0].weight[:, -L:] == 0).all()) and alg.teacher.depth_latent_dim == SCAN
    with torch.no_grad():
        ac.actor[0].weight[:, -L:].normal_(0.0, 0.3)
    start_actor = [p.detach().clone() for p in ac.actor.parameters()]
    start_enc = [p.detach().clone() for p in alg.encoder.parameters()]
    run.learn(1)
    loss, aux = run.last_update
    assert loss > 0.0 and loss == alg.last_distill_loss and aux != aux
    assert all(bool((p != q).any()) for p, q in zip(ac.actor.parameters(), start_actor))
    assert [bool((p != q).any()) for p, q in zip(alg.encoder.parameters(), start_enc)] == [True] * 6
    frozen = [k for k in teacher_sd if not k.startswith("actor.")]
    assert "std" in frozen and any(k.startswith("critic.") for k in frozen) and any(k.startswith("estimator.") for k in frozen)
    for k in frozen:
        assert torch.equal(ac.state_dict()[k], teacher_sd[k]), k
    for k, v in alg.teacher.state_dict().items():
        assert torch.equal(v, teacher_sd[k]), k
    path = str(tmp_path / "student.pt")
    run.save(path)
    d = torch.load(path, weights_only=False)
    assert d["distill"]["teacher"] == {"offset": P - SCAN, "width": SCAN, "dim": SCAN} and d["distill"]["epochs"] == 2 and d["distill"]["learning_rate"] == 3e-4
    assert len(d["distill"]["distill_optimizer_state_dict"]["state"]) == len(start_actor) and d["vision"]["latent_dim"] == L
    env2 = _env()
    cam2 = env2.add_sensor("depth", _camera(env2, FB.EmuApi()))
    run2 = _runner(env2, cam2, teacher_run, distill_epochs=2, distill_learning_rate=3e-4)         # the teacher as a runner
    run2.load(path)
    for a, b in zip(list(ac.parameters()) + list(alg.encoder.parameters()), list(run2.alg.actor_critic.parameters()) + list(run2.alg.encoder.parameters())):
        assert torch.equal(a, b)
    for name in ("distill_optimizer", "e2e_optimizer"):
        sa, sb = getattr(alg, name).state_dict()["state"], getattr(run2.alg, name).state_dict()["state"]
        assert sa and all(torch.equal(sa[k]["exp_avg"], sb[k]["exp_avg"]) and torch.equal(sa[k]["exp_avg_sq"], sb[k]["exp_avg_sq"]) for k in sa)
    run2.learn(1)
    env3 = _env()
    cam3 = env3.add_sensor("depth", _camera(env3, FB.EmuApi()))
    torch.manual_seed(3)
    plain = V.VisionOnPolicyRunner(env3, _train_cfg(aux_snapshots=0), sensor=cam3, encoder=DepthEncoder(12, 16, 2, **ENC), device="cpu", end_to_end=False)
    plain.load(path)
    assert torch.equal(plain.alg.actor_critic.actor[0].weight, ac.actor[0].weight) and type(plain.alg) is V.VisionPPO
    plain.learn(1)
    assert len(plain.last_update) == 5 and all(bool(torch.isfinite(p).all()) for p in plain.alg.actor_critic.parameters())
