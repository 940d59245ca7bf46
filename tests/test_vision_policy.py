"""CPU: the vision policy (learn/vision.py) -- the depth latent as the last segment of the actor input, its rollout storage, the PPO update
that feeds the stored rows back, the encoder's own regression step, the host-side refusals of the two C-ABI entry points and the checkpoint."""
import ctypes
import os
import types

import pytest
import torch

from isaacgymloco_amd import abi, lib
from isaacgymloco_amd.learn.depth_encoder import DepthEncoder
from isaacgymloco_amd.learn.him_ppo import HIMPPO
from isaacgymloco_amd.learn.modules import HIMActorCritic
from isaacgymloco_amd.learn import vision as V

O, P, N1, A = 270, 238, 45, 12          # the policy of tests/test_gpu_learner.py
K_HIM = N1 + 3 + 16


def _small_encoder(latent_dim=10):
    return DepthEncoder(12, 16, 2, c1=4, k1=3, s1=2, c2=8, k2=3, s2=1, latent_dim=latent_dim)


def _perturb(module, scale=0.05):
    with torch.no_grad():
        for p in module.parameters():
            p.add_(scale * torch.randn_like(p))


def test_action_mean_is_the_torch_statement():
    torch.manual_seed(0)
    ac = V.VisionActorCritic(O, P, N1, A, depth_latent_dim=10)
    _perturb(ac)
    assert ac.actor[0].in_features == K_HIM + 10 and ac.critic[0].in_features == P and ac.estimator.encoder[0].in_features == O
    obs, lat = torch.randn(7, O), torch.randn(7, 10)
    with torch.no_grad():
        vel, z = ac.estimator(obs)
        want = ac.actor(torch.cat((obs[:, :N1], vel, z, lat), dim=-1))
        assert torch.equal(ac.act_inference(obs, lat), want)
        ac.update_distribution(obs, lat)
        assert torch.equal(ac.action_mean, want)
        ac.act(obs, depth_latent=lat)
        assert torch.equal(ac.action_mean, want)
        with ac.bound_latent(lat):
            assert torch.equal(ac.actor(ac._actor_input(obs)), want)


def test_warm_start_from_a_him_policy_is_the_him_policy():
    torch.manual_seed(1)
    him = HIMActorCritic(O, P, N1, A)
    _perturb(him)
    vis = V.VisionActorCritic(O, P, N1, A, depth_latent_dim=10)
    _perturb(vis)
    vis.load_him_state_dict(him.state_dict())
    assert torch.equal(vis.actor[0].weight[:, :K_HIM], him.actor[0].weight) and not vis.actor[0].weight[:, K_HIM:].any()
    obs, priv = torch.randn(9, O), torch.randn(9, P)
    with torch.no_grad():
        want = him.act_inference(obs)
        for lat in (torch.randn(9, 10), 1e4 * torch.randn(9, 10), torch.zeros(9, 10)):
            assert torch.equal(vis.act_inference(obs, lat), want)
        assert torch.equal(vis.evaluate(priv), him.evaluate(priv))
    with pytest.raises(ValueError, match="actor.0.weight"):
        vis.load_him_state_dict(vis.state_dict())


def test_a_missing_latent_raises():
    ac = V.VisionActorCritic(O, P, N1, A, depth_latent_dim=10)
    obs, lat = torch.randn(3, O), torch.randn(3, 10)
    for call in (lambda: ac.act_inference(obs), lambda: ac.update_distribution(obs), lambda: ac.act(obs), lambda: ac._actor_input(obs)):
        with pytest.raises(ValueError, match="no depth latent"):
            call()
    for bad in (torch.randn(3, 9), torch.randn(4, 10), torch.randn(30)):
        with pytest.raises(ValueError, match="depth latent must be"):
            ac.act_inference(obs, bad)
    with ac.bound_latent(lat):
        ac.act_inference(obs)
    with pytest.raises(ValueError, match="no depth latent"):       # the binding ends with its block
        ac.act_inference(obs)


def test_minibatches_carry_the_latent_rows_of_the_same_permutation():
    torch.manual_seed(2)
    T, N, L = 4, 8, 10
    st = V.VisionRolloutStorage(N, T, [O], [P], [A], L, "cpu")
    tr = st.Transition()
    for t in range(T):
        tr.observations = torch.randn(N, O)
        tr.observations[:, 0] = torch.arange(t * N, (t + 1) * N)         # the flat row index travels with the row
        tr.critic_observations, tr.next_critic_observations = torch.randn(N, P), torch.randn(N, P)
        tr.actions, tr.action_mean, tr.action_sigma = torch.randn(N, A), torch.randn(N, A), torch.rand(N, A)
        tr.rewards, tr.dones, tr.values, tr.actions_log_prob = torch.randn(N), torch.zeros(N, dtype=torch.bool), torch.randn(N, 1), torch.randn(N)
        tr.depth_latent = torch.randn(N, L)
        st.add_transitions(tr)
    assert st.step == T and st.depth_latent.shape == (T, N, L)
    tr.depth_latent = None
    st.step = 0
    with pytest.raises(ValueError, match="no depth latent"):
        st.add_transitions(tr)
    assert st.step == 0
    batches = list(st.mini_batch_generator(2, num_epochs=2))
    assert len(batches) == 4 and all(len(b) == 11 for b in batches)
    perm = torch.cat([b[0][:, 0] for b in batches[:2]]).long()
    assert sorted(perm.tolist()) == list(range(T * N))
    got = torch.cat([b[10] for b in batches[:2]])
    assert torch.equal(got, st.depth_latent.flatten(0, 1)[perm])
    assert torch.equal(torch.cat([b[2] for b in batches[:2]]), st.actions.flatten(0, 1)[perm])
    assert torch.equal(torch.cat([b[10] for b in batches[2:]]), got)        # one permutation for every epoch


def _rollout(alg, T, N, seed):
    g = torch.Generator().manual_seed(seed)
    obs, crit = torch.randn(N, O, generator=g), torch.randn(N, P, generator=g)
    for _ in range(T):
        alg.act(obs, crit)
        obs, nxt = torch.randn(N, O, generator=g), torch.randn(N, P, generator=g)
        alg.process_env_step(torch.randn(N, generator=g), torch.zeros(N, dtype=torch.bool), {}, nxt)
        crit = nxt
    alg.compute_returns(crit)


def test_ppo_update_trains_the_depth_columns_and_leaves_the_encoder_alone():
    torch.manual_seed(3)
    T, N, L = 4, 8, 10
    ac = V.VisionActorCritic(O, P, N1, A, depth_latent_dim=L)
    enc = _small_encoder(L)
    latent, frames = torch.randn(N, L), torch.randn(N, 2, 12, 16)
    alg = V.VisionPPO(ac, encoder=enc, latent_source=lambda: latent, frames_source=lambda: frames, num_learning_epochs=2, num_mini_batches=2, device="cpu")
    assert alg.height_scan == (P - 187, 187)
    assert not {id(p) for p in enc.parameters()} & {id(p) for g in alg.optimizer.param_groups for p in g["params"]}
    alg.init_storage(N, T, [O], [P], [A])
    assert alg.snapshot_steps() == [0, 1, 2, 3]
    _rollout(alg, T, N, 0)
    assert torch.equal(alg.storage.depth_latent, latent.expand(T, N, L))
    w0 = ac.actor[0].weight.detach().clone()
    enc0 = [p.detach().clone() for p in enc.parameters()]
    out = HIMPPO.update(alg)                        # the PPO half
    assert len(out) == 4 and all(v == v for v in out)
    g = ac.actor[0].weight.grad
    assert g is not None and g[:, K_HIM:].abs().max() > 0
    assert (ac.actor[0].weight[:, K_HIM:] != w0[:, K_HIM:]).any()
    assert all(p.grad is None for p in enc.parameters()) and all(p.grad is None for p in alg.depth_head.parameters())
    assert all(torch.equal(p, q) for p, q in zip(enc.parameters(), enc0))
    aux = alg.encoder_step()                        # the encoder's half
    assert torch.isfinite(aux) and all(p.grad is not None for p in enc.parameters())
    assert all((p != q).any() for p, q in zip(enc.parameters(), enc0))
    assert alg.encoder_step() is None               # the snapshots are consumed
    _rollout(alg, T, N, 1)
    out = alg.update()
    assert len(out) == 5 and out[4] == out[4] and out[4] == alg.last_aux_loss
    alg.latent_source = None
    with pytest.raises(RuntimeError, match="latent source"):
        alg.act(torch.randn(N, O), torch.randn(N, P))


def test_snapshots_are_spread_over_the_rollout():
    ac = V.VisionActorCritic(O, P, N1, A, depth_latent_dim=10)
    alg = V.VisionPPO(ac, device="cpu")
    alg.init_storage(2, 100, [O], [P], [A])
    assert alg.aux_snapshots == 4 and alg.snapshot_steps() == [12, 37, 62, 87]
    alg.init_storage(2, 6, [O], [P], [A])
    assert alg.snapshot_steps() == [0, 2, 3, 5]
    alg.init_storage(2, 2, [O], [P], [A])
    assert alg.snapshot_steps() == [0, 1]


def test_more_than_one_rank_and_a_config_without_height_scan_raise():
    ac = V.VisionActorCritic(O, P, N1, A, depth_latent_dim=10)
    with pytest.raises(NotImplementedError):
        V.VisionPPO(ac, device="cpu", dist_ctx=types.SimpleNamespace(world=2, enabled=True))
    cfg = types.SimpleNamespace(terrain=types.SimpleNamespace(measure_heights=False))
    with pytest.raises(ValueError, match="measure_heights"):
        V.height_scan_block(cfg)
    cfg.terrain.measure_heights = True
    assert V.height_scan_block(cfg) == (abi.DEFINES["LSIM_NUM_PRIV_OBS"] - abi.DEFINES["LSIM_NUM_HEIGHT_PTS"], abi.DEFINES["LSIM_NUM_HEIGHT_PTS"])
    with pytest.raises(ValueError, match="latent"):
        V.VisionPPO(ac, encoder=_small_encoder(12), latent_source=lambda: None, frames_source=lambda: None, device="cpu")


def test_encoder_step_reduces_the_regression_loss():
    """64 samples, 187 targets that are a fixed function of the newest frame, 30 Adam steps through VisionPPO.encoder_step: the loss falls at
    every step and ends at or below 0.95 x its first value (plain torch: 0.90-0.91; the cap only keeps a dead optimiser from passing)"""
    torch.manual_seed(4)
    B, L = 64, 10
    ac = V.VisionActorCritic(O, P, N1, A, depth_latent_dim=L)
    frames = 0.5 * torch.rand(B, 2, 12, 16) - 0.25
    mix = torch.randn(12 * 16, 187) / (12 * 16) ** 0.5
    crit = torch.zeros(B, P)
    crit[:, P - 187:] = torch.tanh(4.0 * frames[:, -1].flatten(1) @ mix)
    alg = V.VisionPPO(ac, encoder=_small_encoder(L), latent_source=lambda: None, frames_source=lambda: frames, aux_snapshots=1, device="cpu")
    alg.init_storage(B, 1, [O], [P], [A])
    losses = []
    for _ in range(30):
        alg.snapshot_if_due(0, crit)
        losses.append(float(alg.encoder_step()))
    print("encoder-step losses:", losses[0], losses[-1], losses[-1] / losses[0])
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert losses[-1] <= 0.95 * losses[0], losses


# ---- the C-ABI's refusals: on the host, before any HIP call, so they are checked without a device
def _fake_policy(L, ptr=0x10000):
    ac = V.VisionActorCritic(O, P, N1, A, depth_latent_dim=L) if L else HIMActorCritic(O, P, N1, A)
    lin = lambda seq: [m for m in seq if isinstance(m, torch.nn.Linear)]
    pol = abi.LsimHimPolicy()
    pad = lambda v: (v + 15) // 16 * 16
    for dst, layers in ((pol.encoder, lin(ac.estimator.encoder)), (pol.actor, lin(ac.actor)), (pol.critic, lin(ac.critic))):
        for d, l in zip(dst, layers):
            d.weight, d.bias = ptr, ptr
            d.k_pad, d.n_pad, d.k_in, d.n_out = pad(l.in_features), pad(l.out_features), l.in_features, l.out_features
    pol.num_obs, pol.num_priv_obs, pol.num_one_step_obs, pol.num_actions = O, P, N1, A
    return pol


def _extra(dim, ld, rows=0x10000, store=None):
    x = abi.LsimPolicyExtra()
    x.rows, x.dim, x.ld, x.store = rows, dim, ld, store
    return x


def _fake_storage(T=3, N=37, ptr=0x10000):
    S = abi.LsimRolloutStorage()
    for k in ("observations", "privileged_observations", "next_privileged_observations", "actions", "values", "actions_log_prob", "mu", "sigma",
              "rewards", "dones"):
        setattr(S, k, ptr)
    S.num_steps, S.num_envs, S.num_obs, S.num_priv_obs, S.num_actions = T, N, O, P, A
    return S


def test_entry_points_refuse_bad_arguments_on_the_host():
    Lb = lib.load()                     # loads without a device
    INV, UNS = abi.E_INVALID, abi.E_UNSUPPORTED
    assert INV != 0 and UNS != 0 and INV != UNS
    p = 0x10000
    pol, S = _fake_policy(10), _fake_storage()
    ref = ctypes.byref

    def fwd(pol_, x, obs=p, priv=p, n=37, mean=p, val=p):
        return Lb.lsim_policy_forward_ext(ref(pol_) if pol_ is not None else None, ref(x) if x is not None else None, obs, priv, n, mean, val, None)

    def act(pol_, x, st=S, step=1, obs=p, std=p, actions=p, prev=-1, dones=None, rew=None, term=None):
        return Lb.lsim_policy_act_post_at_ext(ref(pol_) if pol_ is not None else None, ref(x) if x is not None else None, ref(st) if st is not None else None,
                                              step, 0, obs, p, std, 1, 0, p, p, actions, prev, dones, None, rew, term, 0.99, None)
    for call in (fwd, act):
        assert call(pol, None) == INV                               # a null struct
        assert call(pol, _extra(10, 12, rows=None)) == INV          # null rows
        assert call(pol, _extra(0, 12)) == INV                      # dim < 1
        assert call(pol, _extra(-3, 12)) == INV
        assert call(pol, _extra(10, 9)) == INV                      # ld < dim
        assert call(pol, _extra(9, 12)) == UNS                      # actor[0].k_in != n1 + 3 + nl + dim
        assert call(pol, _extra(11, 12)) == UNS
        assert call(_fake_policy(0), _extra(10, 12)) == UNS         # a HIM policy has no columns for the rows
        assert call(_fake_policy(240), _extra(240, 240)) == UNS     # k_in 304: k_pad above the 272 columns of the LDS buffer
        assert call(None, _extra(10, 12)) == INV                    # what the plain entries refuse
        assert call(pol, _extra(10, 12), obs=None) == INV
        wide = _fake_policy(10)
        wide.encoder[1].n_pad = 288                                 # lands in the narrower LDS buffer
        assert call(wide, _extra(10, 12)) == UNS
    assert fwd(pol, _extra(10, 12), n=0) == INV
    assert act(pol, _extra(10, 12), st=None) == INV
    assert act(pol, _extra(10, 12), std=None) == INV
    assert act(pol, _extra(10, 12), step=3) == INV and act(pol, _extra(10, 12), step=-1) == INV
    assert act(pol, _extra(10, 12), prev=3, dones=p, rew=p, term=p) == INV          # prev_step past the storage
    assert act(pol, _extra(10, 12), prev=0) == INV                                  # a previous step without its buffers
    odd = _fake_storage()
    odd.num_obs = O + 2
    assert act(pol, _extra(10, 12), st=odd) == INV
    # the plain entries go on refusing a policy whose first actor layer is wider
    assert Lb.lsim_policy_forward(ref(pol), p, p, 37, p, p, None) == UNS
    assert Lb.lsim_policy_act_post_at(ref(pol), ref(S), 1, 0, p, p, p, 1, 0, p, p, p, -1, None, None, None, None, 0.99, None) == UNS


def test_struct_mirror_follows_the_header():
    names = [f[0] for f in abi.LsimPolicyExtra._fields_]
    assert names == ["rows", "dim", "ld", "store"]
    assert ctypes.sizeof(abi.LsimPolicyExtra) == 24
    for fn in ("lsim_policy_forward_ext", "lsim_policy_act_post_at_ext"):
        assert abi.PROTOTYPES[fn][1][1] == ctypes.POINTER(abi.LsimPolicyExtra)


def test_checkpoint_round_trips_encoder_head_and_their_optimiser(tmp_path):
    torch.manual_seed(5)

    def hand_built(seed):
        torch.manual_seed(seed)
        L = 10
        ac = V.VisionActorCritic(O, P, N1, A, depth_latent_dim=L)
        frames = torch.randn(8, 2, 12, 16)
        alg = V.VisionPPO(ac, encoder=_small_encoder(L), latent_source=lambda: None, frames_source=lambda: frames, aux_snapshots=1, device="cpu")
        alg.init_storage(8, 1, [O], [P], [A])
        run = V.VisionOnPolicyRunner.__new__(V.VisionOnPolicyRunner)
        run.alg, run.env, run.device, run.graphs = alg, types.SimpleNamespace(), "cpu", None
        run.dist_ctx = types.SimpleNamespace(enabled=False)
        run.current_learning_iteration = 7
        return run, alg
    run, alg = hand_built(10)
    for _ in range(2):                                           # Adam moments of encoder and head
        alg.snapshot_if_due(0, torch.randn(8, P))
        alg.encoder_step()
    path = os.path.join(str(tmp_path), "model.pt")
    run.save(path)
    d = torch.load(path, map_location="cpu", weights_only=False)
    assert {"model_state_dict", "optimizer_state_dict", "estimator_optimizer_state_dict", "iter", "infos"} <= set(d)       # the reference's keys
    assert set(d["model_state_dict"]) == set(alg.actor_critic.state_dict()) and not any("depth" in k for k in d["model_state_dict"])
    assert len(d["optimizer_state_dict"]["param_groups"][0]["params"]) == len(list(alg.actor_critic.parameters()))
    run2, alg2 = hand_built(11)
    assert not torch.equal(alg2.encoder.fc.weight, alg.encoder.fc.weight)
    assert run2.load(path) is None and run2.current_learning_iteration == 7
    for a, b in ((alg.encoder, alg2.encoder), (alg.depth_head, alg2.depth_head), (alg.actor_critic, alg2.actor_critic)):
        sa, sb = a.state_dict(), b.state_dict()
        assert set(sa) == set(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    oa, ob = alg.aux_optimizer.state_dict(), alg2.aux_optimizer.state_dict()
    assert len(oa["state"]) == 8 and set(oa["state"]) == set(ob["state"])
    for k in oa["state"]:
        for name in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(torch.as_tensor(oa["state"][k][name]), torch.as_tensor(ob["state"][k][name]))
    # both continue identically from the checkpoint
    crit = torch.randn(8, P)
    for a in (alg, alg2):
        a.snapshot_if_due(0, crit)
    alg2.frames_source = alg.frames_source
    alg2.snapshot_if_due(0, crit)
    assert float(alg.encoder_step()) == float(alg2.encoder_step())
