"""GPU: the fused rollout launch with the extra actor-input segment (lsim_policy_forward_ext / lsim_policy_act_post_at_ext) against torch, against
the plain launch on a warm-started twin (bit for bit) and against its own two-launch form; the latent store; a vision policy end to end."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
O, P, N1, A = 270, 238, 45, 12          # the policy of tests/test_gpu_learner.py
K_HIM = N1 + 3 + 16
SIZES = [37, 2053]                      # the 16-row kernel with a ragged last block; the 32-row kernel (from 2048 envs) with one
FIELDS = (("observations", O), ("privileged_observations", P), ("next_privileged_observations", P), ("actions", A), ("values", 1),
          ("actions_log_prob", 1), ("mu", A), ("sigma", A), ("rewards", 1))


def _perturb(module, scale=0.05):
    with torch.no_grad():
        for p in module.parameters():
            p.add_(scale * torch.randn_like(p))


def _storage(T, N):
    from isaacgymloco_amd import abi
    st = {k: torch.zeros(T, N, d, device=DEV) for k, d in FIELDS}
    st["dones"] = torch.zeros(T, N, 1, device=DEV, dtype=torch.uint8)
    S = abi.LsimRolloutStorage()
    for k, t in st.items():
        setattr(S, k, t.data_ptr())
    S.num_steps, S.num_envs, S.num_obs, S.num_priv_obs, S.num_actions = T, N, O, P, A
    return st, S


def _outputs(N):
    return torch.zeros(N, A, device=DEV), torch.zeros(N, 1, device=DEV), torch.zeros(N, A, device=DEV)


def _rows(N, L, ld, scale=1.0):
    """[N, L] view with row stride ld of a buffer whose other columns are NaN: a launch that read them would show it"""
    buf = torch.full((N, ld), float("nan"), device=DEV)
    buf[:, :L] = scale * torch.randn(N, L, device=DEV)
    return buf[:, :L]


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("L,ld", [(64, 64), (10, 12)])
@pytest.mark.parametrize("N", SIZES)
def test_forward_ext_matches_torch(N, L, ld):
    """(10, 12): k_in 74, k_pad 80, a latent stride that is not the width.  Tolerance of test_fused_policy_forward_matches_torch."""
    from isaacgymloco_amd.learn.vision import PackedVisionPolicy, VisionActorCritic
    torch.manual_seed(3 + N + L)
    ac = VisionActorCritic(O, P, N1, A, depth_latent_dim=L).to(DEV)
    _perturb(ac)
    assert PackedVisionPolicy.supported(ac)
    pk = PackedVisionPolicy(ac)
    assert pk._P.actor[0].k_in == K_HIM + L and pk._P.actor[0].k_pad == (K_HIM + L + 15) // 16 * 16
    obs, priv, rows = 2.0 * torch.randn(N, O, device=DEV), 2.0 * torch.randn(N, P, device=DEV), _rows(N, L, ld, 2.0)
    mean, val = torch.empty(N, A, device=DEV), torch.empty(N, 1, device=DEV)
    for change in (False, True):
        if change:                                       # an optimiser-like change of the first actor layer, then refresh()
            with torch.no_grad():
                ac.actor[0].weight.add_(0.02 * torch.randn_like(ac.actor[0].weight))
            pk.refresh()
        pk.forward(obs, priv, mean, val, rows=rows)
        with torch.no_grad():
            ac.update_distribution(obs, rows)
            ref_mean, ref_val = ac.action_mean, ac.evaluate(priv)
            vel, z = ac.estimator(obs)
            stated = ac.actor(torch.cat((obs[:, :N1], vel, z, rows), dim=-1))
        print("N", N, "L", L, "max |mean - ref|", float((mean - ref_mean).abs().max()), "scale", float(ref_mean.abs().max()))
        torch.testing.assert_close(ref_mean, stated, rtol=2e-4, atol=2e-5 * float(stated.abs().max()))
        torch.testing.assert_close(mean, ref_mean, rtol=2e-4, atol=2e-5 * float(ref_mean.abs().max()))
        torch.testing.assert_close(val, ref_val, rtol=2e-4, atol=2e-5 * float(ref_val.abs().max()))
    other = torch.empty(N, A, device=DEV)                # the depth columns matter: other rows, other means
    pk.forward(obs, priv, other, val, rows=_rows(N, L, ld, 2.0))
    assert not torch.equal(other, mean)


def _twins(L):
    from isaacgymloco_amd.learn.fused_policy import PackedHimPolicy
    from isaacgymloco_amd.learn.modules import HIMActorCritic
    from isaacgymloco_amd.learn.vision import PackedVisionPolicy, VisionActorCritic
    him = HIMActorCritic(O, P, N1, A).to(DEV)
    _perturb(him)
    vis = VisionActorCritic(O, P, N1, A, depth_latent_dim=L).to(DEV)
    vis.load_him_state_dict(him.state_dict())
    return PackedHimPolicy(him), PackedVisionPolicy(vis)


@pytest.mark.parametrize("N", SIZES)
def test_warm_started_twin_equals_the_plain_launch_bit_for_bit(N):
    """a HIM policy and its warm-started vision twin: the extra products are exact zeros, so means, values, actions and all ten storage tensors
    of the ext act launch equal lsim_policy_act_post_at's, with and without a previous step's post-step store"""
    torch.manual_seed(N)
    for L, ld in ((64, 64), (10, 12)):
        pk_h, pk_v = _twins(L)
        T = 3
        obs, priv, std = torch.randn(N, O, device=DEV), torch.randn(N, P, device=DEV), torch.rand(A, device=DEV) + 0.3
        obs_n, priv_n, term = torch.randn(N, O, device=DEV), torch.randn(N, P, device=DEV), torch.randn(N, P, device=DEV)
        dones = torch.rand(N, device=DEV) < 0.3
        touts = dones & (torch.rand(N, device=DEV) < 0.5)
        rew = torch.randn(N, device=DEV)
        rows, rows_n = _rows(N, L, ld, 50.0), _rows(N, L, ld, 50.0)
        sth, Sh = _storage(T, N)
        stv, Sv = _storage(T, N)
        mh, vh, ah = _outputs(N)
        mv, vv, av = _outputs(N)
        pk_h.forward_act(Sh, 0, 3, obs, priv, std, 5, 1, mh, vh, ah)                      # no previous step
        pk_v.forward_act(Sv, 0, 3, obs, priv, std, 5, 1, mv, vv, av, rows=rows)
        torch.cuda.synchronize()
        assert torch.equal(_bits(mv), _bits(mh)) and torch.equal(_bits(vv), _bits(vh)) and torch.equal(_bits(av), _bits(ah)), (N, L)
        pk_h.forward_act(Sh, 1, 4, obs_n, priv_n, std, 5, 1, mh, vh, ah, prev=(0, dones, touts, rew, term, 0.99))
        pk_v.forward_act(Sv, 1, 4, obs_n, priv_n, std, 5, 1, mv, vv, av, prev=(0, dones, touts, rew, term, 0.99), rows=rows_n)
        torch.cuda.synchronize()
        assert torch.equal(_bits(mv), _bits(mh)) and torch.equal(_bits(vv), _bits(vh)) and torch.equal(_bits(av), _bits(ah)), (N, L)
        for k in sth:
            assert torch.equal(stv[k], sth[k]), (N, L, k)
        assert stv["dones"][0].sum() > 0 and stv["next_privileged_observations"][0].abs().sum() > 0 and stv["actions"][1].abs().sum() > 0
        assert stv["observations"][2].abs().sum() == 0
        # and the forward-only pair
        pk_h.forward(obs, priv, mh, vh)
        pk_v.forward(obs, priv, mv, vv, rows=rows)
        assert torch.equal(_bits(mv), _bits(mh)) and torch.equal(_bits(vv), _bits(vh))


@pytest.mark.parametrize("N", SIZES)
def test_latent_store_receives_the_rows_and_nothing_else(N):
    from isaacgymloco_amd.learn.vision import PackedVisionPolicy, VisionActorCritic
    torch.manual_seed(7 + N)
    L, ld, T, step = 10, 12, 3, 1
    ac = VisionActorCritic(O, P, N1, A, depth_latent_dim=L).to(DEV)
    pk = PackedVisionPolicy(ac)
    obs, priv, std, rows = torch.randn(N, O, device=DEV), torch.randn(N, P, device=DEV), torch.rand(A, device=DEV) + 0.3, _rows(N, L, ld)
    flat = torch.full(((T + 1) * N * L,), float("nan"), device=DEV)          # the tensor and a guard row of the same size behind it
    store, guard = flat[:T * N * L].view(T, N, L), flat[T * N * L:]
    st, S = _storage(T, N)
    m, v, a = _outputs(N)
    pk.forward_act(S, step, 9, obs, priv, std, 5, 1, m, v, a, rows=rows, store=None)      # store = NULL writes none
    torch.cuda.synchronize()
    assert bool(torch.isnan(flat).all()) and st["actions"][step].abs().sum() > 0
    pk.forward_act(S, step, 9, obs, priv, std, 5, 1, m, v, a, rows=rows, store=store)
    torch.cuda.synchronize()
    assert torch.equal(_bits(store[step]), _bits(rows))
    assert bool(torch.isnan(store[0]).all()) and bool(torch.isnan(store[2]).all()) and bool(torch.isnan(guard).all())


@pytest.mark.parametrize("N", SIZES)
def test_ext_act_in_one_launch_equals_forward_ext_then_act(N):
    """as test_policy_act_in_one_launch_equals_forward_then_act does for the plain pair: identical bits"""
    from isaacgymloco_amd import lib
    from isaacgymloco_amd.learn.vision import PackedVisionPolicy, VisionActorCritic
    Lb = lib.load()
    torch.manual_seed(11 + N)
    L, ld, T = 64, 64, 3
    ac = VisionActorCritic(O, P, N1, A, depth_latent_dim=L).to(DEV)
    _perturb(ac)
    pk = PackedVisionPolicy(ac)
    obs, priv, std, rows = torch.randn(N, O, device=DEV), torch.randn(N, P, device=DEV), torch.rand(A, device=DEV) + 0.3, _rows(N, L, ld)
    s = torch.cuda.current_stream().cuda_stream
    st1, S1 = _storage(T, N)
    m1, v1, a1 = _outputs(N)
    pk.forward(obs, priv, m1, v1, rows=rows)
    assert Lb.lsim_rollout_act_at(ctypes.byref(S1), 2, 11, m1.data_ptr(), std.data_ptr(), v1.data_ptr(), obs.data_ptr(), priv.data_ptr(), 5, 1,
                                  a1.data_ptr(), s) == 0
    st2, S2 = _storage(T, N)
    m2, v2, a2 = _outputs(N)
    pk.forward_act(S2, 2, 11, obs, priv, std, 5, 1, m2, v2, a2, rows=rows)
    torch.cuda.synchronize()
    assert torch.equal(_bits(m2), _bits(m1)) and torch.equal(_bits(v2), _bits(v1)) and torch.equal(_bits(a2), _bits(a1))
    for k in st1:
        assert torch.equal(st2[k], st1[k]), (N, k)
    assert st2["actions"][2].abs().sum() > 0 and st2["observations"][0].abs().sum() == 0


def _make_vision(seed, T=6):
    from isaacgymloco_amd.envs import config as C
    from isaacgymloco_amd.envs import sensors
    from isaacgymloco_amd.envs.legged_robot import LeggedRobot
    from isaacgymloco_amd.learn.bench_train import train_cfg_dict
    from isaacgymloco_amd.learn.depth_encoder import DepthEncoder
    from isaacgymloco_amd.learn.vision import VisionOnPolicyRunner
    cfg = C.aliengo_cfg()
    cfg.env.num_envs = 64
    cfg.terrain.terrain_proportions = [1.0, 0.0, 0.0, 0.0]
    env = LeggedRobot(cfg, sim_device=DEV, seed=seed)
    cam = env.add_sensor("depth", sensors.depth_camera(env, 16, 12, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0,
                                                       model=sensors.SensorModel(period=3, stagger=True, latency=1, frames=2, normalise=True)))
    tc = train_cfg_dict("aliengo")
    tc["runner"]["num_steps_per_env"] = T
    torch.manual_seed(seed)
    enc = DepthEncoder(12, 16, 2, c1=4, k1=3, s1=2, c2=8, k2=3, s2=1, latent_dim=10)
    return env, cam, VisionOnPolicyRunner(env, tc, sensor="depth", encoder=enc, device=DEV)


def test_vision_policy_end_to_end(tmp_path):
    from isaacgymloco_amd.learn.vision import VisionRollout
    T, L = 6, 10
    env, cam, run = _make_vision(5, T)
    ac, alg = run.alg.actor_critic, run.alg
    assert run.enable_graphs() and isinstance(run.graphs, VisionRollout)
    assert cam.latent().shape == (64, L) and alg.storage.depth_latent.shape == (T, 64, L)
    env.episode_length_buf[:9] = int(env.max_episode_length) - 3           # these time out, and reset, inside the rollout
    seen = []
    with torch.inference_mode():
        for t in range(T):
            seen.append(cam.latent().clone())
            run.graphs.step()
    run.graphs.flush()
    torch.cuda.synchronize()
    st = alg.storage
    assert int(st.dones.sum()) >= 9
    assert len({int(_bits(s).sum()) for s in seen}) > 1                     # the latent moved during the rollout
    for t in range(T):
        assert torch.equal(_bits(st.depth_latent[t]), _bits(seen[t])), t
        with torch.no_grad():
            ref = ac.act_inference(st.observations[t], st.depth_latent[t])
        torch.testing.assert_close(st.mu[t], ref, rtol=2e-4, atol=2e-5 * float(ref.abs().max()))
    assert all(alg._snap_filled) and len(alg._snap) == 4
    run.graphs.end_iteration()
    st.clear()
    before = {k: v.clone() for k, v in ac.state_dict().items()}
    enc_before = [p.detach().clone() for p in alg.encoder.parameters()]
    run.learn(2)
    assert len(run.last_update) == 5 and run.last_update[4] == run.last_update[4]
    after = ac.state_dict()
    assert all(bool(torch.isfinite(v).all()) for v in after.values())
    assert all(bool(torch.isfinite(p).all()) for p in list(alg.encoder.parameters()) + list(alg.depth_head.parameters()))
    assert (after["actor.0.weight"][:, K_HIM:] != before["actor.0.weight"][:, K_HIM:]).any()
    assert all((p != q).any() for p, q in zip(alg.encoder.parameters(), enc_before))
    assert int(env.nonfinite_envs) == 0
    path = str(tmp_path / "vision.pt")
    run.save(path)
    env2, cam2, run2 = _make_vision(6, T)
    run2.load(path)
    for a, b in ((alg.encoder, run2.alg.encoder), (alg.depth_head, run2.alg.depth_head), (ac, run2.alg.actor_critic)):
        sa, sb = a.state_dict(), b.state_dict()
        assert all(torch.equal(sa[k], sb[k]) for k in sa)
    run2.learn(1)                                       # before enable_graphs(): the eager rollout (VisionPPO.act) and the same update
    assert run2.graphs is None and run2.alg.storage.depth_latent.abs().sum() > 0
    assert run2.enable_graphs()
    run2.learn(1)
    assert all(bool(torch.isfinite(v).all()) for v in run2.alg.actor_critic.state_dict().values()) and int(env2.nonfinite_envs) == 0
