"""GPU: lsim_policy_forward and its ext / act-post forms (csrc/ls_policy.h) at the widths of tests/mlp_shapes_reference.py -- every split of the
output tiles over 8 and 16 waves, the predicated layer form, every shape of the k loop -- against the fp64 numpy reference: exact integer scenes
bit for bit, general scenes within 4 x the distance of the reference's fp32 twins (tests/mlp_shapes_rig.py).  The networks reach the library
through the reference's own packer; PackedHimPolicy / PackedVisionPolicy are pinned against it."""
import ctypes

import numpy as np
import pytest
import torch

import mlp_shapes_reference as R
import mlp_shapes_rig as G

pytestmark = pytest.mark.gpu
DEV = G.DEV
POLICY = list(R.POLICY_CASES)


@pytest.mark.parametrize("n", R.POLICY_ENVS)
@pytest.mark.parametrize("case", POLICY)
def test_exact_scene_bit_for_bit(case, n):
    """integer weights, biases and inputs with every partial sum below 2^24 (asserted in int64 for this batch): means and values to the bit,
    again after an in-place change of the weights and a re-pack into the same device buffers"""
    net, obs, priv, extra = R.exact_policy_scene(case, n)
    mean, val = R.check_exact_policy(case, net, obs, priv, extra)
    pk = G.DevicePolicy(case, net)
    got = pk.forward(obs, priv, extra)
    assert np.array_equal(got[0], mean.astype(np.float32)) and np.array_equal(got[1], val.astype(np.float32)), (case, n)
    # other weights at the same addresses: the first actor and critic layers with another bias and their outputs' rows reversed
    net2 = {k: [(W.copy(), b.copy()) for W, b in v] for k, v in net.items()}
    for name in ("actor", "critic"):
        W, b = net2[name][0]
        net2[name][0] = (W[::-1].copy(), b[::-1] + 2)
    mean2, val2 = R.check_exact_policy(case, net2, obs, priv, extra)
    assert not np.array_equal(mean2, mean) and not np.array_equal(val2, val)
    pk.repack(net2)
    got = pk.forward(obs, priv, extra)
    assert np.array_equal(got[0], mean2.astype(np.float32)) and np.array_equal(got[1], val2.astype(np.float32)), (case, n, "re-packed")


@pytest.mark.parametrize("zero_latent", [False, True])
@pytest.mark.parametrize("n", R.POLICY_ENVS)
@pytest.mark.parametrize("case", POLICY)
def test_general_scene_within_the_twins_tolerance(case, n, zero_latent):
    """zero_latent: the encoder's latent rows and biases are zero, the normalisation is 0 / max(0, 1e-12) = 0, not NaN"""
    sc = G.general_policy_scene(case, zero_latent)
    pk = G.DevicePolicy(case, sc["net"])
    ext = None if sc["extra"] is None else sc["extra"][:n]
    got = pk.forward(sc["obs"][:n], sc["priv"][:n], ext)
    for i, what in enumerate(("mean", "values")):
        err = float(np.abs(got[i].astype(np.float64) - sc["ref"][i][:n]).max())
        print(case, n, what, "max |device - fp64|", err, "tolerance", sc["tol"][i], "twin distance", sc["twin_dist"][i])
        assert np.isfinite(got[i]).all() and err <= sc["tol"][i], (case, n, what, err, sc["tol"][i])


def _act_case(case):
    """the storage kernels copy rows as float2 (include/lsim.h: row sizes even), so lsim_rollout_act_at and with it the one-launch forms refuse an
    odd observation width: `tiny` (P = 7) and `ragged` (O = 87) are asserted to be refused by both, and stand in with P = 8 and O = 116 = 4 x 29"""
    c = dict(R.POLICY_CASES[case])
    if case == "tiny":
        c["P"] = 8
    if case == "ragged":
        c["hist"] = 4
    return c


@pytest.mark.parametrize("n", R.POLICY_ENVS)
@pytest.mark.parametrize("case", POLICY)
def test_act_post_in_one_launch_equals_the_separate_calls(case, n, monkeypatch):
    """lsim_policy_act_post_at / _ext against forward + lsim_rollout_act_at + lsim_rollout_post_at: means, values, actions and all ten storage
    tensors bit for bit, a guard row behind each; A = 1 (tiny), 5 (ext), 12 and 16 (ragged)"""
    from isaacgymloco_amd import abi
    odd = R.POLICY_CASES[case]
    c = _act_case(case)
    O, P, A, T = c["hist"] * c["n1"], c["P"], c["A"], 3
    s = torch.cuda.current_stream().cuda_stream
    if c != odd:                                   # the case at its own, odd width: refused by the host checks of both forms
        pk = G.DevicePolicy(case, R.exact_policy_scene(case, n)[0])
        st, gd, S = G.storage(T, n, odd["hist"] * odd["n1"], odd["P"], A)
        z = torch.zeros(n, max(odd["hist"] * odd["n1"], odd["P"], A), device=DEV)
        assert pk.L.lsim_policy_act_post_at(ctypes.byref(pk.P), ctypes.byref(S), 0, 3, z.data_ptr(), z.data_ptr(), z.data_ptr(), 5, 1, z.data_ptr(), z.data_ptr(),
                                            z.data_ptr(), -1, None, None, None, None, ctypes.c_float(0.99), s) == abi.E_UNSUPPORTED
        assert pk.L.lsim_rollout_act_at(ctypes.byref(S), 0, 3, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 5, 1, z.data_ptr(), s) == abi.E_UNSUPPORTED
        torch.cuda.synchronize()
        assert all(float(t.float().abs().sum()) == 0 for t in st.values()) and G.storage_guards_intact(gd)
    monkeypatch.setitem(R.POLICY_CASES, case, c)
    ac = G.policy_module(case, seed=40 + n)
    pk = G.DevicePolicy(case, G.net_of(ac))
    L = pk.L
    g = torch.Generator().manual_seed(n)
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(DEV)
    obs, priv, obs_n, priv_n, term, rew = rnd(n, O), rnd(n, P), rnd(n, O), rnd(n, P), rnd(n, P), rnd(n)
    std = (torch.rand(A, generator=g) + 0.3).to(DEV)
    dones = (torch.rand(n, generator=g) < 0.3).to(DEV)
    touts = dones & (torch.rand(n, generator=g) < 0.5).to(DEV)
    dones[0] = touts[0] = True                     # a single row still takes the terminal patch and the time-out bootstrap
    ext = ext_n = None
    if c["ext"]:
        ext, ext_n = (torch.full((n, c["ext"][1]), float("nan"), device=DEV) for _ in range(2))
        ext[:, :c["ext"][0]], ext_n[:, :c["ext"][0]] = rnd(n, c["ext"][0]), rnd(n, c["ext"][0])
    outs = lambda: (torch.zeros(n, A, device=DEV), torch.zeros(n, 1, device=DEV), torch.zeros(n, A, device=DEV))

    def fused(S, step, draw, o, p, x, m, v, a, prev_step):
        tail = (int(prev_step), dones.data_ptr(), touts.data_ptr(), rew.data_ptr(), term.data_ptr(), ctypes.c_float(0.99), s)
        head = (ctypes.byref(S), step, draw, o.data_ptr(), p.data_ptr(), std.data_ptr(), 5, 1, m.data_ptr(), v.data_ptr(), a.data_ptr())
        if c["ext"]:
            return L.lsim_policy_act_post_at_ext(ctypes.byref(pk.P), ctypes.byref(pk.extra_struct(x)), *head, *tail)
        return L.lsim_policy_act_post_at(ctypes.byref(pk.P), *head, *tail)

    # A: forward, act, post, forward, act as separate launches; B: two one-launch calls, the second carrying the first step's post-step store
    stA, gA, SA = G.storage(T, n, O, P, A)
    stB, gB, SB = G.storage(T, n, O, P, A)
    mA, vA, aA = outs()
    mB, vB, aB = outs()
    for step, draw, o, p, x in ((0, 3, obs, priv, ext), (1, 4, obs_n, priv_n, ext_n)):
        assert pk.forward_rc(o, p, mA, vA, x) == 0
        assert L.lsim_rollout_act_at(ctypes.byref(SA), step, draw, mA.data_ptr(), std.data_ptr(), vA.data_ptr(), o.data_ptr(), p.data_ptr(), 5, 1, aA.data_ptr(), s) == 0
        if step == 0:
            assert L.lsim_rollout_post_at(ctypes.byref(SA), 0, dones.data_ptr(), touts.data_ptr(), rew.data_ptr(), vA.data_ptr(), priv_n.data_ptr(), term.data_ptr(),
                                          ctypes.c_float(0.99), s) == 0
    assert fused(SB, 0, 3, obs, priv, ext, mB, vB, aB, -1) == 0
    assert fused(SB, 1, 4, obs_n, priv_n, ext_n, mB, vB, aB, 0) == 0
    torch.cuda.synchronize()
    assert torch.equal(G.bits(mB), G.bits(mA)) and torch.equal(G.bits(vB), G.bits(vA)) and torch.equal(G.bits(aB), G.bits(aA)), (case, n)
    for k in stA:
        assert torch.equal(stB[k], stA[k]), (case, n, k)
    assert G.storage_guards_intact(gA) and G.storage_guards_intact(gB)
    assert stB["dones"][0].sum() > 0 and stB["next_privileged_observations"][0].abs().sum() > 0 and stB["actions"][1].abs().sum() > 0
    assert stB["observations"][2].abs().sum() == 0 and stB["rewards"][1].abs().sum() == 0
    # and the means are the policy's: the reference on the second step's inputs, at test_fused_policy_forward_matches_torch's tolerance
    ref = R.policy_forward(case, G.net_of(ac), obs_n.cpu().numpy(), priv_n.cpu().numpy(), None if ext_n is None else ext_n[:, :c["ext"][0]].cpu().numpy())
    np.testing.assert_allclose(mB.cpu().numpy(), ref[0], rtol=2e-4, atol=2e-5 * float(np.abs(ref[0]).max()))


@pytest.mark.parametrize("case", POLICY)
def test_project_packers_equal_the_independent_packer(case):
    """PackedHimPolicy / PackedVisionPolicy: the same bytes, paddings and struct fields as the reference's packer, after construction and after
    an in-place parameter change + refresh(); supported() says yes and the library accepts the struct"""
    from isaacgymloco_amd.learn.fused_policy import PackedHimPolicy
    from isaacgymloco_amd.learn.vision import PackedVisionPolicy
    c = R.POLICY_CASES[case]
    ac = G.policy_module(case).to(DEV)
    cls = PackedVisionPolicy if c["ext"] else PackedHimPolicy
    assert cls.supported(ac)
    pk = cls(ac)
    for change in (False, True):
        if change:
            with torch.no_grad():
                for p in ac.parameters():
                    p.mul_(1.25)
            pk.refresh()
        packed = R.pack_policy(G.net_of(ac))
        flat = packed["encoder"] + packed["actor"] + packed["critic"]
        for i, pl in enumerate(flat):
            lay = pk._P.encoder[i] if i < 3 else (pk._P.actor[i - 3] if i < 7 else pk._P.critic[i - 7])
            assert (lay.k_pad, lay.n_pad, lay.k_in, lay.n_out) == (pl["k_pad"], pl["n_pad"], pl["k_in"], pl["n_out"])
            assert np.array_equal(pk.w[i].cpu().numpy().reshape(-1), pl["weight"]) and np.array_equal(pk.b[i].cpu().numpy(), pl["bias"]), (case, i)
    P = R.policy_struct(case, packed, lambda a: 0)
    assert (pk._P.num_obs, pk._P.num_priv_obs, pk._P.num_one_step_obs, pk._P.num_actions) == (P.num_obs, P.num_priv_obs, P.num_one_step_obs, P.num_actions)
    n = 19
    obs, priv = torch.randn(n, c["hist"] * c["n1"], device=DEV), torch.randn(n, c["P"], device=DEV)
    mean, val = torch.empty(n, c["A"], device=DEV), torch.empty(n, 1, device=DEV)
    if c["ext"]:
        pk.forward(obs, priv, mean, val, rows=torch.randn(n, c["ext"][0], device=DEV))
    else:
        pk.forward(obs, priv, mean, val)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(mean).all())


def test_supported_agrees_with_the_library_on_the_refused_policies():
    """the two mismatches PackedHimPolicy.supported() used to let through (the runner then died in lib.check), on device modules: supported() says
    no, and the struct the class would build is refused by the library before anything is launched"""
    from isaacgymloco_amd import abi, lib
    from isaacgymloco_amd.learn import modules as M
    from isaacgymloco_amd.learn.fused_policy import PackedHimPolicy
    L = lib.load()
    for ac in (M.HIMActorCritic(254, 40, 254, 12), M.HIMActorCritic(100, 40, 45, 12)):
        ac = ac.to(DEV)
        assert not PackedHimPolicy.supported(ac)
        net = G.net_of(ac)
        arrays = G.DeviceArrays()
        packed = R.pack_policy(net)
        P = abi.LsimHimPolicy()
        for nm in packed:
            for i, pl in enumerate(packed[nm]):
                R._fill_layer(getattr(P, nm)[i], pl, arrays.address)
        P.num_obs, P.num_priv_obs, P.num_one_step_obs, P.num_actions = ac.num_actor_obs, 40, ac.num_one_step_obs, 12
        obs, priv = torch.zeros(4, ac.num_actor_obs, device=DEV), torch.zeros(4, 40, device=DEV)
        mean, mflat = G.guarded((4, 12))
        val, vflat = G.guarded((4, 1))
        assert L.lsim_policy_forward(ctypes.byref(P), obs.data_ptr(), priv.data_ptr(), 4, mean.data_ptr(), val.data_ptr(), None) == abi.E_UNSUPPORTED
        torch.cuda.synchronize()
        assert bool(torch.isnan(mflat).all()) and bool(torch.isnan(vflat).all())
