"""CPU: the reference, cases, packer, plan restatement and mutants of the fused MLP shape tests (tests/mlp_shapes_reference.py), and the
refusals of ls_policy_launch / ls_amp_check through the HIP library on host pointers (both answer before any HIP call, so no device is needed;
only refused structs are passed)."""
import ctypes

import numpy as np
import pytest
import torch

import mlp_shapes_reference as R
import mlp_shapes_rig as G

POLICY = list(R.POLICY_CASES)
AMP = list(R.AMP_CASES)


# ---- coverage: a later edit of the cases cannot silently lose a path ---------------------------------------------------------------------
def test_policy_cases_reach_every_tile_and_k_class():
    """every split the two launch forms can take for a layer of at most 32 tiles, and every shape of the k loop: 1-4 chunks without the
    steady state, tails of 2-4 chunks behind it (a tail of one chunk behind the loop cannot occur: the loop leaves 32 < rest <= 64 columns)"""
    got8, got16, gotk = set(), set(), set()
    for case in POLICY:
        assert len(R.policy_plan(case)) == 11
        by_waves, ks = R.policy_plan_union(case)
        got8 |= by_waves[8]; got16 |= by_waves[16]; gotk |= ks
    # per class, the layers that take it: a failure names the class that no layer of any case reaches any more
    where = lambda cls, key: [(case, layer) for case in POLICY for layer, p in R.policy_plan(case).items() if (cls == p[key] if key == "k" else cls in p[key])]
    for key, classes in ((8, R.POLICY_CLASSES_8), (16, R.POLICY_CLASSES_16), ("k", R.POLICY_K_CLASSES)):
        for cls in sorted(classes):
            print(key, cls, where(cls, key))
            assert where(cls, key), (key, cls)
    assert got8 == R.POLICY_CLASSES_8, sorted(got8 ^ R.POLICY_CLASSES_8)
    assert got16 == R.POLICY_CLASSES_16, sorted(got16 ^ R.POLICY_CLASSES_16)
    assert gotk == R.POLICY_K_CLASSES, sorted(gotk ^ R.POLICY_K_CLASSES)
    # without the new cases the shipped shape takes none of the predicated forms
    ship8, ship16 = R.policy_plan_union("shipped")[0][8], R.policy_plan_union("shipped")[0][16]
    assert not any(c.startswith("part") for c in ship8 | ship16)
    assert all(R.k_plan(k)[1] != 1 or R.k_plan(k)[0] == 0 for k in range(16, 513, 16))


def test_amp_cases_reach_every_pass_and_split_class():
    got = set()
    for case in AMP:
        for n in R.AMP_ENVS:
            assert R.amp_nsplit(case, n) in (1, 2)
            got |= R.amp_plan(case, n)
    assert got == R.AMP_CLASSES, sorted(got ^ R.AMP_CLASSES)
    assert {R.amp_nsplit("shipped", n) for n in R.AMP_ENVS} == {1, 2}
    # the predicated head layer (one of a wave's two tiles) is a class of its own: the shipped widths never take it
    assert "t1_per2_valid1" not in set().union(*(R.amp_plan("shipped", n) for n in R.AMP_ENVS))
    assert R.amp_nsplit("wide", 6150) == 2 and R.amp_nsplit("odd", 6150) == 1        # 33 tiles: one block per group would need three per wave


def test_packer_places_every_weight_where_the_header_says():
    rs = np.random.RandomState(0)
    W, b = rs.randn(37, 45).astype(np.float32), rs.randn(37).astype(np.float32)
    pl = R.pack_layer(W, b)
    assert (pl["n_pad"], pl["k_pad"], pl["n_out"], pl["k_in"]) == (48, 48, 37, 45)
    blocks = pl["weight"].reshape(3, 3, 16, 16)
    for n, k in ((0, 0), (36, 44), (16, 15), (15, 16), (20, 33)):
        assert blocks[n // 16, k // 16, n % 16, k % 16] == W[n, k]
    assert np.count_nonzero(pl["weight"]) == np.count_nonzero(W) and not pl["bias"][37:].any() and (pl["bias"][:37] == b).all()


# ---- the reference against the project's torch modules in fp64 --------------------------------------------------------------------------
@pytest.mark.parametrize("case", POLICY)
def test_policy_reference_matches_torch_fp64(case):
    c = R.POLICY_CASES[case]
    ac = G.policy_module(case).double()
    net = G.net_of(ac)
    g = torch.Generator().manual_seed(1)
    obs = 2.0 * torch.randn(33, c["hist"] * c["n1"], generator=g, dtype=torch.float64)
    priv = 2.0 * torch.randn(33, c["P"], generator=g, dtype=torch.float64)
    extra = 2.0 * torch.randn(33, c["ext"][0], generator=g, dtype=torch.float64) if c["ext"] else None
    with torch.no_grad():
        if c["ext"]:
            ac.update_distribution(obs, extra)
        else:
            ac.update_distribution(obs)
        want_mean, want_val = ac.action_mean.numpy(), ac.evaluate(priv).numpy()
    mean, val = R.policy_forward(case, net, obs.numpy(), priv.numpy(), None if extra is None else extra.numpy())
    assert mean.shape == (33, c["A"]) and val.shape == (33, 1)
    np.testing.assert_allclose(mean, want_mean, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(val, want_val, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("case", AMP)
def test_amp_reference_matches_torch_fp64(case):
    from isaacgymloco_amd.learn import amp
    D, _ = R.AMP_CASES[case]
    disc = G.amp_module(case).double()
    ref_disc = G.disc_of(disc)
    g = torch.Generator().manual_seed(2)
    s, nxt, term = (2.0 * torch.randn(21, D, generator=g) for _ in range(3))
    s[:, 0] = 40.0
    task, dones = torch.randn(21, generator=g), torch.rand(21, generator=g) < 0.3
    nz = amp.Normalizer(D)
    nz._mean, nz._var = 0.3 * torch.randn(D, generator=g, dtype=torch.float64), 0.5 + torch.rand(D, generator=g, dtype=torch.float64)
    norm = {"mean": nz._mean.numpy(), "var": nz._var.numpy(), "eps": nz.epsilon, "clip": nz.clip_obs}
    patched = torch.where(dones[:, None], term, nxt)
    # the module's statement with the normaliser's fp32 casts, evaluated in fp64 behind them
    with torch.no_grad():
        x = torch.cat([nz.normalize_torch(s.double()), nz.normalize_torch(patched.double())], dim=-1)
        d = disc.amp_linear(disc.trunk(x))[:, 0]
        r = disc.amp_reward_coef * torch.clamp(1 - 0.25 * torch.square(d - 1), min=0)
        r = (1.0 - disc.task_reward_lerp) * r + disc.task_reward_lerp * task.double()
    rb = amp.ReplayBuffer(D, 30, "cpu")
    rb.step = 20
    rb.insert(s, patched)
    got = R.amp_step(case, ref_disc, s.numpy(), nxt.numpy(), dones.numpy(), term.numpy(), task.numpy(), G.AMP_COEF, G.AMP_LERP, norm,
                     replay=(np.zeros((30, D), np.float32), np.zeros((30, D), np.float32), 20))
    np.testing.assert_allclose(got["d"], d.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got["reward"], r.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(got["replay_s"], rb.states.numpy())
    np.testing.assert_array_equal(got["replay_ns"], rb.next_states.numpy())
    np.testing.assert_array_equal(got["carry"], nxt.numpy())


def test_actor_input_reference_matches_torch_fp64():
    import torch.nn.functional as F
    for n1, latent in R.ACTOR_INPUT_CASES:
        obs, enc, ref, tol = G.actor_input_scene(n1, latent, 37)
        o, e = torch.from_numpy(obs[:, :n1]).double(), torch.from_numpy(enc[:, :3 + latent]).double()
        want = torch.cat((o, e[:, :3], F.normalize(e[:, 3:], dim=-1, p=2)), dim=-1).numpy()
        np.testing.assert_allclose(ref, want, rtol=1e-12, atol=1e-12)
        assert not ref[37 // 2, n1 + 3:].any() and np.isfinite(ref).all()
        for batch in R.ACTOR_INPUT_BATCHES:
            _, e1, _, tol1 = G.actor_input_scene(n1, latent, batch)
            assert any(e1[r, 3:3 + latent].any() for r in range(batch)), "a row whose latent is normalised, at every batch"
            assert batch == 1 or not e1[batch // 2, 3:3 + latent].any()
            # a one-column latent is +-1 in every order of fp32 arithmetic, so its twins cannot differ from the reference; every other scene's do
            assert (tol1 > 0) == (latent > 1), (n1, latent, batch, tol1)


# ---- the independent packer against the project's packers -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", POLICY)
def test_packer_layout_equals_the_projects_view_permute(case):
    """PackedHimPolicy / PackedAmpDisc need a device to construct; their layout statement (fused_policy.py, refresh: a [n_pad, k_pad] image
    cut by view + permute) is restated on CPU tensors here, the buffers of the constructed classes are compared in the GPU files"""
    for layers in G.net_of(G.policy_module(case)).values():
        for W, b in layers:
            pl = R.pack_layer(W, b)
            r = torch.zeros(pl["n_pad"], pl["k_pad"])
            r[:W.shape[0], :W.shape[1]] = torch.from_numpy(W)
            want = r.view(pl["n_pad"] // 16, 16, pl["k_pad"] // 16, 16).permute(0, 2, 1, 3).contiguous()
            assert np.array_equal(pl["weight"], want.numpy().reshape(-1))


# ---- exact scenes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", POLICY)
def test_exact_policy_scenes_are_exact(case):
    """the int64 chain asserts sum |W| |x| + |b| < 2^24 per layer for the batch used; the fp64 reference and every fp32 twin agree with it to the bit"""
    for n in R.POLICY_ENVS:
        net, obs, priv, extra = R.exact_policy_scene(case, n)
        mean, val = R.check_exact_policy(case, net, obs, priv, extra)
        dense = None if extra is None else extra[:, :R.POLICY_CASES[case]["ext"][0]]
        got = R.policy_forward(case, net, obs, priv, dense)
        assert np.array_equal(got[0], mean) and np.array_equal(got[1], val)
        assert mean.max() > 100 and (mean > 0).all() and (val > 0).all()
        if n == 19:
            for _, mm in R.TWINS:
                tw = R.policy_forward(case, net, obs, priv, dense, dtype=np.float32, mm=mm)
                assert np.array_equal(tw[0].astype(np.int64), mean) and np.array_equal(tw[1].astype(np.int64), val)


@pytest.mark.parametrize("case", AMP)
def test_exact_amp_scenes_are_exact(case):
    for n in R.AMP_ENVS:
        disc, prev, nxt, dones, term, task, d = R.exact_amp_scene(case, n)
        got = R.amp_step(case, disc, prev, nxt, dones, term, task, G.AMP_COEF, G.AMP_LERP)
        assert np.array_equal(got["d"], d)
        assert (np.abs(d - 1) < 2).sum() > 0 and (np.abs(d - 1) > 2).sum() > 0, "rows on and off the reward's parabola"
        assert dones.any() and not dones.all()


# ---- general scenes: the tolerance comes from the twins ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", POLICY)
def test_general_policy_scenes_have_a_nonzero_twin_distance(case):
    for zero_latent in (False, True):
        sc = G.general_policy_scene(case, zero_latent)
        assert sc["twin_dist"][0] > 0 and sc["twin_dist"][1] > 0, sc["twin_dist"]
        assert sc["tol"][0] < 1e-3 * np.abs(sc["ref"][0]).max() and sc["tol"][1] < 1e-3 * np.abs(sc["ref"][1]).max()
    plain, zero = G.general_policy_scene(case, False), G.general_policy_scene(case, True)
    assert not np.allclose(plain["ref"][0], zero["ref"][0]) and np.isfinite(zero["ref"][0]).all()


@pytest.mark.parametrize("case", AMP)
def test_general_amp_scenes_have_a_nonzero_twin_distance(case):
    sc = G.general_amp_scene(case)
    assert sc["twin_dist"]["d"] > 0 and sc["twin_dist"]["reward"] > 0, sc["twin_dist"]
    assert (sc["ref"]["reward"] != G.AMP_LERP * sc["task"]).any(), "some style reward is nonzero"


# ---- mutants ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", [m for m, v in R.MUTANTS.items() if v["launch"] == "policy"])
def test_policy_mutants_are_seen(mutant):
    touched = 0
    for case in POLICY:
        c = R.POLICY_CASES[case]
        for n in R.POLICY_ENVS:
            if not R.mutant_touches(mutant, case, n, exact=True):
                continue
            net, obs, priv, extra = R.exact_policy_scene(case, n)
            dense = None if extra is None else extra[:, :c["ext"][0]]
            good, bad = R.policy_forward(case, net, obs, priv, dense), R.policy_forward(case, net, obs, priv, dense, mutant=mutant)
            assert not np.array_equal(good[0], bad[0]) or not np.array_equal(good[1], bad[1]), (mutant, case, n)
            touched += 1
    assert touched or mutant in ("latent_short", "elu_last")
    case = R.MUTANTS[mutant]["case"]
    sc = G.general_policy_scene(case)
    T = G.TWIN_ROWS
    dense = None if sc["extra"] is None else sc["extra"][:T, :R.POLICY_CASES[case]["ext"][0]]
    bad = R.policy_forward(case, sc["net"], sc["obs"][:T], sc["priv"][:T], dense, mutant=mutant)
    miss = max(np.abs(bad[i] - sc["ref"][i][:T]).max() / sc["tol"][i] for i in range(2))
    print(mutant, case, "misses the tolerance by", miss)
    assert miss > 10.0


@pytest.mark.parametrize("mutant", [m for m, v in R.MUTANTS.items() if v["launch"] == "amp"])
def test_amp_mutants_are_seen(mutant):
    for case in AMP:
        for n in R.AMP_ENVS:
            if not R.mutant_touches(mutant, case, n, exact=True):
                continue
            disc, prev, nxt, dones, term, task, _ = R.exact_amp_scene(case, n)
            ns = R.amp_nsplit(case, n)
            good = R.amp_step(case, disc, prev, nxt, dones, term, task, G.AMP_COEF, G.AMP_LERP, nsplit=ns)
            bad = R.amp_step(case, disc, prev, nxt, dones, term, task, G.AMP_COEF, G.AMP_LERP, nsplit=ns, mutant=mutant)
            assert any(not np.array_equal(good[k], bad[k]) for k in ("d", "carry")), (mutant, case, n)
    case = R.MUTANTS[mutant]["case"]
    sc = G.general_amp_scene(case)
    T = G.TWIN_ROWS
    bad = R.amp_step(case, sc["disc"], sc["prev"][:T], sc["nxt"][:T], sc["dones"][:T], sc["term"][:T], sc["task"][:T], G.AMP_COEF, G.AMP_LERP, sc["norm"],
                     nsplit=2, mutant=mutant)
    if mutant == "patch_carry":          # a copy: any difference misses a bit-exact check
        assert not np.array_equal(bad["carry"], sc["nxt"][:T])
    else:
        miss = np.abs(bad["d"] - sc["ref"]["d"][:T]).max() / sc["tol"]["d"]
        print(mutant, case, "misses the tolerance by", miss)
        assert miss > 10.0


# ---- refusals through the HIP library, on host pointers ------------------------------------------------------------------------------------
def _policy_refusals():
    """(name, case, edit(P, keep), extra or None, expected code) -- each edits one thing of a struct the library accepts"""
    from isaacgymloco_amd import abi
    U, I = abi.E_UNSUPPORTED, abi.E_INVALID
    out = []
    def add(name, edit, code=U, case="ragged", extra=None):
        out.append((name, case, edit, extra, code))
    # every bound of ls_pol_check_layer, on one layer of each network
    for net, idx in (("encoder", 1), ("actor", 2), ("critic", 0)):
        lay = lambda P, net=net, idx=idx: getattr(P, net)[idx]
        add(f"{net}[{idx}].weight NULL", lambda P, h, lay=lay: setattr(lay(P), "weight", None))
        add(f"{net}[{idx}].bias NULL", lambda P, h, lay=lay: setattr(lay(P), "bias", None))
        add(f"{net}[{idx}].k_pad 0", lambda P, h, lay=lay: setattr(lay(P), "k_pad", 0))
        add(f"{net}[{idx}].n_pad 0", lambda P, h, lay=lay: setattr(lay(P), "n_pad", 0))
        add(f"{net}[{idx}].k_pad not a multiple of 16", lambda P, h, lay=lay: setattr(lay(P), "k_pad", lay(P).k_pad + 8))
        add(f"{net}[{idx}].n_pad not a multiple of 16", lambda P, h, lay=lay: setattr(lay(P), "n_pad", lay(P).n_pad + 8))
        add(f"{net}[{idx}].k_in > k_pad", lambda P, h, lay=lay: setattr(lay(P), "k_pad", lay(P).k_pad - 16))
        add(f"{net}[{idx}].n_out > n_pad", lambda P, h, lay=lay: setattr(lay(P), "n_pad", lay(P).n_pad - 16))
        add(f"{net}[{idx}].k_in chain broken", lambda P, h, lay=lay: setattr(lay(P), "k_in", lay(P).k_in - 1))
        add(f"{net}[{idx}].n_pad 528", lambda P, h, lay=lay: setattr(lay(P), "n_pad", 528))
        add(f"{net}[{idx}].k_pad 528", lambda P, h, lay=lay: setattr(lay(P), "k_pad", 528))
        add(f"{net}[{idx}].weight misaligned", lambda P, h, lay=lay: setattr(lay(P), "weight", lay(P).weight + 4))
        add(f"{net}[{idx}].bias misaligned", lambda P, h, lay=lay: setattr(lay(P), "bias", lay(P).bias + 4))
    # the 272-wide LDS buffer B: second and last layer of each network
    for net, idx in (("encoder", 1), ("actor", 1), ("actor", 3), ("critic", 1), ("critic", 3)):
        add(f"{net}[{idx}].n_pad 288 lands in buffer B", lambda P, h, net=net, idx=idx: setattr(getattr(P, net)[idx], "n_pad", 288))
    for net in ("encoder", "actor", "critic"):
        add(f"{net}[0].k_pad 288", lambda P, h, net=net: setattr(getattr(P, net)[0], "k_pad", 288))
    # a layer that would read columns its predecessor did not write
    for net, idx in (("encoder", 2), ("actor", 2), ("critic", 3)):
        add(f"{net}[{idx}].k_pad beyond {net}[{idx - 1}].n_pad", lambda P, h, net=net, idx=idx: setattr(getattr(P, net)[idx], "k_pad", getattr(P, net)[idx - 1].n_pad + 16))
    add("num_actions 0", lambda P, h: setattr(P, "num_actions", 0))
    add("num_actions 17", lambda P, h: (setattr(P, "num_actions", 17), setattr(P.actor[3], "n_out", 17), setattr(P.actor[3], "n_pad", 32)))
    add("actor[3].n_out != num_actions", lambda P, h: setattr(P, "num_actions", 15))
    add("critic[3].n_out 2", lambda P, h: setattr(P.critic[3], "n_out", 2))
    add("encoder[2].n_out 3", lambda P, h: (setattr(P.encoder[2], "n_out", 3), setattr(P.actor[0], "k_in", P.num_one_step_obs + 3)))
    add("num_obs 273", lambda P, h: setattr(P, "num_obs", 273))
    add("num_priv_obs 273", lambda P, h: setattr(P, "num_priv_obs", 273))
    add("encoder[0].k_in != num_obs", lambda P, h: setattr(P, "num_obs", P.num_obs - 29))
    add("critic[0].k_in != num_priv_obs", lambda P, h: setattr(P, "num_priv_obs", P.num_priv_obs - 1))
    add("actor[0].k_in != num_one_step_obs + encoder[2].n_out", lambda P, h: setattr(P, "num_one_step_obs", P.num_one_step_obs + 1))
    # the ext checks
    X = abi.LsimPolicyExtra
    def extra(dim, ld, rows=True):
        return lambda h: _extra(X, h, dim, ld, rows)
    add("ext: the plain entry refuses the wider first actor layer", lambda P, h: None, case="ext", extra=None)
    add("ext: rows NULL", lambda P, h: None, I, case="ext", extra=extra(23, 25, rows=False))
    add("ext: dim 0", lambda P, h: None, I, case="ext", extra=extra(0, 25))
    add("ext: ld < dim", lambda P, h: None, I, case="ext", extra=extra(23, 22))
    add("ext: dim does not match actor[0].k_in", lambda P, h: None, case="ext", extra=extra(22, 25))
    add("ext: actor[0].k_pad 288", lambda P, h: setattr(P.actor[0], "k_pad", 288), case="ext", extra=extra(23, 25))
    add("ext on a policy without the segment", lambda P, h: None, case="ragged", extra=extra(23, 25))
    return out


def _extra(X, h, dim, ld, rows):
    x = X()
    buf = np.zeros((4, max(ld, 1)), dtype=np.float32)
    h.keep.append(buf)
    x.rows, x.dim, x.ld = (buf.ctypes.data if rows else None), dim, ld
    return x


@pytest.mark.parametrize("name,case,edit,extra,code", _policy_refusals(), ids=[r[0] for r in _policy_refusals()])
def test_policy_launch_refuses_on_the_host(name, case, edit, extra, code):
    from isaacgymloco_amd import lib
    L = lib.load()
    P, h, (obs, priv, mean, val) = G.host_policy(case)
    edit(P, h)
    before = (mean.tobytes(), val.tobytes())
    if extra is not None:
        x = extra(h)
        rc = L.lsim_policy_forward_ext(ctypes.byref(P), ctypes.byref(x), obs.ctypes.data, priv.ctypes.data, 4, mean.ctypes.data, val.ctypes.data, None)
    else:
        rc = L.lsim_policy_forward(ctypes.byref(P), obs.ctypes.data, priv.ctypes.data, 4, mean.ctypes.data, val.ctypes.data, None)
    assert rc == code, (name, rc)
    assert (mean.tobytes(), val.tobytes()) == before


def test_policy_launch_refuses_null_arguments_and_a_first_actor_layer_padded_to_288():
    from isaacgymloco_amd import abi, lib
    L = lib.load()
    P, h, (obs, priv, mean, val) = G.host_policy("tiny")
    ptrs = [obs.ctypes.data, priv.ctypes.data, 4, mean.ctypes.data, val.ctypes.data]
    assert L.lsim_policy_forward(None, *ptrs, None) == abi.E_INVALID
    for i in (0, 1, 3, 4):
        a = list(ptrs); a[i] = None
        assert L.lsim_policy_forward(ctypes.byref(P), *a, None) == abi.E_INVALID, i
    a = list(ptrs); a[2] = 0
    assert L.lsim_policy_forward(ctypes.byref(P), *a, None) == abi.E_INVALID
    assert L.lsim_policy_forward_ext(ctypes.byref(P), None, *ptrs, None) == abi.E_INVALID
    # a history of one step with 254 observations: num_obs 254 <= 272, but the first actor layer reads 254 + 3 + 16 = 273 -> 288 columns
    W = lambda n, k: (np.zeros((n, k), np.float32), np.zeros(n, np.float32))
    net = {"encoder": [W(16, 254), W(16, 16), W(19, 16)], "actor": [W(16, 273), W(16, 16), W(16, 16), W(12, 16)], "critic": [W(16, 8), W(16, 16), W(16, 16), W(1, 16)]}
    packed = R.pack_policy(net)
    P = abi.LsimHimPolicy()
    for nm in packed:
        for i, pl in enumerate(packed[nm]):
            R._fill_layer(getattr(P, nm)[i], pl, h.address)
    P.num_obs, P.num_priv_obs, P.num_one_step_obs, P.num_actions = 254, 8, 254, 12
    assert P.actor[0].k_pad == 288
    o, p, m, v = np.zeros((4, 254), np.float32), np.zeros((4, 8), np.float32), np.full((4, 12), 7.25, np.float32), np.full((4, 1), 7.25, np.float32)
    assert L.lsim_policy_forward(ctypes.byref(P), o.ctypes.data, p.ctypes.data, 4, m.ctypes.data, v.ctypes.data, None) == abi.E_UNSUPPORTED
    assert (m == 7.25).all() and (v == 7.25).all()


class _OnDevice:
    """stands for a module's parameters where supported() only asks whether they are on the device"""
    is_cuda = True


def _shape_verdict(ac):
    """PackedHimPolicy.supported() with the device question answered yes: its verdict on the shapes alone"""
    from isaacgymloco_amd.learn.fused_policy import PackedHimPolicy
    orig = ac.parameters
    ac.parameters = lambda: iter([_OnDevice()])
    try:
        return PackedHimPolicy.supported(ac)
    finally:
        ac.parameters = orig


def test_supported_is_the_librarys_rule():
    """the two mismatches supported() used to admit, and the other bounds a config can break, against the library's verdict on the struct PackedHimPolicy would build (host pointers: refusals only)"""
    from isaacgymloco_amd import abi, lib
    from isaacgymloco_amd.learn import modules as M
    L = lib.load()

    def verdict(ac):
        h = G.HostArrays()
        net = G.net_of(ac)
        packed = R.pack_policy(net)
        P = abi.LsimHimPolicy()
        for nm in packed:
            for i, pl in enumerate(packed[nm]):
                R._fill_layer(getattr(P, nm)[i], pl, h.address)
        P.num_obs, P.num_priv_obs, P.num_one_step_obs, P.num_actions = ac.num_actor_obs, net["critic"][0][0].shape[1], ac.num_one_step_obs, ac.num_actions
        o, p = np.zeros((4, P.num_obs), np.float32), np.zeros((4, P.num_priv_obs), np.float32)
        m, v = np.zeros((4, P.num_actions), np.float32), np.zeros((4, 1), np.float32)
        return L.lsim_policy_forward(ctypes.byref(P), o.ctypes.data, p.ctypes.data, 4, m.ctypes.data, v.ctypes.data, None)

    wide = M.HIMActorCritic(254, 40, 254, 12)                       # a history of 1 with 254 observations: actor[0] pads to 288
    assert wide.actor[0].in_features == 273 and verdict(wide) == abi.E_UNSUPPORTED and not _shape_verdict(wide)
    ragged = M.HIMActorCritic(100, 40, 45, 12)                      # int(100 / 45) * 45 = 90 != 100: the estimator reads 90 columns
    assert ragged.estimator.encoder[0].in_features == 90 and verdict(ragged) == abi.E_UNSUPPORTED and not _shape_verdict(ragged)
    # the bounds a training config can break through actor_hidden_dims / critic_hidden_dims and the observation sizes
    for what, ac in (("a hidden layer of 528", M.HIMActorCritic(90, 40, 45, 12, actor_hidden_dims=(528, 256, 128))),
                     ("a second layer of 288", M.HIMActorCritic(90, 40, 45, 12, critic_hidden_dims=(512, 288, 128))),
                     ("17 actions", M.HIMActorCritic(90, 40, 45, 17)),
                     ("273 privileged observations", M.HIMActorCritic(90, 273, 45, 12)),
                     ("a history of 276", M.HIMActorCritic(276, 40, 46, 12))):
        assert verdict(ac) == abi.E_UNSUPPORTED and not _shape_verdict(ac), what
    for case in POLICY:                                             # and the cases stay in
        assert _shape_verdict(G.policy_module(case)), case


def _amp_refusals():
    from isaacgymloco_amd import abi
    U, I = abi.E_UNSUPPORTED, abi.E_INVALID
    H = lambda S, i: S.hidden[i]
    return [
        ("head_weight NULL", lambda S: setattr(S, "head_weight", None), I),
        ("head_bias NULL", lambda S: setattr(S, "head_bias", None), I),
        ("amp_dim 0", lambda S: setattr(S, "amp_dim", 0), U),
        ("amp_dim 33", lambda S: setattr(S, "amp_dim", 33), U),
        ("norm_mean without norm_var", lambda S: setattr(S, "norm_mean", S.head_weight), I),
        ("hidden[0].weight NULL", lambda S: setattr(H(S, 0), "weight", None), I),
        ("hidden[1].bias NULL", lambda S: setattr(H(S, 1), "bias", None), I),
        ("hidden[0].k_pad 0", lambda S: setattr(H(S, 0), "k_pad", 0), I),
        ("hidden[1].n_pad 0", lambda S: setattr(H(S, 1), "n_pad", 0), I),
        ("hidden[0].k_pad not a multiple of 16", lambda S: setattr(H(S, 0), "k_pad", H(S, 0).k_pad + 8), I),
        ("hidden[1].n_pad not a multiple of 16", lambda S: setattr(H(S, 1), "n_pad", H(S, 1).n_pad + 8), I),
        ("hidden[0].k_in > k_pad", lambda S: setattr(H(S, 0), "k_pad", H(S, 0).k_pad - 16), I),
        ("hidden[1].n_out > n_pad", lambda S: setattr(H(S, 1), "n_pad", H(S, 1).n_pad - 16), I),
        ("hidden[1].weight misaligned", lambda S: setattr(H(S, 1), "weight", H(S, 1).weight + 4), I),
        ("hidden[0].bias misaligned", lambda S: setattr(H(S, 0), "bias", H(S, 0).bias + 4), I),
        ("head_weight misaligned", lambda S: setattr(S, "head_weight", S.head_weight + 4), I),
        ("hidden[0].k_in != 2 amp_dim", lambda S: setattr(S, "amp_dim", S.amp_dim - 1), I),
        ("hidden[0].k_pad 80", lambda S: setattr(H(S, 0), "k_pad", 80), I),
        ("hidden[1].k_in != hidden[0].n_out", lambda S: setattr(H(S, 1), "k_in", H(S, 1).k_in - 1), I),
        ("hidden[1].k_pad != hidden[0].n_pad", lambda S: setattr(H(S, 1), "k_pad", H(S, 1).k_pad + 16), I),
        ("hidden[0].n_pad 1040", lambda S: (setattr(H(S, 0), "n_pad", 1040), setattr(H(S, 1), "k_pad", 1040)), U),
    ]


@pytest.mark.parametrize("name,edit,code", _amp_refusals(), ids=[r[0] for r in _amp_refusals()])
def test_amp_check_refuses_on_the_host(name, edit, code):
    from isaacgymloco_amd import lib
    L = lib.load()
    case, n = "odd", 4
    D = R.AMP_CASES[case][0]
    disc = R.exact_amp_scene(case, n)[0]
    h = G.HostArrays()
    S = R.amp_struct(case, R.pack_amp(disc), h.address, G.AMP_COEF, G.AMP_LERP)
    edit(S)
    z = lambda *s: np.zeros(s, np.float32)
    prev, nxt, task, rew, d = z(n, D), z(n, D), z(n), np.full(n, 7.25, np.float32), np.full(n, 7.25, np.float32)
    ws = np.zeros(1024, np.int32)
    rc = L.lsim_amp_step(ctypes.byref(S), prev.ctypes.data, nxt.ctypes.data, None, None, task.ctypes.data, n, rew.ctypes.data, d.ctypes.data, None, None, None, 0, 0,
                         ws.ctypes.data, ws.nbytes, None)
    assert rc == code, (name, rc)
    assert (rew == 7.25).all() and (d == 7.25).all() and not ws.any()
