"""CPU: the statements, plan restatement, case tables, scenes and mutants of the loss-head shape tests (tests/loss_heads_reference.py), and the
refusals of the five entries through the HIP library on host pointers (they answer before any HIP call, so no device is needed; only refused
calls are made)."""
import ctypes

import numpy as np
import pytest
import torch

import loss_heads_reference as R

F64 = torch.float64


# ---- coverage: a later edit of the tables cannot silently lose a path ----------------------------------------------------------------------
def test_cases_reach_every_class():
    """all four estimator instantiations and both Sinkhorn ones, each vector flag and `fold` both ways, every multi-in-flight loop with no pass,
    with passes, with and without a tail, every PPO finish block count, every Adam slice class: from the restated plan alone"""
    where = R.all_classes()
    assert set(where) <= R.CLASSES, sorted(set(where) - R.CLASSES)
    for cls in sorted(R.CLASSES):
        print(cls, where.get(cls, [])[:4])
        assert where.get(cls), "no case reaches " + cls
    for lp in ("scale32", "scale64", "est_tail", "ppo_finish"):
        assert {"%s:%s" % (lp, c) for c in ("passes>0", "passes=0", "tail", "notail")} <= set(where)
    assert {R.PPO_CASES[n]["B"] for n in R.PPO_CASES if R.PPO_CASES[n]["entry"] == "std"} == set(R._ppo_batches().values())
    assert sorted(R.ceil_div(B, 256) for B in R._ppo_batches().values()) == list(R.PPO_BLOCKS)


def test_estimator_case_table_reaches_what_it_was_built_for():
    """partials, blocks and instantiations of the estimator cases the case table was built around; every case on the single-wave plan"""
    want = {"b1-d1-k1": ((32, 16), 1), "b63-d5-k3": ((32, 16), 1), "b65-d16-k32": ((32, 16), 2), "b130-d20-k28": ((32, 32), 3), "b129-d17-k31": ((32, 32), 3),
            "b777-d9-k50": ((64, 16), 13), "b200-d32-k64": ((64, 32), 4), "b3700-d32-k64": ((64, 32), 58), "b7300-d4-k36": ((64, 16), 115),
            "b14400-d4-k8": ((32, 16), 225), "b3585-d17-k33": ((64, 32), 57)}
    for name, (inst, blocks) in want.items():
        B, D, K, _ = R.EST_CASES[name]
        p = R.estimator_plan(B, D, K)
        assert (p["inst"], p["blocks"], p["small"]) == (inst, blocks, True), (name, p)
    p = lambda n: R.estimator_plan(*R.EST_CASES[n][:3])
    assert (p("b3700-d32-k64")["partials"], p("b7300-d4-k36")["partials"], p("b3585-d17-k33")["partials"]) == (463, 913, 449)
    assert not p("b3585-d17-k33")["fold"] and not p("b63-d5-k3")["fold"] and not p("b129-d17-k31")["fold"] and p("b3700-d32-k64")["fold"]
    # 225 blocks on 32 slices: slice 0 makes exactly one pass and has no tail, every other slice only a tail; 115 on 16: three slices pass
    assert p("b14400-d4-k8")["scale"]["per"][0] == (1, 0) and p("b14400-d4-k8")["scale"]["per"][1] == (0, 7)
    assert [x[0] for x in p("b7300-d4-k36")["scale"]["per"]] == [1, 1, 1] + [0] * 13
    assert R.sinkhorn_plan(58000, 5)["blocks"] == 227 and [x[0] for x in R.sinkhorn_plan(58000, 5)["scale"]["per"]][:4] == [1, 1, 1, 0]
    assert R.inflight(13, 3, 4)["per"] == [(1, 1), (1, 0), (1, 0)] and R.inflight(10, 3, 4)["per"] == [(1, 0), (0, 3), (0, 3)]
    for n in range(1, 600):                       # every row is owned once, by the loop or by a tail
        lp = R.inflight(n, 16, 8)
        assert sum(8 * a + b for a, b in lp["per"]) == n


def test_cases_stay_small():
    assert max(B * K for B, K, _ in R.SK_CASES.values()) == 58000 * 5
    assert max(c[0] for c in R.EST_CASES.values()) <= 14400 and max(c["B"] for c in R.PPO_CASES.values()) <= 6400
    for K, layout in ((8, "vec"), (8, "odd"), (8, "off4"), (64, "odd"), (64, "off4"), (5, "vec")):
        off, lds = R.sk_layout(K, layout)
        assert lds > K and R.sk_vec_in(K, layout) == (layout == "vec" and K % 4 == 0)


def test_plan_restatement_against_the_library():
    """the *_workspace functions are host code: the restated byte counts for every case and for the update's shapes"""
    from isaacgymloco_amd import abi, lib
    L = lib.load()
    n = ctypes.c_size_t(0)
    for B, D, K in [c[:3] for c in R.EST_CASES.values()] + [(102400, 16, 32), (5, 33, 8), (5, 8, 65), (0, 8, 8)]:
        rc, p = L.lsim_estimator_loss_workspace(B, D, K, ctypes.byref(n)), R.estimator_plan(B, D, K)
        assert (rc, n.value) == (0, p["bytes"]) if p else rc == abi.E_INVALID, (B, D, K, rc, n.value, p)
    for B, K in [c[:2] for c in R.SK_CASES.values()] + [(102400, 32)]:
        assert (L.lsim_sinkhorn_workspace(B, K, ctypes.byref(n)), n.value) == (0, R.sinkhorn_plan(B, K)["bytes"]), (B, K)
    for c in R.PPO_CASES.values():
        if c["entry"] == "std":
            rc = L.lsim_ppo_loss_std_workspace(c["B"], c["A"], ctypes.byref(n))
        else:
            rc = L.lsim_ppo_loss_workspace(c["B"], ctypes.byref(n))
        assert (rc, n.value) == (0, R.ppo_plan(c["B"], c["A"], c["entry"] == "std")["bytes"])
    assert L.lsim_ppo_loss_std_workspace(300, 61, ctypes.byref(n)) == abi.E_INVALID
    for count in (1, 7, 48):
        assert (L.lsim_adam_clip_step_workspace(count, ctypes.byref(n)), n.value) == (0, R.adam_bytes(count))
    assert L.lsim_adam_clip_step_workspace(49, ctypes.byref(n)) == abi.E_INVALID


# ---- the statements against torch in fp64 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,iters", [("b63-d5-k3", 3), ("b65-d16-k32", 1), ("b129-d17-k31", 3)])
def test_estimator_statement_matches_torch_autograd_fp64(name, iters):
    """the torch statement of tests/test_gpu_learner.py::test_fused_estimator_loss_matches_torch_autograd on the CPU; two of the cases hold rows that
    F.normalize clamps (its backward through the clamp is the plain scale)"""
    sc = R.estimator_scene(name)
    e64, t64, p64 = (torch.from_numpy(sc[k]).double().requires_grad_(True) for k in ("enc", "tgt", "proto"))
    z_s = torch.nn.functional.normalize(e64[:, 3:], dim=-1)
    z_t = torch.nn.functional.normalize(t64, dim=-1)
    S_s, S_t = z_s @ p64.T, z_t @ p64.T

    def sk(scores):
        Q = torch.exp(scores.detach() / R.SK_EPS).T
        Q /= Q.sum()
        for _ in range(iters):
            Q /= Q.sum(dim=1, keepdim=True); Q /= Q.shape[0]
            Q /= Q.sum(dim=0, keepdim=True); Q /= Q.shape[1]
        return (Q * Q.shape[1]).T
    T = R.TEMPERATURE
    swap = -0.5 * (sk(S_s) * torch.log_softmax(S_t / T, -1) + sk(S_t) * torch.log_softmax(S_s / T, -1)).mean()
    est = torch.nn.functional.mse_loss(e64[:, :3], torch.from_numpy(sc["vel"]).double())
    (est + swap).backward()
    for form in ("direct", "factored", "reversed"):
        o = R.estimator_loss(sc["enc"], sc["tgt"], sc["proto"], sc["vel"], T, R.SK_EPS, iters, form=form)
        np.testing.assert_allclose([o["est"], o["swap"], o["total"]], [est.item(), swap.item(), (est + swap).item()], rtol=1e-12)
        for got, want in ((np.concatenate([o["d_vel"], o["d_lat"]], 1), e64.grad), (o["d_tgt"], t64.grad), (o["d_proto"], p64.grad)):
            w = want.numpy()
            rowmax = np.maximum(np.abs(w).max(axis=-1, keepdims=True), 1e-300)       # per row: a clamped row is 1e12 x the others
            assert float((np.abs(got - w) / rowmax).max()) < 1e-9, (form, float((np.abs(got - w) / rowmax).max()))
    np.testing.assert_allclose(R.sinkhorn(S_s.detach().numpy(), R.SK_EPS, iters, form="factored"), sk(S_s).numpy(), rtol=1e-11)


@pytest.mark.parametrize("name", ["std-a12-b511-c1", "sigma-a60-b511-c0", "sigma-a1-b768-c1", "ties-std", "ties-sigma"])
def test_ppo_statement_matches_torch_autograd_fp64(name):
    """the torch statement of tests/test_gpu_learner.py::test_fused_ppo_loss_matches_torch_autograd on the CPU, on general scenes and on the scene of
    ties and closed ends: torch's maximum and clamp fix the sub-gradients there"""
    from torch.distributions import Normal
    if name.startswith("ties"):
        std_mode, clipped = name == "ties-std", 1
        s, clip, _ = R.ppo_tie_scene(std_mode=std_mode)
    else:
        c = R.PPO_CASES[name]
        s, clip, std_mode, clipped = R.ppo_scene(name), R.PPO_CLIP, c["entry"] == "std", c["clipped"]
    clip = float(np.float32(clip))
    t = {k: torch.from_numpy(v).double() for k, v in s.items()}
    mu, sg, value = t["mu"].requires_grad_(True), t["sigma"].requires_grad_(True), t["value"].requires_grad_(True)
    sigma = mu * 0.0 + sg
    dist = Normal(mu, sigma)
    logp, ent = dist.log_prob(t["actions"]).sum(-1), dist.entropy().sum(-1)
    ratio = torch.exp(logp - t["old_logp"])
    sur = torch.max(-t["adv"] * ratio, -t["adv"] * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
    if clipped:
        vc = t["tv"] + (value - t["tv"]).clamp(-clip, clip)
        vl = torch.max((value - t["returns"]).pow(2), (vc - t["returns"]).pow(2)).mean()
    else:
        vl = (t["returns"] - value).pow(2).mean()
    kl = torch.sum(torch.log(sigma / t["old_sigma"] + 1e-5) + (t["old_sigma"] ** 2 + (t["old_mu"] - mu) ** 2) / (2 * sigma ** 2) - 0.5, -1).mean()
    total = sur + R.PPO_CV * vl - R.PPO_CE * ent.mean()
    total.backward()
    for form in R.PPO_TWINS:
        o = R.ppo_loss(s, clip, R.PPO_CV, R.PPO_CE, clipped, std_mode, form=form)
        np.testing.assert_allclose(o["stats"], [x.item() for x in (sur, vl, ent.mean(), kl, total)], rtol=1e-10, atol=1e-13)
        np.testing.assert_allclose(o["g_mu"], mu.grad.numpy(), rtol=1e-9, atol=1e-16)
        np.testing.assert_allclose(o["g_std" if std_mode else "g_sigma"], sg.grad.numpy(), rtol=1e-9, atol=1e-15)
        np.testing.assert_allclose(o["g_value"], value.grad.numpy(), rtol=1e-9, atol=1e-16)


@pytest.mark.parametrize("name", ["n7-clip3-active-dev", "n7-clip7-off0-host", "n1-clip0-active-dev"])
def test_adam_statement_matches_torch_fp64(name):
    """clip_grad_norm_ + torch.optim.Adam in fp64, with per-parameter step counters and weight decay per group"""
    c, s = R.ADAM_CASES[name], R.adam_scene(name)
    lr, b1, b2, eps = (float(np.float32(x)) for x in (R.ADAM_LR, R.ADAM_B1, R.ADAM_B2, R.ADAM_EPS))
    ps = [torch.from_numpy(p).double().requires_grad_(True) for p in s["p"]]
    opt = torch.optim.Adam([dict(params=[p], weight_decay=w) for p, w in zip(ps, c["wd"])], lr=lr, betas=(b1, b2), eps=eps)
    for i, p in enumerate(ps):
        p.grad = torch.from_numpy(s["g"][i]).double()
        opt.state[p] = dict(step=torch.tensor(c["steps"][i], dtype=F64), exp_avg=torch.from_numpy(s["m"][i]).double(), exp_avg_sq=torch.from_numpy(s["v"][i]).double())
    norm = 0.0
    if c["max_norm"] > 0 and c["clip_count"]:
        norm = float(torch.nn.utils.clip_grad_norm_(ps[:c["clip_count"]], c["max_norm"]))
    elif c["clip_count"]:
        norm = float(torch.linalg.vector_norm(torch.cat([p.grad for p in ps[:c["clip_count"]]])))
    opt.step()
    for form in ("lerp", "b1m"):
        o = R.adam_clip_step(s["p"], s["g"], s["m"], s["v"], c["steps"], c["wd"], c["clip_count"], lr, b1, b2, eps, c["max_norm"], form=form)
        np.testing.assert_allclose(o["norm"], norm, rtol=1e-12)
        for i, p in enumerate(ps):
            st = opt.state[p]
            for got, want in ((o["p"][i], p.detach()), (o["g"][i], p.grad), (o["m"][i], st["exp_avg"]), (o["v"][i], st["exp_avg_sq"])):
                np.testing.assert_allclose(got, want.numpy(), rtol=1e-9, atol=1e-14)
            assert o["step"][i] == float(st["step"])


# ---- scenes --------------------------------------------------------------------------------------------------------------------------------
def test_ppo_general_scenes_have_no_row_near_a_boundary():
    for name in R.PPO_CASES:
        assert R.ppo_case(name)["near"] == [0, 0, 0], name


def test_ppo_tie_scene_is_what_it_claims():
    for std_mode in (True, False):
        s, clip, rows = R.ppo_tie_scene(std_mode=std_mode)
        o = R.ppo_loss(s, clip, R.PPO_CV, R.PPO_CE, 1, std_mode)
        B = s["mu"].shape[0]
        v, tv, Rt = (s[k].astype(np.float64) for k in ("value", "tv", "returns"))
        assert (s["adv"][rows["adv0"]] == 0).all() and (o["g_mu"][rows["adv0"]] == 0).all()
        assert (v[rows["v_eq_tv"]] == tv[rows["v_eq_tv"]]).all() and (np.abs(v[rows["end"]] - tv[rows["end"]]) == clip).all()
        vc = tv + np.clip(v - tv, -clip, clip)
        assert ((v - Rt) ** 2 == (vc - Rt) ** 2)[rows["mid"]].all() and (np.abs(v - tv) > clip)[rows["mid"]].all() and (v != Rt)[rows["mid"]].all()
        for k in ("v_eq_tv", "end"):
            np.testing.assert_array_equal(o["g_value"][rows[k]], R.PPO_CV * 2 * (v - Rt)[rows[k]] / B)
        np.testing.assert_array_equal(o["g_value"][rows["mid"]], R.PPO_CV * (v - Rt)[rows["mid"]] / B)
        d = (s["actions"].astype(np.float64) - s["mu"]) / np.broadcast_to(s["sigma"], s["mu"].shape).astype(np.float64) ** 2
        same = rows["same"]
        np.testing.assert_allclose(o["g_mu"][same], (-s["adv"][same].astype(np.float64) / B)[:, None] * d[same], rtol=1e-6)


def test_estimator_clamped_rows_are_the_large_ones():
    for name, (B, D, K, clamp) in R.EST_CASES.items():
        if clamp:
            out = R.estimator_case(name, 3)["out"]
            (rs, rt) = R.clamped_rows(B)
            for k, rows in (("d_lat", rs), ("d_tgt", rt)):
                for r in rows:
                    assert out["%s[%d]" % (k, r)]["scale"] > 1e10 * out[k]["scale"]


# ---- mutants -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", [m for m, (fam, _) in R.MUTANTS.items() if fam in ("est", "est3")])
def test_estimator_mutants_are_seen(mutant):
    fam, cases = R.MUTANTS[mutant]
    names = cases()
    assert names
    for name in names:
        for iters in ((3,) if fam == "est3" else R.ITERS):
            case = R.estimator_case(name, iters)
            sc = case["scene"]
            o = R.estimator_loss(sc["enc"], sc["tgt"], sc["proto"], sc["vel"], R.TEMPERATURE, R.SK_EPS, iters, mutant=mutant)
            bad = R.beyond(case["out"], R.est_split(name, o))
            print(mutant, name, iters, bad)
            assert bad, (mutant, name, iters)


@pytest.mark.parametrize("mutant", list(R.SK_MUTANTS))
def test_sinkhorn_mutants_are_seen(mutant):
    names = R.SK_MUTANTS[mutant]()
    assert names
    for name in names:
        for iters in ((3,) if mutant == "last_step_not_folded" else R.ITERS):
            case = R.sinkhorn_case(name, iters)
            bad = R.beyond(case["out"], {"q": R.sinkhorn(case["scores"], R.SK_EPS, iters, mutant=mutant)})
            assert bad, (mutant, name, iters)


def test_ppo_mutants_are_seen():
    for std_mode in (True, False):
        case = R.ppo_tie_case(std_mode)
        for mutant, keys in (("tie_weights_10", ("mid",)), ("clamp_open", ("end",))):
            o = R.ppo_outputs(R.ppo_loss(case["scene"], case["clip"], R.PPO_CV, R.PPO_CE, 1, std_mode, mutant=mutant))
            assert "g_value" in R.beyond(case["out"], o), mutant
            d = np.abs(o["g_value"] - case["out"]["g_value"]["ref"])
            # (dyadic values: another row may tie by chance; the rows built for the mutant must all show it)
            assert set(np.flatnonzero(d > case["out"]["g_value"]["tol"])) >= set(np.concatenate([case["rows"][k] for k in keys]))
    for name in R.MUTANTS["g_std_missing_block"][1]():
        case, c = R.ppo_case(name), R.PPO_CASES[name]
        o = R.ppo_outputs(R.ppo_loss(case["scene"], R.PPO_CLIP, R.PPO_CV, R.PPO_CE, c["clipped"], True, mutant="g_std_missing_block"))
        assert R.beyond(case["out"], o) == ["g_std"], name


@pytest.mark.parametrize("mutant", [m for m, (fam, _) in R.MUTANTS.items() if fam == "adam"])
def test_adam_mutants_are_seen(mutant):
    names = R.MUTANTS[mutant][1]()
    assert names
    for name in names:
        case, c, s = R.adam_case(name), R.ADAM_CASES[name], R.adam_case(name)["scene"]
        o = R.adam_clip_step(s["p"], s["g"], s["m"], s["v"], c["steps"], c["wd"], c["clip_count"], np.float32(R.ADAM_LR), np.float32(R.ADAM_B1),
                             np.float32(R.ADAM_B2), np.float32(R.ADAM_EPS), c["max_norm"], mutant=mutant)
        assert R.beyond(case["out"], R.adam_outputs(o)), (mutant, name)


def test_every_mutant_of_the_list_is_tested():
    assert set(R.MUTANTS) == {"d0_quarter", "u_other", "last_block_dropped", "clamp_missing", "last_step_not_folded", "c_with_B", "loop_tail_skipped",
                              "tie_weights_10", "clamp_open", "g_std_missing_block", "step0_for_all", "norm_all_tensors", "decay_written_back"}


# ---- tolerances ----------------------------------------------------------------------------------------------------------------------------
def test_tolerances_follow_the_twins_and_stay_tight():
    """4 x the twin distance, floored at 4 * 2^-23 of the output's scale -- and nowhere wider than 1e-4 of the scale except the surrogate and KL means,
    which may cancel to a small value (their twin distance is a few 1e-8 absolute)"""
    worst = {}
    for fam, cases in (("est", [R.estimator_case(n, i)["out"] for n in R.EST_CASES for i in R.ITERS]),
                       ("sk", [R.sinkhorn_case(n, i)["out"] for n in R.SK_CASES for i in R.ITERS]),
                       ("ppo", [R.ppo_case(n)["out"] for n in R.PPO_CASES]), ("adam", [R.adam_case(n)["out"] for n in R.ADAM_CASES])):
        for out in cases:
            for k, o in out.items():
                assert o["tol"] == max(4.0 * o["dist"], 4.0 * R.ULP * o["scale"])
                key = (fam, k.split("[")[0])
                worst[key] = max(worst.get(key, 0.0), o["dist"] / o["scale"] if o["scale"] else 0.0)
    for key, v in sorted(worst.items()):
        print("largest twin distance over scale", key, "%.2e" % v)
        assert v < (1e-3 if key in (("ppo", "stat0"), ("ppo", "stat3")) else 2.5e-5), key


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
class _Host:
    def __init__(self):
        self.keep = []

    def address(self, floats):
        a = np.full(floats + 8, np.nan, dtype=np.float32)
        off = (-a.ctypes.data % 16) // 4
        self.keep.append(a)
        return a.ctypes.data + 4 * off

    def untouched(self):
        return all(np.isnan(a).all() for a in self.keep)


def test_entries_refuse_on_the_host():
    from isaacgymloco_amd import abi, lib
    L = lib.load()
    assert {f for _, f, _, _ in R.REFUSALS} == set(R.SIGNATURES)
    labels = " | ".join(r[0] for r in R.REFUSALS)
    for must in ("sinkhorn workspace 4 bytes off", "sinkhorn out 4 bytes off", "est latent 33", "est K 65", "ppo_std num_actions 61", "adam count 49", "adam clip_count > count"):
        assert must in labels
    for label, fam, edits, code in R.REFUSALS:
        h = _Host()
        rc = R.refusal_call(L, fam, edits, h.address)
        assert rc == getattr(abi, code), (label, rc)
        assert h.untouched(), label
