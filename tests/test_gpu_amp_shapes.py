"""GPU: lsim_amp_step (csrc/ls_amp.h) at the discriminator widths of tests/mlp_shapes_reference.py -- trunk[0] ending on a full, a half-filled
and an idle pass, trunk[1] with one and two tiles per wave, an odd tile count under the two-block split, the split forced above 32 tiles per
block -- at env counts that select two blocks per row group and one (the restatement picks; the A/B environment switch stays unset)."""
import os

import numpy as np
import pytest
import torch

import mlp_shapes_reference as R
import mlp_shapes_rig as G

pytestmark = pytest.mark.gpu
AMP = list(R.AMP_CASES)


@pytest.mark.parametrize("n", R.AMP_ENVS)
@pytest.mark.parametrize("case", AMP)
def test_exact_scene(case, n):
    """signed integer weights and inputs, no normaliser: disc_out to the bit under either split; the rewards at test_gpu_amp_step.py's
    tolerance; carry and the wrapped replay insert are copies, bit-exact; three launches leave the workspace's counters at zero"""
    assert "LSIM_AMP_NSPLIT" not in os.environ and R.amp_nsplit(case, n) in (1, 2)
    disc, prev, nxt, dones, term, task, d = R.exact_amp_scene(case, n)
    cap = n + 100
    cursor = cap - n // 2                             # the insert wraps
    D = R.AMP_CASES[case][0]
    ring = np.full((cap, D), np.nan, dtype=np.float32)
    ref = R.amp_step(case, disc, prev, nxt, dones, term, task, G.AMP_COEF, G.AMP_LERP, replay=(ring, ring, cursor))
    assert np.array_equal(ref["d"], d)
    pk = G.DeviceAmp(case, disc, n)
    got = pk.step(prev, nxt, dones, term, task, cap, cursor, launches=3)
    assert np.array_equal(got["d"], d.astype(np.float32)), (case, n)
    np.testing.assert_allclose(got["reward"], ref["reward"], rtol=1e-5, atol=1e-6)
    assert np.array_equal(got["carry"], nxt.astype(np.float32))
    for k in ("replay_s", "replay_ns"):
        assert np.array_equal(got[k], ref[k], equal_nan=True), (case, n, k)
    assert np.isnan(got["replay_s"]).sum() == 100 * D
    assert int(pk.counters(n).abs().sum()) == 0


@pytest.mark.parametrize("n", R.AMP_ENVS)
@pytest.mark.parametrize("case", AMP)
def test_general_scene_within_the_twins_tolerance(case, n):
    sc = G.general_amp_scene(case)
    pk = G.DeviceAmp(case, sc["disc"], n, norm=sc["norm"])
    got = pk.step(sc["prev"][:n], sc["nxt"][:n], sc["dones"][:n], sc["term"][:n], sc["task"][:n], n, 0)
    for k in ("d", "reward"):
        err = float(np.abs(got[k].astype(np.float64) - sc["ref"][k][:n]).max())
        print(case, n, k, "max |device - fp64|", err, "tolerance", sc["tol"][k], "twin distance", sc["twin_dist"][k])
        assert np.isfinite(got[k]).all() and err <= sc["tol"][k], (case, n, k, err, sc["tol"][k])
    assert np.array_equal(got["carry"], sc["nxt"][:n])
    patched = np.where(sc["dones"][:n, None], sc["term"][:n], sc["nxt"][:n])
    assert np.array_equal(got["replay_s"], sc["prev"][:n]) and np.array_equal(got["replay_ns"], patched)
    assert int(pk.counters(n).abs().sum()) == 0


@pytest.mark.parametrize("case", AMP)
def test_project_packer_equals_the_independent_packer(case):
    from isaacgymloco_amd.learn.fused_amp import PackedAmpDisc
    disc = G.amp_module(case).to(G.DEV)
    disc.device = G.DEV
    assert PackedAmpDisc.supported(disc)
    pk = PackedAmpDisc(disc, None, 64)
    for change in (False, True):
        if change:
            with torch.no_grad():
                for p in disc.parameters():
                    p.mul_(1.25)
            pk.refresh()
        d = {"hidden": [(m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy()) for m in (disc.trunk[0], disc.trunk[2])],
             "head_w": disc.amp_linear.weight.detach().cpu().numpy().reshape(-1), "head_b": disc.amp_linear.bias.detach().cpu().numpy()}
        packed = R.pack_amp(d)
        for i, pl in enumerate(packed["hidden"]):
            h = pk._D.hidden[i]
            assert (h.k_pad, h.n_pad, h.k_in, h.n_out) == (pl["k_pad"], pl["n_pad"], pl["k_in"], pl["n_out"])
            assert np.array_equal(pk.w[i].cpu().numpy().reshape(-1), pl["weight"]) and np.array_equal(pk.b[i].cpu().numpy(), pl["bias"])
        assert np.array_equal(pk.head_w.cpu().numpy(), packed["head_w"]) and np.array_equal(pk.head_b.cpu().numpy(), packed["head_b"])
    assert pk._D.amp_dim == R.AMP_CASES[case][0]
