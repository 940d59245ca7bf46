"""Deployment export: export_policy_as_jit / PolicyExporterHIM (HLP:201-264) and checkpoint interchange with the
reference's own classes.  CPU; the reference side is stored under tests/golden/."""
import os

import numpy as np
import torch

from isaacgymloco_amd.learn.export import PolicyExporterHIM, export_policy_as_jit
from isaacgymloco_amd.learn.modules import HIMActorCritic


def _policy(seed=3):
    torch.manual_seed(seed)
    ac = HIMActorCritic(270, 238, 45, 12, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128], activation="elu", init_noise_std=1.0)
    with torch.no_grad():      # move away from the initialisation so that every parameter matters
        for p in ac.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return ac


def test_exported_torchscript_reproduces_act_inference(tmp_path):
    ac = _policy()
    path = export_policy_as_jit(ac, str(tmp_path / "exported" / "policies"))
    assert os.path.basename(path) == "policy.pt"                       # the file name play.py's consumers expect (HLP:259)
    mod = torch.jit.load(path)
    obs = torch.randn(37, 270)
    with torch.no_grad():
        want = ac.act_inference(obs)
        got = mod(obs)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=1e-6)
    assert sorted(mod.state_dict()) == sorted(PolicyExporterHIM(ac).state_dict())
    assert all(k.startswith(("actor.", "estimator.")) for k in mod.state_dict())      # the reference exporter's module tree


def test_reference_classes_load_a_build_checkpoint(tmp_path):
    """a checkpoint saved with the runner's keys has exactly the parameter names, order and shapes of the reference's HIMActorCritic (what
    its play.py / runner.load need for a STRICT load and for the optimiser state) and gives the reference's act_inference / evaluate outputs
    to 1e-6; the reference's own exporter and ours write modules with identical outputs and module trees.  The reference side is stored in
    tests/golden/export_reference.npz (tools/gen_golden_export.py: the reference's classes on this same seeded checkpoint)."""
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "export_reference.npz"))
    ac = _policy(seed=5)
    ck = str(tmp_path / "model_7.pt")
    opt = torch.optim.Adam(ac.parameters(), lr=1e-3)
    torch.save({"model_state_dict": ac.state_dict(), "optimizer_state_dict": opt.state_dict(),
                "estimator_optimizer_state_dict": ac.estimator.optimizer.state_dict(), "iter": 7, "infos": None}, ck)   # HIMR:233-240
    d = torch.load(ck, weights_only=False)
    pad = lambda shape: list(shape) + [0] * (2 - len(shape))
    sd = d["model_state_dict"]
    assert list(sd) == fx["state_dict_keys"].tolist() and [pad(v.shape) for v in sd.values()] == fx["state_dict_shapes"].tolist()   # strict load
    assert [n for n, _ in ac.named_parameters()] == fx["param_names"].tolist()          # HIMR:247-249 load_optimizer=True: same parameter order
    assert [pad(p.shape) for p in ac.parameters()] == fx["param_shapes"].tolist()
    assert len(d["optimizer_state_dict"]["param_groups"][0]["params"]) == len(fx["param_names"])
    back = HIMActorCritic(270, 238, 45, 12, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128], activation="elu", init_noise_std=1.0)
    back.load_state_dict(sd)
    obs, crit = torch.from_numpy(fx["obs"]), torch.from_numpy(fx["crit"])
    with torch.no_grad():
        np.testing.assert_allclose(back.act_inference(obs).numpy(), fx["act_inference"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(back.evaluate(crit).numpy(), fx["evaluate"], rtol=0, atol=1e-6)
    mine = torch.jit.load(export_policy_as_jit(ac, str(tmp_path / "exp")))
    with torch.no_grad():
        np.testing.assert_allclose(mine(obs).numpy(), fx["exported"], rtol=0, atol=1e-6)
    assert sorted(mine.state_dict()) == fx["exporter_state_dict_keys"].tolist()
