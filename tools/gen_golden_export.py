"""tests/golden/export_reference.npz: what the reference's own classes give for the checkpoint tests/test_export.py builds -- the parameter
names and shapes of its HIMActorCritic (a strict state-dict load and the optimiser state depend on both), its act_inference / evaluate on
seeded observations, and the outputs and module tree of its policy exporter (HLP:248-264) scripted on its own module.

    python tools/gen_golden_export.py PATH/TO/rsl_rl"""
import copy
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, os.path.join(HERE, ".."))


def main(rsl_rl):
    sys.path.insert(0, rsl_rl)
    from rsl_rl.modules import HIMActorCritic as RefAC
    from test_export import _policy
    ac = _policy(seed=5)
    ref = RefAC(270, 238, 45, 12, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128], activation="elu", init_noise_std=1.0)
    ref.load_state_dict(ac.state_dict())
    g = torch.Generator().manual_seed(11)
    obs, crit = torch.randn(29, 270, generator=g), torch.randn(29, 238, generator=g)

    class RefExporter(torch.nn.Module):       # the reference exporter, HLP:248-264 (legged_gym.utils.helpers imports isaacgym)
        def __init__(self, actor_critic):
            super().__init__()
            self.actor = copy.deepcopy(actor_critic.actor)
            self.estimator = copy.deepcopy(actor_critic.estimator.encoder)

        def forward(self, obs_history):
            parts = self.estimator(obs_history)[:, 0:19]
            vel, z = parts[..., :3], parts[..., 3:]
            z = F.normalize(z, dim=-1, p=2.0)
            return self.actor(torch.cat((obs_history[:, 0:45], vel, z), dim=1))
    script = torch.jit.script(RefExporter(ref))
    with torch.no_grad():
        act, value, exported = ref.act_inference(obs), ref.evaluate(crit), script(obs)
    names = [n for n, _ in ref.named_parameters()]
    keys = list(ref.state_dict())
    np.savez(os.path.join(HERE, "..", "tests", "golden", "export_reference.npz"), obs=obs.numpy(), crit=crit.numpy(),
             act_inference=act.numpy(), evaluate=value.numpy(), exported=exported.numpy(),
             param_names=np.array(names), param_shapes=np.array([list(p.shape) + [0] * (2 - p.dim()) for p in ref.parameters()]),
             state_dict_keys=np.array(keys), state_dict_shapes=np.array([list(v.shape) + [0] * (2 - v.dim()) for v in ref.state_dict().values()]),
             exporter_state_dict_keys=np.array(sorted(script.state_dict())))


if __name__ == "__main__":
    main(sys.argv[1])
