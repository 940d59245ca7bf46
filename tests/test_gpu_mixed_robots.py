"""GPU: several quadrupeds in one environment instance through the HIP library (lsim_create_mixed).  Every per-env row of robot k equals the
single-robot instance of robot k bit for bit (CPU counterpart: tests/test_mixed_robots.py), and a mixed env trains like any other."""
import math

import pytest
import torch

from mixed_robots_common import MIXES, mixed_and_single_cfgs, run_lockstep

pytestmark = pytest.mark.gpu


def _make(cfg, seed):
    from isaacgymloco_amd.envs.legged_robot import LeggedRobot
    return LeggedRobot(cfg, sim_device="cuda:0", seed=seed)


@pytest.mark.parametrize("terrain", ["flat", "stairs"])
@pytest.mark.parametrize("mix", list(MIXES))
def test_gpu_mixed_rows_equal_single_robot_instances(mix, terrain):
    """N = 4096, TGS, command curriculum off: 100 env-steps with the same seeded actions and one reset_idx on a subset"""
    env = run_lockstep(_make, mix, terrain, num_envs=4096, steps=100, reset_at=50)
    assert int(env.nonfinite_envs) == 0
    env.close()


def test_gpu_mixed_env_drives_the_runner():
    """Aliengo + Go2 at N = 4096 with the command curriculum on: two iterations of HIMOnPolicyRunner.learn"""
    from isaacgymloco_amd.learn.bench_train import train_cfg_dict
    from isaacgymloco_amd.learn.runner import HIMOnPolicyRunner
    cfg, _ = mixed_and_single_cfgs("aliengo+go2", "flat", 4096, curriculum=True)
    env = _make(cfg, 3)
    assert env.robot_ids.shape == (4096,) and env.default_dof_pos.shape == (4096, 12)
    tc = train_cfg_dict("aliengo")
    tc["runner"]["num_steps_per_env"] = 24
    torch.manual_seed(0)
    run = HIMOnPolicyRunner(env, tc, log_dir=None, device="cuda:0")
    run.learn(2, init_at_random_ep_len=True)
    losses = [float(x) for x in run.last_update[:4]]
    assert all(math.isfinite(x) for x in losses), losses
    assert all(torch.isfinite(v).all() for v in run.alg.actor_critic.state_dict().values())
    assert int(env.nonfinite_envs) == 0
    env.close()
