"""TEST INFRASTRUCTURE -- shared by tests/test_mixed_robots.py (lane emulator) and tests/test_gpu_mixed_robots.py (HIP library): a mixed
instance (config.mixed_cfg, lsim_create_mixed) against one single-robot instance per robot, same N, seed and terrain, stepped with the same
seeded actions.  Every per-env buffer row of robot k's envs must equal the single-robot instance of robot k bit for bit."""
import copy

import torch

from helpers import C

# buffers that are not indexed by env
SHARED_BUFFERS = {"stats", "nonfinite", "height_grid", "terrain_origins", "terrain_mesh"}
MIXES = {
    "aliengo+go2": {"aliengo": 0.5, "go2": 0.5},
    "aliengo+go1+go2": {"aliengo": 0.5, "go1": 0.25, "go2": 0.25},
}


def mixed_and_single_cfgs(mix, terrain, num_envs, curriculum=False):
    """the mixed env config and the single-robot config of each of its robots"""
    cfg, _ = C.mixed_cfg("aliengo", MIXES[mix])
    if terrain == "flat":
        cfg.terrain.terrain_proportions = [1.0, 0.0, 0.0, 0.0]
    else:
        cfg.terrain = copy.deepcopy(C.aliengo_stairs_cfg().terrain)
    cfg.env.num_envs = num_envs
    cfg.commands.curriculum = curriculum
    return cfg, [C.robot_cfg(cfg, k) for k in range(len(cfg.robots))]


def per_env_buffers(env):
    return {k: v for k, v in env.buf.items() if k not in SHARED_BUFFERS and v.shape[0] == env.num_envs}


def assert_rows_equal(mixed, singles, what):
    ids = mixed.robot_ids
    bufs = per_env_buffers(mixed)
    assert {"obs", "priv_obs", "rew", "reset", "time_out", "root_states", "dof_state", "rigid_body_states", "contact_forces", "torques",
            "episode_sums", "terrain_levels"} <= set(bufs)
    for k, single in enumerate(singles):
        rows = (ids == k).nonzero(as_tuple=False).flatten()
        assert rows.numel() > 0
        for name, b in bufs.items():
            a = b[rows].reshape(rows.numel(), -1).contiguous().view(torch.uint8)        # bit patterns (NaN rows compare too)
            s = single.buf[name][rows].reshape(rows.numel(), -1).contiguous().view(torch.uint8)
            if not torch.equal(a, s):
                bad = (a != s).any(dim=1).nonzero().flatten()
                raise AssertionError(f"{what}: buffer {name!r}, robot {k} ({mixed.robot_names[k]}): envs {rows[bad].tolist()[:8]} differ")


def run_lockstep(make_env, mix, terrain, num_envs, steps, reset_at, seed=5):
    """create the mixed env and the single-robot envs with make_env(cfg, seed), step them in lock step; compare after creation, after
    reset(), after every step and after a reset_idx on a subset.  Returns the mixed env."""
    cfg, single_cfgs = mixed_and_single_cfgs(mix, terrain, num_envs)
    mixed = make_env(cfg, seed)
    singles = [make_env(c, seed) for c in single_cfgs]
    envs = [mixed] + singles
    assert mixed.robot_names == list(MIXES[mix])
    assert_rows_equal(mixed, singles, "after creation")
    for e in envs:
        e.reset()
    assert_rows_equal(mixed, singles, "after reset()")
    gen = torch.Generator().manual_seed(11)
    subset = torch.arange(1, num_envs, 3)
    for t in range(steps):
        actions = (torch.randn(num_envs, 12, generator=gen) * 0.6).to(mixed.device)
        for e in envs:
            e.step(actions)
        assert_rows_equal(mixed, singles, f"step {t}")
        if t == reset_at:
            for e in envs:
                e.reset_idx(subset.to(mixed.device))
            assert_rows_equal(mixed, singles, f"reset_idx after step {t}")
    for e in singles:
        e.close()
    return mixed
