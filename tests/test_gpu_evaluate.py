"""GPU: the evaluator launch (lsim_eval_accumulate) and learn/evaluate.py on a real device, against the float64 restatement of the semantics
(tests/eval_reference.py) replayed over per-step snapshots of the simulator's buffers.  Bounds: the ones tests/test_evaluate.py derives."""
import ctypes
import json

import numpy as np
import pytest

import eval_reference as REF
from helpers import C, abi

pytestmark = pytest.mark.gpu
W = abi.EVAL_WORDS
SNAP = {"rew": "rew", "reset_buf": "reset", "time_out_buf": "time_out", "commands": "commands", "base_lin_vel": "base_lin_vel", "base_ang_vel": "base_ang_vel",
        "root_states": "root_states", "dof_state": "dof_state", "torques": "torques", "actions": "actions", "last_actions": "last_actions",
        "contact_filt": "contact_filt", "contact_forces": "contact_forces", "terrain_types": "terrain_types", "terrain_levels": "terrain_levels"}


def case_cfg(num_envs, curriculum=True, delay=True):
    """Aliengo + Go2 on stairs and flat ground, episodes of 0.6 s (30 steps) so that time-outs happen within 200 steps; the terrain curriculum
    stays on so that levels change at resets (the case the group latch exists for)"""
    cfg = C.mixed_cfg("aliengo", {"aliengo": 0.5, "go2": 0.5})[0]
    cfg.env.num_envs = num_envs
    cfg.env.episode_length_s = 0.6
    cfg.terrain.num_rows, cfg.terrain.num_cols = 4, 4
    cfg.terrain.terrain_proportions = [0.25, 0.0, 0.0, 0.0, 0.4, 0.35]
    cfg.terrain.curriculum = curriculum
    cfg.commands.curriculum = False
    cfg.domain_rand.delay = delay
    return cfg


def seeded_actions(num_envs, steps, scale=3.0, seed=11):
    import torch
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(num_envs, 12, generator=g) * scale for _ in range(steps)]


def make_env(cfg, seed=5):
    from isaacgymloco_amd.envs.legged_robot import LeggedRobot
    env = LeggedRobot(cfg, sim_device="cuda:0", seed=seed)
    env.reset()
    return env


def snapshot(env, ev):
    b = {k: env.buf[name].cpu().numpy().copy() for k, name in SNAP.items()}
    b["torque_limits"] = ev._const["torque_limits"].cpu().numpy()
    return b


def run_case(num_envs=256, steps=200, group_by=("robot", "type", "level"), trace_envs=(0, 7, 255), snap=False, cfg=None):
    from isaacgymloco_amd.learn.evaluate import Evaluator
    env = make_env(cfg or case_cfg(num_envs))
    ev = Evaluator(env, group_by=group_by, trace_envs=trace_envs, trace_capacity=steps)
    snaps = []
    for a in seeded_actions(num_envs, steps):
        env.step_device(a.to("cuda:0"))
        ev.accumulate()
        if snap:
            snaps.append(snapshot(env, ev))
    table, trace = ev.table.cpu().numpy().copy(), ev.trace_buf.cpu().numpy().copy()
    return env, ev, table, trace, snaps


def test_tables_and_traces_match_the_reference_replay():
    """N = 256, 200 steps, snapshots after every step replayed through the float64 reference: counts equal, fixed-point words within the derived
    bound, trace rows equal their sources"""
    env, ev, table, trace, snaps = run_case(snap=True)
    ref = REF.RefEvaluator(256, 2, ev.num_types, ev.num_levels, ev.mask, robot_ids=env.robot_ids.cpu().numpy())
    for b in snaps:
        ref.step(b)
    T = ref.table
    groups_with = lambda w: int((T[:, REF.W[w]] > 0).sum())
    print("time-outs", int(T[:, REF.W["time_outs"]].sum()), "in", groups_with("time_outs"), "groups; falls", int(T[:, REF.W["falls"]].sum()), "in", groups_with("falls"), "groups")
    assert groups_with("time_outs") >= 2 and groups_with("falls") >= 2, "the input must end episodes both ways in several groups"
    assert len({tuple(b["terrain_levels"]) for b in snaps}) > 1, "levels must change at resets"
    for name in REF.EXACT_WORDS:
        np.testing.assert_array_equal(table[:, W[name]], T[:, REF.W[name]], err_msg=name)
    bound = ref.bound()
    for name in REF.FIX_WORDS:
        diff = np.abs(table[:, W[name]].astype(np.float64) - T[:, REF.W[name]].astype(np.float64))
        bd = bound[:, REF.W[name]]
        print(f"{name:>18}: max |diff| {diff.max():.3e} words, bound there {bd[diff.argmax()]:.3e}")
        assert (diff <= bd).all(), (name, diff.max(), bd[diff.argmax()])
    assert table[:, W["samples"]].sum() + table[:, W["episodes"]].sum() == 256 * 200
    assert table[:, W["nonfinite"]].sum() == 0 and int(env.nonfinite_envs.item()) == 0
    scale, q0 = ev._const["action_scale"].cpu().numpy(), ev._const["default_dof_pos"].cpu().numpy()
    feet = [int(v) for v in env.model.feet_bodies]
    for t in (0, 1, 57, 199):
        for k, i in enumerate((0, 7, 255)):
            want = REF.trace_row(snaps[t], i, feet, scale, q0)
            np.testing.assert_array_equal(trace[t, k, 12:], want[12:].astype(np.float32))
            prod = snaps[t]["actions"][i].astype(np.float64) * scale[i].astype(np.float64)
            ulp = np.spacing(np.maximum(np.abs(prod), np.abs(prod + q0[i])).astype(np.float32)).astype(np.float64)     # see tests/test_evaluate.py: target_ulp
            assert (np.abs(trace[t, k, :12].astype(np.float64) - want[:12]) <= ulp).all()


def test_same_run_twice_is_bitwise_equal():
    _, _, t1, r1, _ = run_case()
    _, _, t2, r2, _ = run_case()
    np.testing.assert_array_equal(t1, t2)
    np.testing.assert_array_equal(r1.view(np.uint32), r2.view(np.uint32))


def test_captured_step_and_accumulate_replay_equals_eager():
    """lsim_step + lsim_eval_accumulate captured in ONE single-stream graph and replayed 60 times == the same 60 steps launched eagerly.
    lsim_step passes its step counter (the Philox step word) to the kernels by value, so a captured step replays the counter it was captured
    with; the eager twin is given that same counter before every step (lsim_set_step_counter), which makes the two runs the same computation.
    Action delay off: its draw is keyed by the counter alone and would be the same in both runs anyway; curricula off."""
    import torch
    from isaacgymloco_amd.learn.evaluate import Evaluator
    steps, N = 60, 256
    acts = [a.to("cuda:0") for a in seeded_actions(N, steps)]
    out = []
    for mode in ("eager", "graph"):
        env = make_env(case_cfg(N, curriculum=False))
        ev = Evaluator(env, trace_envs=(3, 200), trace_capacity=steps)
        static = torch.zeros(N, 12, device="cuda:0")
        c0 = ctypes.c_int64()
        env._L.lsim_get_step_counter(env._h, ctypes.byref(c0))
        torch.cuda.synchronize()
        if mode == "graph":
            state0, table0 = ev.state.clone(), ev.table.clone()
            arena0 = env._arena.clone()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                env.step_device(static)
                ev.accumulate()
            torch.cuda.synchronize()
            env._arena.copy_(arena0); ev.state.copy_(state0); ev.table.copy_(table0); ev.trace_buf.zero_()     # whatever capture ran or not: start clean
        for a in acts:
            static.copy_(a)
            if mode == "graph":
                g.replay()
            else:
                env._L.lsim_set_step_counter(env._h, ctypes.c_int64(c0.value))
                env.step_device(static)
                ev.accumulate()
        torch.cuda.synchronize()
        out.append((ev.table.cpu().numpy().copy(), ev.trace_buf.cpu().numpy().copy(), ev.steps))
    assert out[0][2] == out[1][2] == steps
    assert out[0][0][:, W["episodes"]].sum() > 0
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1].view(np.uint32), out[1][1].view(np.uint32))


def test_group_masks_sum_to_the_ungrouped_table_at_4096():
    tables = {}
    for by in ((), ("robot",), ("type", "level"), ("robot", "type", "level")):
        env, ev, table, _, _ = run_case(num_envs=4096, steps=40, group_by=by, trace_envs=())
        assert table[:, W["nonfinite"]].sum() == 0 and int(env.nonfinite_envs.item()) == 0
        tables[by] = table
    flat = tables[()]
    assert flat.shape[0] == 1 and flat[0, W["samples"]] + flat[0, W["episodes"]] == 4096 * 40
    for by, t in tables.items():
        total = t.sum(axis=0)
        total[W["peak_torque_ratio"]] = t[:, W["peak_torque_ratio"]].max()
        np.testing.assert_array_equal(total, flat[0], err_msg=str(by))


@pytest.mark.parametrize("fused", [True, False])
def test_evaluate_end_to_end_reads_and_never_writes(fused):
    import torch
    from isaacgymloco_amd.learn.evaluate import evaluate, play_cfg
    from isaacgymloco_amd.learn.modules import HIMActorCritic
    N, steps = 1024, 50
    cfg = play_cfg(case_cfg(N))
    env = make_env(cfg)
    torch.manual_seed(3)
    ac = HIMActorCritic(env.num_obs, env.num_privileged_obs, env.num_one_step_obs, env.num_actions).to("cuda:0")
    recorded = []
    step_device = env.step_device
    env.step_device = lambda a, flags=0: (recorded.append(a.clone()), step_device(a, flags))[1]
    ev = evaluate(env, ac, steps, commands=(1.0, 0.0, 0.0), trace_envs=(0, 1023), fused=fused)
    res = ev.result()
    assert json.loads(json.dumps(res)) == res
    assert res["steps"] == steps and len(recorded) == steps
    assert sum(g["samples"] + g["episodes"] for g in res["groups"]) == N * steps == res["total"]["samples"] + res["total"]["episodes"]
    assert {g["key"]["robot"] for g in res["groups"]} == {"aliengo", "go2"}
    for g in res["groups"] + [res["total"]]:
        for k in ("lin_vel_error_mean", "lin_vel_error_rms", "yaw_rate_error_rms", "mechanical_power_mean", "torque_rms", "action_rate_mean",
                  "feet_in_contact_mean", "torque_saturation_rate", "peak_torque_ratio"):
            assert np.isfinite(g[k]), (g.get("key"), k)
    assert res["nonfinite"] == {"addends": 0, "simulator_env_steps": 0}
    tr = ev.trace()
    assert tr["dof_pos_target"].shape == (steps, 2, 12) and tr["root_pos"].shape == (steps, 2, 3) and tr["reset"].shape == (steps, 2, 1)
    np.testing.assert_array_equal(tr["commands"][-1], np.tile(np.float32([1.0, 0.0, 0.0]), (2, 1)))
    # the same actions on a twin env WITHOUT an evaluator: every simulator buffer equal, bit for bit
    twin = make_env(cfg)
    cmd = torch.tensor([1.0, 0.0, 0.0], device="cuda:0")
    for a in recorded:
        twin.commands[:, :3] = cmd
        twin.step_device(a)
    torch.cuda.synchronize()
    for name in env.buf:
        assert torch.equal(env.buf[name].view(torch.uint8), twin.buf[name].view(torch.uint8)), name
