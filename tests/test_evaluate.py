"""Policy evaluation on the device (include/lsim.h lsim_eval_*, isaacgymloco_amd/learn/evaluate.py), the checks that need no GPU: the kernel
source compiled for the CPU (tests/emu/emu_eval.cpp) against a float64 restatement of the documented semantics (tests/eval_reference.py), the
Python layer's bookkeeping, the command line's argument errors and the host-side argument checks of the HIP library."""
import ctypes
import json

import numpy as np
import pytest

import eval_reference as REF
from eval_emu_binding import FIELDS, EmuApi, EmuEval
from helpers import C, abi

W = abi.EVAL_WORDS
N_SYN, STEPS_SYN, R_SYN, T_SYN, L_SYN = 96, 300, 2, 3, 4
FEET = (4, 8, 12, 16)


def synthetic_script(seed=0, N=N_SYN, steps=STEPS_SYN):
    """a 300-step episode script for 96 envs: random states, resets (time-outs and falls), level changes at reset, ONE NaN torque and ONE
    torque whose square lies beyond the addend clamp (2000^2 > 2^20)"""
    rs = np.random.RandomState(seed)
    const = {"robot_ids": (np.arange(N) % R_SYN).astype(np.uint8), "torque_limits": np.tile(rs.uniform(20, 45, (1, 12)), (N, 1)).astype(np.float32),
             "default_dof_pos": rs.uniform(-1, 1, (N, 12)).astype(np.float32), "action_scale": rs.uniform(0.1, 0.5, (N, 12)).astype(np.float32)}
    types = rs.randint(0, T_SYN, N).astype(np.int64)
    levels = rs.randint(0, L_SYN, N).astype(np.int64)
    out = []
    for t in range(steps):
        b = {k: None for k in FIELDS}
        b.update(const)
        reset = rs.rand(N) < 0.02
        b["reset_buf"] = reset.astype(np.uint8)
        b["time_out_buf"] = (reset & (rs.rand(N) < 0.5)).astype(np.uint8)
        levels = np.where(reset, rs.randint(0, L_SYN, N), levels).astype(np.int64)       # on a reset step the buffer already holds the next level
        b["terrain_levels"], b["terrain_types"] = levels.copy(), types.copy()
        b["rew"] = rs.normal(0.02, 0.05, N).astype(np.float32)
        b["commands"] = rs.uniform(-1, 1, (N, 4)).astype(np.float32)
        b["base_lin_vel"] = rs.normal(0, 0.7, (N, 3)).astype(np.float32)
        b["base_ang_vel"] = rs.normal(0, 0.7, (N, 3)).astype(np.float32)
        b["root_states"] = rs.normal(0, 3.0, (N, 13)).astype(np.float32)
        b["dof_state"] = rs.normal(0, 4.0, (N, 12, 2)).astype(np.float32)
        b["torques"] = rs.normal(0, 20.0, (N, 12)).astype(np.float32)
        b["actions"] = rs.normal(0, 1.5, (N, 12)).astype(np.float32)
        b["last_actions"] = rs.normal(0, 1.5, (N, 12)).astype(np.float32)
        b["contact_filt"] = (rs.rand(N, 4) < 0.5).astype(np.uint8)
        b["contact_forces"] = rs.normal(0, 50.0, (N, 17, 3)).astype(np.float32)
        if t == 17:
            b["torques"][5, 7] = np.nan
            b["reset_buf"][5] = 0
            b["time_out_buf"][5] = 0
        if t == 23:
            b["torques"][11, 2] = 2000.0
            b["reset_buf"][11] = 0
            b["time_out_buf"][11] = 0
        out.append(b)
    return out


def run_emu(script, group_by, order=None, trace_envs=(), trace_capacity=1):
    ev = EmuEval(N_SYN, R_SYN, T_SYN, L_SYN, group_by, trace_envs=trace_envs, trace_capacity=trace_capacity, feet_bodies=FEET)
    for b in script:
        for k, arr in b.items():
            ev.bufs[k][...] = arr
        ev.accumulate(order)
    return ev


def run_ref(script, group_by):
    ref = REF.RefEvaluator(N_SYN, R_SYN, T_SYN, L_SYN, group_by, robot_ids=script[0]["robot_ids"])
    for b in script:
        ref.step(b)
    return ref


def compare_tables(table, ref):
    """count words (and the return) equal; fixed-point words within the reference's derived bound; returns the worst |diff| / bound"""
    for name in REF.EXACT_WORDS:
        np.testing.assert_array_equal(table[:, W[name]], ref.table[:, REF.W[name]], err_msg=name)
    bound = ref.bound()
    worst = 0.0
    for name in REF.FIX_WORDS:
        diff = np.abs(table[:, W[name]].astype(np.float64) - ref.table[:, REF.W[name]].astype(np.float64))
        bd = bound[:, REF.W[name]]
        print(f"{name:>18}: max |diff| {diff.max():.3e} words, bound there {bd[diff.argmax()]:.3e}")
        assert (diff <= bd).all(), (name, diff.max(), bd[diff.argmax()])
        worst = max(worst, float((diff / np.maximum(bd, 1.0)).max()))
    return worst


def test_word_names_follow_the_header():
    assert [n for n, _ in sorted(W.items(), key=lambda kv: kv[1])] == [n for n, _ in sorted(REF.W.items(), key=lambda kv: kv[1])]
    from isaacgymloco_amd.learn import evaluate as E
    assert E.TRACE_COLUMNS == {k: (a, b - a) for k, (a, b) in REF.TRACE_COLS.items()}
    assert abi.ABI_VERSION == 7


def test_kernel_source_on_cpu_matches_reference():
    script = synthetic_script()
    by = REF.BY_ROBOT | REF.BY_TYPE | REF.BY_LEVEL
    ev, ref = run_emu(script, by), run_ref(script, by)
    assert ref.table[:, REF.W["time_outs"]].sum() > 0 and ref.table[:, REF.W["falls"]].sum() > 0
    assert ref.table[:, REF.W["nonfinite"]].sum() == 3          # the NaN torque: power, torque_sq and the peak candidate of that one sample
    assert (ref.table[:, REF.W["episodes"]] > 0).sum() >= 2
    compare_tables(ev.table, ref)
    # samples + episodes = env-steps
    assert ev.table[:, W["samples"]].sum() + ev.table[:, W["episodes"]].sum() == N_SYN * STEPS_SYN
    # the clamp: the 2000 N m torque's square entered as exactly 2^20
    env11 = [b for b in script][23]
    assert float(env11["torques"][11, 2]) ** 2 > REF.CLAMP


def test_grouped_tables_sum_to_the_ungrouped_table_exactly():
    script = synthetic_script()
    flat = run_emu(script, 0).table
    assert flat.shape[0] == 1
    for by in (REF.BY_ROBOT, REF.BY_TYPE | REF.BY_LEVEL, REF.BY_ROBOT | REF.BY_TYPE | REF.BY_LEVEL):
        t = run_emu(script, by).table
        peak = W["peak_torque_ratio"]
        total = t.sum(axis=0)
        total[peak] = t[:, peak].max()
        np.testing.assert_array_equal(total, flat[0])


def test_env_order_does_not_change_the_table():
    script = synthetic_script()
    by = REF.BY_ROBOT | REF.BY_TYPE | REF.BY_LEVEL
    a = run_emu(script, by).table
    perm = np.random.RandomState(5).permutation(N_SYN).astype(np.int32)
    b = run_emu(script, by, order=perm).table
    np.testing.assert_array_equal(a, b)


def target_ulp(b, env):
    """1 ulp for dof_pos_target = a * scale + default formed in fp32: two roundings (the product, the sum; one if fused), each at most half an
    ulp of its own result, so at most one ulp of the larger of |a * scale| and |sum| -- the sum alone may be small by cancellation"""
    prod = b["actions"][env].astype(np.float64) * b["action_scale"][env].astype(np.float64)
    big = np.maximum(np.abs(prod), np.abs(prod + b["default_dof_pos"][env].astype(np.float64)))
    return np.spacing(big.astype(np.float32)).astype(np.float64)


def test_trace_rows_equal_their_sources():
    script = synthetic_script()[:40]
    envs, cap = (3, 95, 17), 16
    ev = run_emu(script, 0, trace_envs=envs, trace_capacity=cap)
    dim = abi.DEFINES["LSIM_EVAL_TRACE_DIM"]
    assert ev.trace.shape == (cap, 3, dim)
    assert int(ev.state[:8].view(np.int64)[0]) == 40
    for t in range(40 - cap, 40):
        for k, env in enumerate(envs):
            want = REF.trace_row(script[t], env, FEET, script[t]["action_scale"], script[t]["default_dof_pos"])
            got = ev.trace[t % cap, k]
            np.testing.assert_array_equal(got[12:], want[12:].astype(np.float32))
            assert (np.abs(got[:12].astype(np.float64) - want[:12]) <= target_ulp(script[t], env)).all()


PLAY_OVERRIDES = {"terrain.curriculum": False, "terrain.max_init_terrain_level": 5, "noise.add_noise": False, "domain_rand.randomize_friction": False,
                  "domain_rand.push_robots": False, "domain_rand.disturbance": False, "domain_rand.randomize_payload_mass": False,
                  "commands.heading_command": False, "commands.curriculum": False, "commands.resampling_time": 10000.0}


def _get(cfg, dotted):
    for part in dotted.split("."):
        cfg = getattr(cfg, part)
    return cfg


@pytest.mark.parametrize("mixed", [False, True])
def test_play_cfg_overrides(mixed):
    from isaacgymloco_amd.learn.evaluate import play_cfg
    base = C.mixed_cfg("aliengo", {"aliengo": 0.5, "go2": 0.5})[0] if mixed else C.aliengo_cfg()
    before = json.dumps(base.to_dict(), sort_keys=True, default=str)
    num_envs = base.env.num_envs
    p = play_cfg(base)
    assert json.dumps(base.to_dict(), sort_keys=True, default=str) == before, "play_cfg must not modify its argument"
    for key, want in PLAY_OVERRIDES.items():
        assert _get(p, key) == want, key
    assert p.env.num_envs == num_envs
    assert list(p.asset.terminate_after_contacts_on) == list(base.asset.terminate_after_contacts_on)
    q = play_cfg(base, keep_terminations=False)
    assert list(q.asset.terminate_after_contacts_on) == []
    if mixed:
        assert [r["name"] for r in p.robots] == ["aliengo", "go2"]
        for k in range(2):
            assert list(C.robot_cfg(q, k).asset.terminate_after_contacts_on) == []
            assert C.robot_cfg(p, k).domain_rand.push_robots is False


def test_group_keys_round_trip():
    from isaacgymloco_amd.learn import evaluate as E
    names = ["aliengo", "go2"]
    for by in ((), ("robot",), ("type", "level"), ("robot", "type", "level")):
        mask = E.group_mask(by)
        shape = E.group_shape(mask, 2, 3, 4)
        n = shape[0] * shape[1] * shape[2]
        seen = set()
        for g in range(n):
            key = E.group_key(mask, shape, g, names)
            assert set(key) == set(by)
            assert E.key_index(mask, shape, key, names) == g
            seen.add(json.dumps(key, sort_keys=True))
        assert len(seen) == n
    assert E.group_index(E.group_mask(("robot", "type", "level")), (2, 3, 4), 1, 2, 3) == (1 * 3 + 2) * 4 + 3
    with pytest.raises(ValueError):
        E.group_mask(("robot", "terrain"))


def test_metrics_use_the_right_denominators():
    from isaacgymloco_amd.learn.evaluate import metrics_of_row, FIX_ONE
    row = np.zeros(abi.NUM_EVAL_WORDS, np.int64)
    row[W["samples"]], row[W["episodes"]], row[W["falls"]], row[W["time_outs"]] = 40, 4, 1, 3
    row[W["lin_err"]], row[W["lin_err_sq"]] = int(20 * FIX_ONE), int(160 * FIX_ONE)
    row[W["torque_sat"]], row[W["feet_contact"]], row[W["length"]] = 48, 80, 44
    row[W["return"]], row[W["distance"]], row[W["torque_sq"]] = int(-6 * FIX_ONE), int(10 * FIX_ONE), int(40 * 12 * 9 * FIX_ONE)
    m = metrics_of_row(row)
    assert m["lin_vel_error_mean"] == 0.5 and m["lin_vel_error_rms"] == 2.0 and m["torque_rms"] == 3.0
    assert m["torque_saturation_rate"] == 0.1 and m["feet_in_contact_mean"] == 2.0
    assert m["fall_rate"] == 0.25 and m["time_out_rate"] == 0.75
    assert m["episode_return_mean"] == -1.5 and m["episode_length_mean"] == 11.0 and m["episode_distance_mean"] == 2.5
    empty = metrics_of_row(np.zeros(abi.NUM_EVAL_WORDS, np.int64))
    assert empty["samples"] == 0 and np.isnan(empty["fall_rate"]) and np.isnan(empty["lin_vel_error_mean"])


def _emu_env(N=64, mixed=True, episode_length_s=0.4):
    from eval_emu_binding import emu_mixed_env
    from isaacgymloco_amd.learn.evaluate import play_cfg
    cfg = C.mixed_cfg("aliengo", {"aliengo": 0.5, "go2": 0.5})[0] if mixed else C.aliengo_cfg()
    cfg = play_cfg(cfg)
    cfg.env.num_envs = N
    cfg.env.episode_length_s = episode_length_s
    cfg.terrain.num_rows, cfg.terrain.num_cols = 4, 4
    cfg.terrain.terrain_proportions = [0.5, 0.0, 0.0, 0.0, 0.25, 0.25]
    return emu_mixed_env(cfg, seed=3)


def test_evaluator_result_schema_on_the_lane_emulator():
    """the Python layer end to end on the CPU: the product's LeggedRobot surface over the lane emulator of kernels A / B, the evaluator through
    the CPU shim of ITS kernel source.  Terrain curriculum off, so groups never change: samples + episodes == env-steps in every group."""
    import torch
    from isaacgymloco_amd.learn.evaluate import Evaluator
    env = _emu_env()
    env.reset()
    ev = Evaluator(env, trace_envs=(0, 5), trace_capacity=8, api=EmuApi())
    steps = 30
    g = torch.Generator().manual_seed(0)
    for _ in range(steps):
        env.step_device(torch.randn(env.num_envs, 12, generator=g) * 3.0)
        ev.accumulate()
    res = ev.result()
    res2 = json.loads(json.dumps(res))
    assert res2["steps"] == steps and res2["num_envs"] == 64 and res2["group_by"] == ["robot", "type", "level"]
    assert res2["conventions"]["abi_version"] == abi.ABI_VERSION and res2["conventions"]["robot_names"] == ["aliengo", "go2"]
    assert res2["conventions"]["torque_saturation_threshold"] == 0.98 and res2["conventions"]["addend_clamp"] == 2.0 ** 20
    assert res2["conventions"]["robots"]["names"] == ["aliengo", "go2"]
    assert res2["nonfinite"] == {"addends": 0, "simulator_env_steps": 0}
    members = {}
    for r, t, l in zip(env.robot_ids.tolist(), env.terrain_types.tolist(), env.terrain_levels.tolist()):
        members[(env.robot_names[r], t, l)] = members.get((env.robot_names[r], t, l), 0) + 1
    assert len(res2["groups"]) == len(members) >= 4
    for grp in res2["groups"]:
        k = grp["key"]
        assert grp["samples"] + grp["episodes"] == members[(k["robot"], k["type"], k["level"])] * steps
        assert grp["episodes"] == grp["falls"] + grp["time_outs"]
        assert all(np.isfinite(grp[m]) for m in ("lin_vel_error_rms", "mechanical_power_mean", "torque_rms", "peak_torque_ratio"))
    tot = res2["total"]
    assert tot["samples"] + tot["episodes"] == 64 * steps and tot["time_outs"] >= 1 and tot["falls"] >= 1      # episode_length_s = 0.4 s = 20 steps; actions of 3 sigma throw some robots over
    assert tot["peak_torque_ratio"] == max(grp["peak_torque_ratio"] for grp in res2["groups"])
    tr = ev.trace()
    assert tr["step"].tolist() == list(range(steps - 8, steps)) and tr["envs"].tolist() == [0, 5]
    assert tr["dof_pos"].shape == (8, 2, 12) and tr["commands"].shape == (8, 2, 3) and tr["contact_forces_z"].shape == (8, 2, 4) and tr["rew"].shape == (8, 2, 1)
    np.testing.assert_array_equal(tr["dof_pos"][-1], env.dof_pos[[0, 5]].numpy())
    np.testing.assert_array_equal(tr["root_quat"][-1], env.root_states[[0, 5], 3:7].numpy())
    np.testing.assert_array_equal(tr["contact_forces_z"][-1], env.contact_forces[[0, 5]][:, env.feet_indices, 2].numpy())


def test_action_scales_hold_the_hip_reduction_per_robot():
    env = _emu_env(N=8)
    assert tuple(env.action_scales.shape) == (8, 12)
    for i in range(8):
        lc = env._robot_lcfgs[int(env.robot_ids[i])]
        want = [np.float32(lc.action_scale) * (np.float32(lc.hip_reduction) if j % 3 == 0 else np.float32(1)) for j in range(12)]
        np.testing.assert_allclose(env.action_scales[i].numpy(), want, rtol=1e-7)


@pytest.mark.parametrize("argv", [
    ["--task", "aliengo", "--checkpoint", "m.pt"],                                                       # --out missing
    ["--task", "nope", "--checkpoint", "m.pt", "--out", "o.json"],
    ["--task", "aliengo", "--checkpoint", "m.pt", "--out", "o.json", "--commands", "1,2"],
    ["--task", "aliengo", "--checkpoint", "m.pt", "--out", "o.json", "--commands", "a,b,c"],
    ["--task", "aliengo", "--checkpoint", "m.pt", "--out", "o.json", "--envs", "0"],
    ["--task", "aliengo", "--checkpoint", "m.pt", "--out", "o.json", "--group-by", "robot,terrain"],
    ["--task", "aliengo", "--checkpoint", "m.pt", "--out", "o.json", "--trace-envs", "0,1"],             # no --trace-out
    ["--task", "aliengo", "--checkpoint", "m.pt", "--out", "o.json", "--envs", "8", "--trace-envs", "8", "--trace-out", "t.npz"],
    ["--task", "aliengo", "--checkpoint", "m.pt", "--out", "o.json", "--robots", "aliengo:0.5"],
])
def test_cli_argument_errors(argv):
    from isaacgymloco_amd.learn.evaluate import parse_args
    with pytest.raises(SystemExit):
        parse_args(argv)


def test_cli_parses_a_full_command_line():
    from isaacgymloco_amd.learn.evaluate import parse_args
    a = parse_args(["--task", "aliengo", "--robots", "aliengo=0.5,go2=0.5", "--checkpoint", "m.pt", "--envs", "128", "--steps", "10", "--commands", "1.0,0,0",
                    "--out", "o.json", "--trace-envs", "0,1", "--trace-out", "t.npz"])
    assert a.robots == {"aliengo": 0.5, "go2": 0.5} and a.commands == (1.0, 0.0, 0.0) and a.trace_envs == (0, 1) and a.group_by == ("robot", "type", "level")


def _valid_struct():
    ev = EmuEval(64, 2, 3, 4, 7, trace_envs=(1, 2), trace_capacity=4)
    return ev, ev.e


@pytest.mark.parametrize("which", ["emu", "hip"])
def test_host_side_argument_checks(which):
    """LSIM_E_INVALID before any launch; "hip" goes through the cross-compiled HIP library (loading it needs no GPU; only INVALID structs are passed)"""
    if which == "hip":
        from isaacgymloco_amd import lib
        L = lib.load()
        sizes, clear, acc = L.lsim_eval_sizes, (lambda e: L.lsim_eval_clear(e, None)), (lambda e: L.lsim_eval_accumulate(e, None))
    else:
        api = EmuApi()
        sizes, clear, acc = api.lsim_eval_sizes, (lambda e: api.lsim_eval_clear(e, None)), (lambda e: api.lsim_eval_accumulate(e, None))
    INV = abi.E_INVALID
    s = [ctypes.c_size_t() for _ in range(3)]
    refs = [ctypes.byref(v) for v in s]
    assert sizes(4096, 24, 2, 100, *refs) == 0
    assert s[1].value == 24 * abi.NUM_EVAL_WORDS * 8 and s[2].value == 100 * 2 * abi.DEFINES["LSIM_EVAL_TRACE_DIM"] * 4 and s[0].value >= 4096 * 32
    assert sizes(4096, 0, 0, 1, *refs) == INV
    assert sizes(4096, abi.DEFINES["LSIM_EVAL_MAX_GROUPS"] + 1, 0, 1, *refs) == INV
    assert sizes(4096, 24, 65, 1, *refs) == INV
    assert sizes(4096, 24, 0, 0, *refs) == INV
    assert sizes(0, 24, 0, 1, *refs) == INV
    assert sizes(4096, 24, 0, 1, None, refs[1], refs[2]) == INV
    assert clear(None) == INV and acc(None) == INV
    keep, e = _valid_struct()

    def broken(**kw):
        c = abi.LsimEval.from_buffer_copy(e)
        for k, v in kw.items():
            setattr(c, k, v)
        return ctypes.byref(c)
    for fn in (clear, acc):
        assert fn(broken(torques=None)) == INV
        assert fn(broken(state=None)) == INV
        assert fn(broken(table=None)) == INV
        assert fn(broken(trace=None)) == INV                                  # two trace envs listed
        assert fn(broken(torques=e.torques + 4)) == INV                       # misaligned 16-byte rows
        assert fn(broken(table=e.table + 4)) == INV
        assert fn(broken(num_types=0)) == INV
        assert fn(broken(num_levels=-1)) == INV
        assert fn(broken(num_robots=5)) == INV
        assert fn(broken(num_groups=23)) == INV                               # not the product of the kept extents
        assert fn(broken(group_by=8)) == INV
        assert fn(broken(num_trace_envs=65)) == INV
        assert fn(broken(trace_capacity=0)) == INV
        c = abi.LsimEval.from_buffer_copy(e)
        c.trace_envs[1] = 64                                                  # >= num_envs
        assert fn(ctypes.byref(c)) == INV
        c = abi.LsimEval.from_buffer_copy(e)
        c.feet_bodies[0] = 17
        assert fn(ctypes.byref(c)) == INV
    if which == "emu":
        assert clear(ctypes.byref(e)) == 0 and acc(ctypes.byref(e)) == 0
        c = abi.LsimEval.from_buffer_copy(e)
        c.robot_ids = None                                                    # one robot: allowed
        c.num_robots, c.num_groups = 1, 12
        assert acc(ctypes.byref(c)) == 0
