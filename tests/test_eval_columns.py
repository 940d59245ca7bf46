"""Caller-supplied columns into the evaluator's groups (include/lsim.h lsim_eval_columns_*, learn/evaluate.py Evaluator.add_columns), the checks
that need no GPU: the kernel source compiled for the CPU (tests/emu/emu_eval_columns.cpp) against a numpy restatement of the documented
semantics, bit for bit; the host-side argument checks of the shim and of the HIP library; the Python layer through the shim."""
import ctypes
import json
import math

import numpy as np
import pytest

import eval_columns_emu_binding as CB
from helpers import C, abi

W = abi.EVAL_WORDS
SIZES = [1, 255, 256, 257, 700]


def run(N, num_cols, ld, big, order_seed=None):
    """three steps of CB.script through the shim and through the restatement; asserts word 0 == the main table's samples after every step"""
    steps, pair = CB.script(N, num_cols, ld, big)
    rig = CB.Rig(N, num_cols, ld, big)
    want = np.zeros_like(rig.table)
    for t, step in enumerate(steps):
        rig.feed(step)
        rig.ev.accumulate()
        order = None if order_seed is None else np.random.RandomState(order_seed + t).permutation(N).astype(np.int32)
        rig.accumulate_columns(order)
        CB.reference_add(want, rig.group1(), step["reset_buf"], step["values"], rig.groups, num_cols)
        np.testing.assert_array_equal(rig.table[:, 0], rig.ev.table[:, W["samples"]], err_msg=f"step {t}")
    return rig, want, steps, pair


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("num_cols,pad", [(1, 0), (1, 3), (6, 0), (6, 3)])
@pytest.mark.parametrize("N", SIZES)
def test_shim_equals_the_stated_semantics(N, num_cols, pad, big):
    rig, want, steps, pair = run(N, num_cols, num_cols + pad, big)
    np.testing.assert_array_equal(rig.table, want)
    assert rig.table[:, 0].sum() == sum(int((s["reset_buf"] == 0).sum()) for s in steps)
    if N >= 255:
        nonfinite = rig.table[:, 3::3].sum()
        assert nonfinite > 0 and rig.table[:, 1::3].any() and (rig.table[:, 2::3] >= 0).all()
        assert any(s["reset_buf"].any() for s in steps[1:])
    if big and N >= 255:
        assert (rig.table[:, 0] > 0).sum() > 100                    # many groups per block


def test_value_mix_holds_every_special_case():
    """what the tables above were fed: NaN, both infinities, values beyond the clamp, below the resolution, negative numbers, exact zeros; and
    what the semantics make of them"""
    steps, _ = CB.script(700, 6, 6, True)
    v = np.concatenate([s["values"].ravel() for s in steps])
    assert np.isnan(v).any() and (v == np.inf).any() and (v == -np.inf).any() and (v == np.float32(3e6)).any() and (v == np.float32(-3e6)).any()
    assert (v == np.float32(1e-12)).any() and (v == 0).any() and (v < 0).any() and (v == np.float32(1e30)).any()
    assert CB.fix(np.float32(3e6)) == 2 ** 52 and CB.fix(np.float32(-3e6)) == -2 ** 52 and CB.fix(np.float32(1e-12)) == 0
    assert CB.fix(np.float32(1.5)) == 3 * 2 ** 31 and CB.fix(np.float32(np.inf)) == 2 ** 52
    t = np.zeros((1, 4), np.int64)
    for val in (3e6, 1e30, -2.0, 1e-12, np.nan, np.inf):
        CB.reference_add(t, [1], [0], np.array([[val]], np.float32), 1, 1)
    assert t.tolist() == [[6, 2 ** 52 + 2 ** 52 - 2 * 2 ** 32, 2 ** 52 + 2 ** 52 + 4 * 2 ** 32, 2]]


def test_two_groups_of_one_block_share_a_start_slot():
    """the 320-group script puts envs 0 and 1 (the same block) into two groups whose first probe of the block's hash is the same slot"""
    a, b = CB.colliding_groups()
    assert a != b and CB.start_slot(a) == CB.start_slot(b)
    rig, want, steps, pair = run(257, 6, 6, True)
    assert pair == (a, b)
    g1 = rig.group1()
    assert (g1[0] - 1, g1[1] - 1) == (a, b)
    assert rig.table[a, 0] >= 3 and rig.table[b, 0] >= 3            # both envs sampled in all three steps (others may share the groups)
    np.testing.assert_array_equal(rig.table, want)
    # and the hash in numpy is the kernel's: a block of distinct groups fills distinct slots (the tables agree), 320 groups cannot all start apart
    assert len({CB.start_slot(g) for g in range(320)}) < 320


def test_launch_before_the_first_evaluator_launch_adds_nothing():
    steps, _ = CB.script(257, 6, 9, True)
    rig = CB.Rig(257, 6, 9, True)
    rig.feed(steps[0])
    rig.table[...] = 0
    rig.accumulate_columns()
    assert not rig.table.any() and not rig.group1().any()
    rig.ev.accumulate()
    rig.accumulate_columns()
    assert rig.table[:, 0].sum() == 257


@pytest.mark.parametrize("N,big", [(257, True), (700, True), (700, False)])
def test_env_order_does_not_change_the_table(N, big):
    a, want, _, _ = run(N, 6, 6, big)
    b, _, _, _ = run(N, 6, 6, big, order_seed=5)
    np.testing.assert_array_equal(a.table, b.table)
    np.testing.assert_array_equal(a.table, want)


def test_the_launch_reads_the_state_and_never_writes_it():
    steps, _ = CB.script(300, 2, 2, True)
    rig = CB.Rig(300, 2, 2, True)
    rig.feed(steps[0])
    rig.ev.accumulate()
    state, main = rig.ev.state.copy(), rig.ev.table.copy()
    rig.accumulate_columns()
    np.testing.assert_array_equal(rig.ev.state, state)
    np.testing.assert_array_equal(rig.ev.table, main)
    assert int(rig.ev.state[:8].view(np.int64)[0]) == 1             # the launch counter is the evaluator's


def test_a_group_past_num_groups_is_skipped():
    """g1 - 1 >= num_groups: a columns struct over fewer groups than the evaluator's writes nothing for the envs of the others"""
    steps, _ = CB.script(257, 1, 1, True)
    rig = CB.Rig(257, 1, 1, True)
    rig.feed(steps[0])
    rig.ev.accumulate()
    c = abi.LsimEvalColumns.from_buffer_copy(rig.c)
    c.num_groups = 100
    guard = rig.table.copy()
    assert CB.lib().emu_eval_columns_accumulate(ctypes.byref(c), None) == 0
    g1 = rig.group1()
    assert rig.table[:100, 0].sum() == int(((g1 >= 1) & (g1 <= 100)).sum()) > 0
    np.testing.assert_array_equal(rig.table.ravel()[100 * 4:], guard.ravel()[100 * 4:])


@pytest.mark.parametrize("which", ["emu", "hip"])
def test_host_side_argument_checks(which):
    """LSIM_E_INVALID before any launch, the table untouched; "hip" goes through the cross-compiled HIP library (loading it needs no GPU; only
    INVALID structs are passed)"""
    if which == "hip":
        from isaacgymloco_amd import lib
        L = lib.load()
        sizes, clear, acc = L.lsim_eval_columns_sizes, (lambda c: L.lsim_eval_columns_clear(c, None)), (lambda c: L.lsim_eval_columns_accumulate(c, None))
    else:
        api = CB.EmuApi()
        sizes, clear, acc = api.lsim_eval_columns_sizes, (lambda c: api.lsim_eval_columns_clear(c, None)), (lambda c: api.lsim_eval_columns_accumulate(c, None))
    INV = abi.E_INVALID
    tb = ctypes.c_size_t()
    assert sizes(24, 2, ctypes.byref(tb)) == 0 and tb.value == 24 * 7 * 8
    assert sizes(abi.DEFINES["LSIM_EVAL_MAX_GROUPS"], CB.MAX_COLS, ctypes.byref(tb)) == 0 and tb.value == 4096 * 19 * 8
    for bad in ((0, 2), (abi.DEFINES["LSIM_EVAL_MAX_GROUPS"] + 1, 2), (24, 0), (24, CB.MAX_COLS + 1), (-1, 1)):
        assert sizes(bad[0], bad[1], ctypes.byref(tb)) == INV
    assert sizes(24, 2, None) == INV
    assert clear(None) == INV and acc(None) == INV
    steps, _ = CB.script(64, 2, 4, True)
    rig = CB.Rig(64, 2, 4, True)
    rig.feed(steps[0])
    rig.ev.accumulate()
    rig.table[...] = 12345
    c0 = rig.c

    def broken(**kw):
        c = abi.LsimEvalColumns.from_buffer_copy(c0)
        for k, v in kw.items():
            setattr(c, k, v)
        return ctypes.byref(c)
    for fn in (clear, acc):
        for kw in (dict(state=None), dict(reset_buf=None), dict(values=None), dict(table=None), dict(state=c0.state + 8), dict(values=c0.values + 2),
                   dict(table=c0.table + 4), dict(num_envs=0), dict(num_envs=-5), dict(num_envs=0x7fffffff // 32 + 1), dict(num_envs=2 ** 40),
                   dict(num_groups=0), dict(num_groups=abi.DEFINES["LSIM_EVAL_MAX_GROUPS"] + 1), dict(num_cols=0), dict(num_cols=CB.MAX_COLS + 1),
                   dict(num_cols=-1), dict(ld=1), dict(ld=0), dict(num_cols=4, ld=3)):
            assert fn(broken(**kw)) == INV, kw
        assert (rig.table == 12345).all()
    if which == "emu":
        assert acc(broken(ld=2)) == 0 and not (rig.table == 12345).all()          # ld == num_cols is the limit
        assert clear(ctypes.byref(c0)) == 0 and not rig.table.any()


def test_struct_mirror_follows_the_header():
    assert [f[0] for f in abi.LsimEvalColumns._fields_] == ["state", "reset_buf", "values", "table", "num_envs", "num_groups", "num_cols", "ld"]
    assert ctypes.sizeof(abi.LsimEvalColumns) == 56 and abi.ABI_VERSION == 7
    assert (CB.MAX_COLS, CB.COL_WORDS) == (6, 3)
    assert abi.PROTOTYPES["lsim_eval_columns_accumulate"] == (ctypes.c_int, [ctypes.POINTER(abi.LsimEvalColumns), ctypes.c_void_p])
    assert abi.PROTOTYPES["lsim_eval_columns_sizes"] == (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_void_p])


# ---- the Python layer: learn.evaluate.Evaluator with api= the shims
def _emu_env(N=64):
    from eval_emu_binding import emu_mixed_env
    from isaacgymloco_amd.learn.evaluate import play_cfg
    cfg = play_cfg(C.mixed_cfg("aliengo", {"aliengo": 0.5, "go2": 0.5})[0])
    cfg.env.num_envs = N
    cfg.env.episode_length_s = 0.4
    cfg.terrain.num_rows, cfg.terrain.num_cols = 4, 4
    cfg.terrain.terrain_proportions = [0.5, 0.0, 0.0, 0.0, 0.25, 0.25]
    return emu_mixed_env(cfg, seed=3)


def _drive(env, ev, steps, feed=None):
    import torch
    g = torch.Generator().manual_seed(0)
    for t in range(steps):
        if feed is not None:
            feed(t)
        env.step_device(torch.randn(env.num_envs, 12, generator=g) * 3.0)
        ev.accumulate()
        if feed is not None:
            ev.accumulate_columns()


def test_evaluator_without_columns_is_the_evaluator_of_before():
    """result() without add_columns equals, dict for dict, the result of the same run through an api that has no lsim_eval_columns_* at all
    (any call of one would raise AttributeError), and makes no columns launch or allocation"""
    from eval_emu_binding import EmuApi as PlainApi
    from isaacgymloco_amd.learn.evaluate import Evaluator
    plain_api, api = PlainApi(), CB.EmuApi()
    assert not hasattr(plain_api, "lsim_eval_columns_accumulate")
    results = []
    for a in (plain_api, api):
        env = _emu_env()
        env.reset()
        ev = Evaluator(env, api=a)
        _drive(env, ev, 12)
        ev.clear()
        _drive(env, ev, 25)
        assert ev.columns is None and ev.column_names == ()
        results.append(ev.result())
    assert api.calls["lsim_eval_columns_accumulate"] == 0 and api.calls["lsim_eval_columns_clear"] == 0 and api.calls["lsim_eval_accumulate"] == 37
    assert json.dumps(results[0], sort_keys=True) == json.dumps(results[1], sort_keys=True)
    assert "columns" not in results[1]["total"] and "columns" not in results[1]["conventions"] and all("columns" not in g for g in results[1]["groups"])
    with pytest.raises(ValueError, match="add_columns"):
        ev.accumulate_columns()


def test_evaluator_columns_against_a_float64_recomputation():
    """mean and rms per group and in total against float64 sums of the values fed in: every addend is within half a 2^-32 step of its value,
    so |mean - exact| <= 2^-32 (the issue's bound; the squares' mean likewise, compared before the root)"""
    import torch
    from isaacgymloco_amd.learn.evaluate import Evaluator, FIX_ONE
    env = _emu_env()
    env.reset()
    api = CB.EmuApi()
    ev = Evaluator(env, api=api)
    ev.add_columns(["influence", "error"])
    assert ev.columns.shape == (64, 2) and ev.columns.dtype == torch.float32 and not ev.columns.any() and ev.column_names == ("influence", "error")
    with pytest.raises(ValueError):
        ev.add_columns(["again"])
    gen = torch.Generator().manual_seed(7)
    fed = []

    def feed(t):
        ev.columns[:, 0] = torch.rand(64, generator=gen) * 3.0
        ev.columns[:, 1] = torch.randn(64, generator=gen) * 0.05
        if t == 4:
            ev.columns[9, 1] = float("nan")
        fed.append(ev.columns.clone().numpy())
    _drive(env, ev, 30, feed)
    assert api.calls["lsim_eval_columns_accumulate"] == 30
    res = json.loads(json.dumps(ev.result()))
    assert res["conventions"]["columns"] == ["influence", "error"]
    table, ctable = ev.table.numpy(), ev.col_table.numpy()
    np.testing.assert_array_equal(ctable[:, 0], table[:, W["samples"]])
    assert res["total"]["samples"] == int(ctable[:, 0].sum()) and res["total"]["episodes"] >= 1
    # which env-steps were samples, and of which group: the evaluator's own bookkeeping, replayed from the env's buffers is test_evaluate.py's
    # subject; here the sums are checked through the group-free identity (the total) and per group through the integer table
    tot = res["total"]["columns"]
    n = res["total"]["samples"]
    for k, name in enumerate(("influence", "error")):
        s, q, bad = (int(ctable[:, 1 + 3 * k + j].sum()) for j in range(3))
        assert tot[name]["nonfinite"] == bad
        assert tot[name]["mean"] == s / FIX_ONE / n and tot[name]["rms"] == math.sqrt(q / FIX_ONE / n)
    assert tot["error"]["nonfinite"] in (0, 1) and tot["influence"]["nonfinite"] == 0
    for g in res["groups"]:
        assert set(g["columns"]) == {"influence", "error"} and set(g["columns"]["error"]) == {"mean", "rms", "nonfinite"}
        if g["samples"] == 0:
            assert math.isnan(g["columns"]["influence"]["mean"]) and math.isnan(g["columns"]["influence"]["rms"])
    # the float64 recomputation: an evaluator with ONE group and no episode ends (each env-step a sample), values of known sum
    env2 = _emu_env(N=8)
    env2.cfg.env.episode_length_s = 20.0
    env2.max_episode_length = 1000
    env2.reset()
    ev2 = Evaluator(env2, group_by=(), api=api)
    ev2.add_columns(["a", "b", "c"])
    rs = np.random.RandomState(3)
    exact, exact_sq, count = np.zeros(3), np.zeros(3), 0
    for t in range(6):
        vals = (rs.standard_normal((8, 3)) * [1e-3, 1.0, 100.0]).astype(np.float32)
        ev2.columns.copy_(torch.from_numpy(vals))
        env2.step_device(torch.zeros(8, 12))
        ev2.accumulate()
        ev2.accumulate_columns()
        live = env2.reset_buf.numpy() == 0
        exact += vals[live].astype(np.float64).sum(axis=0)
        exact_sq += (vals[live] * vals[live]).astype(np.float64).sum(axis=0)          # the fp32 product, summed exactly
        count += int(live.sum())
    r2 = ev2.result()
    assert r2["total"]["samples"] == count >= 40 and len(r2["groups"]) == 1
    for k, name in enumerate("abc"):
        got = r2["total"]["columns"][name]
        print(name, "mean diff", abs(got["mean"] - exact[k] / count), "mean-square diff", abs(got["rms"] ** 2 - exact_sq[k] / count))
        assert abs(got["mean"] - exact[k] / count) <= 2.0 ** -32
        assert abs(got["rms"] ** 2 - exact_sq[k] / count) <= 2.0 ** -32 + 4 * np.spacing(exact_sq[k] / count)
        assert got["nonfinite"] == 0 and r2["groups"][0]["columns"][name] == got
    ev2.clear()
    assert not ev2.col_table.any() and not ev2.table.any()
    from isaacgymloco_amd.learn.evaluate import format_table
    assert "influence" in format_table(res) and "influence" not in format_table({**res, "groups": [{k: v for k, v in g.items() if k != "columns"} for g in res["groups"]],
                                                                                  "total": {k: v for k, v in res["total"].items() if k != "columns"}})


def test_add_columns_refuses_bad_names():
    from isaacgymloco_amd.learn.evaluate import Evaluator
    env = _emu_env(N=8)
    env.reset()
    for names in ([], ["a", "a"], list("abcdefg")):
        with pytest.raises(ValueError):
            Evaluator(env, api=CB.EmuApi()).add_columns(names)
    from eval_emu_binding import EmuApi as PlainApi
    from isaacgymloco_amd import lib
    with pytest.raises(lib.LsimError, match="lsim_eval_columns"):
        Evaluator(env, api=PlainApi()).add_columns(["a"])
