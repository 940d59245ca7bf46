"""CPU: the statements, plan restatements, case tables, twins and bounds of tests/amp_update_reference.py (the discriminator-update column kernels, the
running moments and the pair rows), and the refusals of those entries through the HIP library on host pointers (they answer before any HIP call, so
no device is needed; only refused calls are made)."""
import ctypes

import numpy as np
import pytest

import amp_update_reference as R


# ---- column kernels ----------------------------------------------------------------------------------------------------------------------------
def test_colk_cases_reach_every_class():
    where = {cls: [] for cls in R.COLK_CLASSES}
    for name, c in R.COLK_CASES.items():
        got = R.colk_classes(c)
        assert got <= R.COLK_CLASSES
        for cls in got:
            where[cls].append(name)
    for cls in sorted(where):
        print(cls, where[cls][:4])
        assert where[cls], "no case reaches " + cls
    assert {c["n"] for c in R.COLK_CASES.values() if not R.colk_plan(c["batch"], c["n"])["floor"]} == {4, 64, 1024}
    assert all(c["batch"] * max(c["ld"], c["ldv"], c["ldm"]) * 4 <= 40e6 for c in R.COLK_CASES.values())


def test_colk_plan_against_the_library():
    """lsim_relu_cols_workspace is host code: the restated byte count for every case, the update's shapes and the refused widths"""
    from isaacgymloco_amd import abi, lib
    L = lib.load()
    shapes = [(c["batch"], c["n"]) for c in R.COLK_CASES.values()] + [(102400, 512), (20000, 1024), (20000, 256), (5, 12), (5, 20), (5, 1028), (5, 2048), (5, 30), (0, 32), (-3, 32), (5, 0)]
    for batch, n in shapes:
        need = ctypes.c_size_t(0)
        rc = L.lsim_relu_cols_workspace(batch, n, ctypes.byref(need))
        p = R.colk_plan(batch, n)
        if p is None:
            assert rc == abi.E_UNSUPPORTED, (batch, n, rc)
        else:
            assert (rc, need.value) == (0, p["bytes"]), ("the launch plan changed: re-derive the batches of tests/amp_update_reference.py", batch, n, rc, need.value, p)
    assert L.lsim_relu_cols_workspace(5, 32, None) == abi.E_INVALID
    p = R.colk_plan(102400, 512)
    assert (p["rl"], p["rps"], p["slices"]) == (2, 100, 1024)


@pytest.mark.parametrize("name", [n for n, c in R.COLK_CASES.items() if c["batch"] <= 5000])
def test_colk_kernel_order_twin_is_exact_on_exact_scenes(name):
    """on the integer scenes the twin that adds in the kernel's own order (and the reduce kernel's) equals the fp64 statement: the restated ownership of
    rows -- row lane, slice, reduce group -- counts every row once; and the NaN the scene puts under a non-positive mask never reaches a sum"""
    c = R.COLK_CASES[name]
    a, gd, w3 = R.head_scene(c, True)
    ref = R.head_reference(a, gd, w3)
    assert ((a == 0) & np.signbit(a)).any() and ((a == 0) & ~np.signbit(a)).any()
    for vals, want in zip(R.head_addends(a, gd, ref), (ref["db2"], ref["dhead"][:c["n"]], ref["dhead"][c["n"]:c["n"] + 1])):
        assert float(np.abs(want).max()) < 2 ** 24
        for tw in R.colsum_twins(vals, c).values():
            assert np.array_equal(tw.astype(np.float64), want), name
    v, m = R.colsum_scene(c, True)
    assert np.isnan(v[~(m > 0)]).all() and not np.isnan(v[m > 0]).any()
    want = R.colsum_reference(v, m)
    for tw in R.colsum_twins(np.where(m > 0, v, np.float32(0)), c).values():
        assert np.array_equal(tw.astype(np.float64), want), name
    # a kernel that counted -0.0 or +0.0 as unmasked, or multiplied instead of selecting, would differ
    assert not np.array_equal(np.where(m >= 0, np.nan_to_num(v, nan=7.0), 0).sum(0), want) or c["batch"] * c["n"] <= 4


def test_colk_general_tolerances():
    for name in ("n4-b1025", "n64-b65", "n1024-b4097", "n256-b17"):
        c = R.COLK_CASES[name]
        a, gd, w3 = R.head_scene(c, False)
        ref = R.head_reference(a, gd, w3)
        for vals, want, out in zip(R.head_addends(a, gd, ref), (ref["db2"], ref["dhead"][:c["n"]], ref["dhead"][c["n"]:c["n"] + 1]), ("grad_bias", "d head_weight", "d head_bias")):
            tol, dist = R.twin_tolerance(vals, want, c)
            print(name, out, "twin distance", dist, "tolerance", tol, "scale", float(np.abs(want).max()))
            assert tol <= 1e-5 * max(1.0, float(np.abs(want).max()))


# ---- running moments ---------------------------------------------------------------------------------------------------------------------------
def test_mom_plan_table():
    got = {b: (R.mom_plan(b)["rps"], R.mom_plan(b)["slices"]) for b in R.MOM_BATCHES}
    assert got == {1: (16, 1), 3: (16, 1), 15: (16, 1), 16: (16, 1), 17: (16, 2), 4096: (16, 256), 4097: (20, 205), 70001: (276, 254)}
    assert {c["start"] for c in R.MOM_CASES.values()} == set(R.MOM_STARTS) and {c["dim"] for c in R.MOM_CASES.values()} == set(R.MOM_DIMS)
    assert any(c["ldx"] > c["dim"] for c in R.MOM_CASES.values())
    for dim in R.MOM_DIMS:
        kinds = set()
        for c in R.MOM_CASES.values():
            if c["dim"] == dim:
                kinds |= set(R.mom_scene(c)[2])
        assert kinds == set(R.COLUMN_KINDS) or dim == 1, dim
    assert {k for c in R.MOM_CASES.values() if c["dim"] == 1 for k in R.mom_scene(c)[2]} >= {"o1", "const0.1", "const1234.567"}


@pytest.mark.parametrize("name", list(R.MOM_CASES))
def test_mom_float64_twin_stays_inside_the_derived_bound(name):
    """three updates in a row: the float64 twin in the kernel's order stays within the derived bound of the longdouble reference, on every column; the
    count is exact.  On a constant column the one-pass batch variance is rounding noise of either sign -- inside the bound, which at 0.1 and 1234.567 is
    below the Normalizer's epsilon (var + epsilon > 0) and at 98 765.43 is not: the merged variance is clamped at 0"""
    c = R.MOM_CASES[name]
    xs, state, kinds = R.mom_scene(c)
    ref, tw, err, count = state, state, None, state[2][0]
    for i, x in enumerate(xs):
        count = count + float(c["batch"])                  # float64, as the device adds it
        ref, err = R.mom_reference(x, ref, err)
        tw, bvar = R.mom_twin(x, tw)
        dm, dv = np.abs(tw[0] - ref[0].astype(np.float64)), np.abs(tw[1] - ref[1].astype(np.float64))
        print(name, "update", i, "mean: twin distance", dm.max(), "bound", err[0].max(), "| var: twin distance", dv.max(), "bound", err[1].max(),
              "| largest distance / bound", max((dm / err[0]).max(), (dv / err[1]).max()))
        assert (dm <= err[0]).all() and (dv <= err[1]).all(), name
        assert tw[2][0] == count and abs(float(ref[2][0]) - count) <= 2 * R.U * count
        assert (tw[1] >= 0).all()
        for j, k in enumerate(kinds):
            if k in R.CONSTANTS:
                if i == 0 and c["start"] == "count0":
                    assert float(ref[1][j]) == 0.0 and abs(bvar[j]) <= err[1][j], (name, k)
                if k != "const98765.43":
                    assert err[1][j] < R.NORMALIZER_EPS and bvar[j] + R.NORMALIZER_EPS > 0, (name, k)


def test_mom_constant_column_noise_can_exceed_epsilon():
    """why lsim_k_moments_merge clamps: on a column constant at 98 765.43 the derived bound of the one-pass variance (2e-4 .. 5e-4) exceeds the
    Normalizer's epsilon of 1e-4, so var + epsilon > 0 is not guaranteed there; the float64 emulation in the kernel's order gives batch variances of
    either sign, down to -9.5e-6 (a tenth of epsilon) at the row counts tried here.  With the clamp the merged variance is never negative"""
    worst = 0.0
    for batch in (4096, 4097, 70001, 5000, 12345, 33333):
        x = np.full((batch, 1), 98765.43, dtype=np.float32)
        (_, var, _), bvar = R.mom_twin(x, (np.zeros(1), np.ones(1), np.zeros(1)))
        _, err = R.mom_reference(x, (np.zeros(1), np.ones(1), np.zeros(1)))
        print("constant 98765.43,", batch, "rows: emulated one-pass batch variance", bvar[0], "bound", err[1][0])
        assert abs(bvar[0]) <= err[1][0] and var[0] >= 0
        worst = min(worst, bvar[0])
    x = np.full((4097, 1), 98765.43, dtype=np.float32)
    assert R.mom_reference(x, (np.zeros(1), np.ones(1), np.zeros(1)))[1][1][0] > R.NORMALIZER_EPS
    print("most negative emulated batch variance", worst)


# ---- pair rows -----------------------------------------------------------------------------------------------------------------------------------
def test_pair_cases():
    trips = {n: R.pair_blocks(c["batch"], c["dim"]) for n, c in R.PAIR_CASES.items()}
    assert trips["d64-b65600"] == (8192, 5) and all(b < 8192 and t <= 4 for n, (b, t) in trips.items() if n != "d64-b65600")
    assert 65600 * 2 * 64 > 8192 * 1024
    for name, c in R.PAIR_CASES.items():
        s, ns, mean, var = R.pair_scene(c)
        out = R.pair_twin(s, ns, mean, var)
        assert out[0, 0] == R.PAIR_CLIP and out[0, c["dim"]] == -R.PAIR_CLIP and np.abs(out).max() <= R.PAIR_CLIP
        if c["batch"] >= 5:
            assert out[0, 0] == 10.0 and 9.99999 < out[1, 0] < 10.0 and out[2, 0] == 10.0 and out[3, 0] == -10.0 and -10.0 < out[4, 0] < -9.99999
        if c["dim"] >= 30 and c["batch"] >= 1025:
            assert not np.array_equal(out, R.pair_twin(s, ns, mean, var, sum_in_float32=True)), "the rounding of var + eps does not show in this scene"


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------
def _host():
    keep = []

    def address(floats):
        a = np.full(floats + 8, np.nan, dtype=np.float32)
        keep.append(a)
        return a.ctypes.data + (-a.ctypes.data % 16)

    return keep, address


def test_column_entries_refuse_on_host_pointers():
    from isaacgymloco_amd import abi, lib
    L = lib.load()
    for name, entry, edits, code in R.COLK_REFUSALS:
        keep, address = _host()
        rc = R.colk_refusal_call(L, entry, edits, address)
        assert rc == getattr(abi, code), (name, entry, rc)
        assert all(np.isnan(a).all() for a in keep), name


def test_moments_and_pair_rows_refuse_on_host_pointers():
    from isaacgymloco_amd import abi, lib
    L = lib.load()
    keep, address = _host()
    x, mean, var, count, ws, out = (address(4096) for _ in range(6))
    need = ctypes.c_size_t(0)
    assert L.lsim_running_moments_workspace(ctypes.byref(need)) == 0 and need.value == R.MOM_SLICES * 2 * R.MOM_MAX_DIM * 8
    big = address(need.value // 4)
    assert L.lsim_running_moments_update(x, 65, 5, 65, mean, var, count, big, need.value, None) == abi.E_UNSUPPORTED
    for args in ((None, 8, 5, 8, mean, var, count, big, need.value), (x, 8, 5, 8, None, var, count, big, need.value), (x, 8, 5, 8, mean, None, count, big, need.value),
                 (x, 8, 5, 8, mean, var, None, big, need.value), (x, 8, 5, 8, mean, var, count, None, need.value), (x, 7, 5, 8, mean, var, count, big, need.value),
                 (x, 8, 0, 8, mean, var, count, big, need.value), (x, 8, 5, 0, mean, var, count, big, need.value), (x, 8, 5, 8, mean, var, count, big, need.value - 1),
                 (x, 8, 5, 8, mean, var, count, big + 4, need.value)):
        assert L.lsim_running_moments_update(*args, None) == abi.E_INVALID, args
    dm, dv = ctypes.cast(mean, ctypes.c_void_p), ctypes.cast(var, ctypes.c_void_p)
    for args in ((x, 8, x, 8, dm, None, 1e-4, 10.0, 5, 8, out, 16), (x, 8, x, 8, None, dv, 1e-4, 10.0, 5, 8, out, 16), (None, 8, x, 8, dm, dv, 1e-4, 10.0, 5, 8, out, 16),
                 (x, 8, None, 8, dm, dv, 1e-4, 10.0, 5, 8, out, 16), (x, 8, x, 8, dm, dv, 1e-4, 10.0, 5, 8, None, 16), (x, 7, x, 8, dm, dv, 1e-4, 10.0, 5, 8, out, 16),
                 (x, 8, x, 7, dm, dv, 1e-4, 10.0, 5, 8, out, 16), (x, 8, x, 8, dm, dv, 1e-4, 10.0, 5, 8, out, 15), (x, 8, x, 8, dm, dv, 1e-4, 10.0, 0, 8, out, 16),
                 (x, 8, x, 8, dm, dv, 1e-4, 10.0, 5, 0, out, 16)):
        assert L.lsim_amp_pair_rows(*args, None) == abi.E_INVALID, args
    assert all(np.isnan(a).all() for a in keep)
