"""CPU: the reference, plan restatement, case table, scenes and mutants of the weight-gradient shape tests (tests/wgrad_shapes_reference.py), and the
refusals of the weight-gradient entries through the HIP library on host pointers (they answer before any HIP call, so no device is needed; only
refused calls are made)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import wgrad_shapes_reference as R

NAMES = list(R.CASES)


# ---- coverage: a later edit of the cases cannot silently lose a path ---------------------------------------------------------------------
def test_cases_reach_every_class():
    """all 44 (NT, KT) of the single-wave kernel, all 24 <VX, VG, KG, FZ> of the tiled one, every tile kind under every vector class, every
    quarter and hand-over of loop3, every form of the reduce: from the restated plan alone"""
    assert len(R.sw_pairs()) == 44
    assert len({c for c in R.CLASSES if c.startswith("tiled<")}) == 24
    where = {cls: [] for cls in R.CLASSES}
    for name, c in R.CASES.items():
        got = R.case_classes(c)
        assert got <= R.CLASSES, sorted(got - R.CLASSES)
        for cls in got:
            where[cls].append(name)
    for cls in sorted(where):
        print(cls, where[cls][:4])
        assert where[cls], "no case reaches " + cls
    # what the update's own shape and batch reach: none of the short or ragged classes
    ship = R.case_classes(R._case("elu", 512, 256, 102400))
    assert not ship & {"quarter16", "quarter20", "wave_ragged", "waves_without_rows", "edge_k_vx2", "gy_scalar_store", "handover4", "handover8"}


def test_cases_stay_small_and_exact():
    for name, c in R.CASES.items():
        assert c["batch"] <= 17000 and (c["batch"] <= 11000 or R.plan(c["batch"], c["k_in"], c["n_out"])["small"]), name
        assert 9 * 4 * c["batch"] < 2 ** 24
        assert c["ldx"] > c["k_in"] and c["ldg"] > c["n_out"] and (not c["fz"] or c["ldz"] > c["n_out"]), name


def test_plan_restatement_against_the_library():
    """lsim_linear_wgrad_workspace is host code: the restated partial count and byte count for every case and for the update's shapes"""
    from isaacgymloco_amd import abi, lib
    L = lib.load()
    shapes = [(c["batch"], c["k_in"], c["n_out"]) for c in R.CASES.values()]
    shapes += [(102400, 512, 256), (102363, 238, 512), (20492, 60, 1024), (1, 1, 1), (5, 350, 400), (5, 351, 399), (7, 1, 140000), (0, 4, 4), (3, 128, 33), (9, 129, 16)]
    for batch, k_in, n_out in shapes:
        nbytes, parts = ctypes.c_size_t(0), ctypes.c_int(0)
        rc = L.lsim_linear_wgrad_workspace(batch, k_in, n_out, ctypes.byref(nbytes), ctypes.byref(parts))
        p = R.plan(batch, k_in, n_out)
        if p is None:
            assert rc == abi.E_UNSUPPORTED, (batch, k_in, n_out)
        else:
            assert (rc, parts.value, nbytes.value) == (0, p["partials"], p["bytes"]), \
                ("the plan changed: re-derive the batches of wgrad_shapes_reference.py", batch, k_in, n_out, rc, parts.value, nbytes.value, p)


def test_plan_table_of_the_quarters():
    """batch = slices * 4 q - 5 gives full slices of quarter q and a last slice of 75-123 rows"""
    for (k_in, n_out), slices in {(512, 256): 32, (238, 512): 32, (60, 1024): 32, (64, 512): 64, (130, 260): 51, (270, 128): 85, (700, 200): 21,
                                  (3, 1400): 23, (1, 4100): 7}.items():
        for q in (20, 24, 28, 32):
            batch = slices * 4 * q - 5
            p = R.plan(batch, k_in, n_out)
            assert (p["partials"], p["rows"]) == (slices, 4 * q), (k_in, n_out, q, p)
            rows = [b1 - b0 for _, b0, b1 in R.waves(p, batch)]
            assert rows[:4] == [q] * 4 and sum(rows) == batch and 75 <= sum(rows[-4:]) <= 123
    assert [R.loop3(r) for r in (19, 20, 24, 28, 31, 32, 44)] == [(0, 0), (1, 20), (1, 20), (1, 20), (1, 20), (2, 32), (3, 44)]


def test_waves_own_every_row_once_and_the_renumbering_is_a_bijection():
    for name, c in R.CASES.items():
        p = R.plan(c["batch"], c["k_in"], c["n_out"])
        own = np.zeros(c["batch"], dtype=np.int64)
        for _, b0, b1 in R.waves(p, c["batch"]):
            assert 0 <= b0 <= b1 <= c["batch"]
            own[b0:b1] += 1
        assert (own == 1).all(), name
        if not p["small"]:
            assert sorted(R.xcd_order(p["blocks"])) == list(range(p["blocks"])), name
    for total in list(range(1, 70)) + [510, 513, 2048]:
        assert sorted(R.xcd_order(total)) == list(range(total))


def test_vector_classes_of_the_layouts():
    for width in (1, 3, 60, 64, 130, 238, 262, 512):
        for code, want in (("2", 2), ("1", 1), ("1p", 1), ("0", 0), ("0p", 0)):
            off, ld = R.layout(code, width)
            assert ld > width and R.vec_class(off, ld) == want, (width, code)
        for code in ("0", "0p", "0h"):
            assert R.vec_class(*R.layout(code, width), pairs=False) == 0


# ---- the reference against torch in fp64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["plain", "elu", "relu"])
def test_reference_matches_torch_autograd_fp64(entry):
    import torch.nn.functional as F
    c = R._case(entry, 37, 150, 53)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(53, 37, generator=g, dtype=torch.float64)
    W = torch.randn(150, 37, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(150, generator=g, dtype=torch.float64, requires_grad=True)
    go = torch.randn(53, 150, generator=g, dtype=torch.float64)
    pre = F.linear(x, W, b)
    pre.retain_grad()
    out = {"plain": lambda t: t, "elu": F.elu, "relu": F.relu}[entry](pre)
    out.backward(go)
    z = None if entry == "plain" else out.detach().numpy()
    ref = R.reference(c, x.numpy(), go.numpy(), z)
    np.testing.assert_allclose(ref["dw"], W.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ref["db"], b.grad.numpy(), rtol=1e-12, atol=1e-12)
    if entry != "plain":
        np.testing.assert_allclose(R.grad_pre(c, go.numpy(), z), pre.grad.numpy(), rtol=1e-12, atol=1e-12)


# ---- exact scenes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_exact_scenes_are_exact(name):
    """multiples of 1/4 below 2^24: the fp64 sums are exactly representable in fp32, the row-by-row ownership sums equal them, and on a short case
    the fp32 twins of every summation order agree to the bit"""
    c = R.CASES[name]
    x, g, z = R.exact_scene(c)
    ref = R.reference(c, x, g, z)
    for k in ("dw", "db"):
        assert np.array_equal(ref[k] * 4, np.round(ref[k] * 4)) and np.abs(ref[k]).max() * 4 < 2 ** 24
        assert np.array_equal(ref[k].astype(np.float32).astype(np.float64), ref[k])
    assert np.abs(ref["dw"]).max() > 0
    st = R.structured(c, x, g, z)
    assert np.array_equal(st["dw"], ref["dw"]) and np.array_equal(st["db"], ref["db"])
    if c["fz"]:
        assert np.array_equal(ref["gy"].astype(np.float64), R.grad_pre(c, g, z)), "the fp32 factor is exact on an exact scene"
        if c["batch"] >= 8:
            assert (z == 0).any() and (z > 0).any(), "both sides of the boundary"
            assert (np.signbit(z) & (z == 0)).any() == (c["entry"] == "elu")
    if c["batch"] <= 200:
        gy = ref["gy"] if c["fz"] else g
        for order in (range(c["batch"]), range(c["batch"] - 1, -1, -1)):
            acc = np.zeros((c["n_out"], c["k_in"]), dtype=np.float32)
            for b in order:
                acc += gy[b][:, None] * x[b][None, :]
            assert np.array_equal(acc.astype(np.float64), ref["dw"])


def test_padded_buffers_hold_nan_everywhere_else():
    c = R.CASES[NAMES[0]]
    a = np.arange(12, dtype=np.float32).reshape(4, 3)
    flat = R.padded(a, 3, 5)
    assert flat.size == 3 + (4 + R.EXTRA_ROWS) * 5 and np.isnan(flat).sum() == flat.size - 12
    assert all(flat[3 + 5 * b + j] == a[b, j] for b in range(4) for j in range(3))


# ---- general scenes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.GENERAL)
def test_general_scenes_have_a_nonzero_twin_distance(name):
    sc = R.general_case(name)
    assert sc["twin_dist"][0] > 0 and sc["twin_dist"][1] > 0, sc["twin_dist"]
    assert sc["tol"][0] < 1e-4 * np.abs(sc["ref"]["dw"]).max() and sc["tol"][1] < 1e-4 * np.abs(sc["ref"]["db"]).max()
    c = R.CASES[name]
    if c["fz"]:
        assert (sc["z"] > 0).any() and (sc["z"] <= 0).any()


def test_general_cases_cover_the_families():
    got = [R.CASES[n] for n in R.GENERAL]
    plans = [R.plan(c["batch"], c["k_in"], c["n_out"]) for c in got]
    assert {p["small"] for p in plans} == {True, False} and {p["kg"] for p in plans} == {0, 1, 2}
    assert {c["entry"] for c in got} == {"plain", "elu", "relu"}
    assert any(c["n_out"] % 4 for c in got if c["gy"]) and any(c["k_in"] < 4 for c in got)


# ---- mutants ---------------------------------------------------------------------------------------------------------------------------
def _differs(a, b):
    return any(not np.array_equal(a[k], b[k]) for k in ("dw", "db")) or (a["gy"] is not None and not np.array_equal(a["gy"], b["gy"]))


@functools.lru_cache(maxsize=None)
def _mutant_table():
    """{mutant: [(case, differs)]} over the exact scenes: each scene and its unmutated sums are formed once"""
    table = {m: [] for m in R.MUTANTS}
    for name, c in R.CASES.items():
        todo = [m for m in R.MUTANTS if R.mutant_touches(m, c)]
        if not todo:
            continue
        x, g, z = R.exact_scene(c)
        good = R.structured(c, x, g, z)
        for m in todo:
            bad = R.structured(c, x, g, z, mutant=m)
            if m == "gy_from_kb1":
                assert bad["gy_stores"] > good["gy_stores"] == 1, "the mutant is there, and no value shows it"
            table[m].append((name, _differs(good, bad)))
    return table


@pytest.mark.parametrize("mutant", list(R.MUTANTS))
def test_mutants_are_seen(mutant):
    """every exact scene a mutant can touch gives another dw, db or grad_pre; the two mutants that cannot change a value by construction are
    asserted to change none, and R.MUTANTS says why no check can see them"""
    rows = _mutant_table()[mutant]
    touched = [name for name, _ in rows]
    print(mutant, len(touched), "scenes:", touched[:6])
    assert touched
    for name, differs in rows:
        assert differs == (R.MUTANTS[mutant] == "values"), (mutant, name)
    if mutant in ("handover_skipped", "handover_twice"):
        for cls in ("handover4", "handover8"):
            assert any(cls in R.case_classes(R.CASES[n]) for n in touched), cls


def test_mutants_miss_the_general_tolerance():
    """the value mutants against the twins' tolerance of a general scene they touch: far outside"""
    for mutant, sees in R.MUTANTS.items():
        if sees != "values":
            continue
        names = [n for n in R.GENERAL if R.mutant_touches(mutant, R.CASES[n])]
        assert names, mutant
        c = R.CASES[names[0]]
        sc = R.general_case(names[0])
        bad = R.structured(c, sc["x"], sc["g"], sc["z"], mutant=mutant)
        miss = max(np.abs(bad["dw"] - sc["ref"]["dw"]).max() / sc["tol"][0], np.abs(bad["db"] - sc["ref"]["db"]).max() / sc["tol"][1])
        print(mutant, names[0], "misses the tolerance by", miss)
        assert miss > 10.0, (mutant, names[0], miss)


# ---- refusals through the HIP library, on host pointers -----------------------------------------------------------------------------------
class _Host:
    def __init__(self):
        self.keep = []

    def address(self, floats):
        a = np.full(floats + 4, np.nan, dtype=np.float32)
        self.keep.append(a)
        return a.ctypes.data + (-a.ctypes.data) % 16

    def untouched(self):
        return all(np.isnan(a).all() for a in self.keep)


@pytest.mark.parametrize("name,entry,edits,code", R.REFUSALS, ids=[r[0] for r in R.REFUSALS])
def test_entries_refuse_on_the_host(name, entry, edits, code):
    from isaacgymloco_amd import abi, lib
    L = lib.load()
    for deferred in (None, abi.LsimWgradPending()):
        h = _Host()
        rc = R.refusal_call(L, entry, edits, h.address, deferred)
        assert rc == getattr(abi, code), (name, rc)
        assert h.untouched()
        if deferred is not None:
            assert not deferred.part and not deferred.out and deferred.num_partials == 0, "a refused call leaves the record alone"


def test_deferred_entries_refuse_a_null_record_and_the_batched_sum_refuses_bad_items():
    from isaacgymloco_amd import abi, lib
    L = lib.load()
    h = _Host()
    for entry in R.ENTRY:
        s = R.REFUSAL_SHAPE
        p = R.plan(s["batch"], s["k_in"], s["n_out"])
        a = [h.address(6 * 68), 68, h.address(6 * 84), 84] + ([h.address(6 * 84), 84] if entry != "plain" else []) + [s["batch"], s["k_in"], s["n_out"], h.address(5120), h.address(80)]
        a += ([h.address(400)] if entry != "plain" else []) + [h.address(p["bytes"] // 4), p["bytes"], None]
        assert getattr(L, R.ENTRY[entry] + "_deferred")(*a, None) == abi.E_INVALID, entry
    part, out = h.address(64), h.address(16)
    def item(**kw):
        it = abi.LsimWgradPending()
        it.part, it.out, it.num_partials, it.count = part, out, 4, 16
        for k, v in kw.items():
            setattr(it, k, v)
        return it
    arr = lambda *items: (abi.LsimWgradPending * len(items))(*items)
    assert L.lsim_wgrad_reduce_batch(arr(item()), -1, None) == abi.E_INVALID
    assert L.lsim_wgrad_reduce_batch(None, 1, None) == abi.E_INVALID
    assert L.lsim_wgrad_reduce_batch(arr(item(), item(part=None)), 2, None) == abi.E_INVALID
    assert L.lsim_wgrad_reduce_batch(arr(item(out=None)), 1, None) == abi.E_INVALID
    assert L.lsim_wgrad_reduce_batch(arr(item(count2=4)), 1, None) == abi.E_INVALID                      # count2 > 0 without part2
    assert L.lsim_wgrad_reduce_batch(arr(item(count2=4, part2=part)), 1, None) == abi.E_INVALID          # ... or without out2
    assert L.lsim_wgrad_reduce_batch(arr(item(num_partials=0)), 1, None) == abi.E_INVALID
    assert L.lsim_wgrad_reduce_batch(arr(item(count=0)), 1, None) == abi.E_INVALID
    assert h.untouched()
