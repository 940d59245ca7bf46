"""CPU: the reference, plan restatement, case table, scenes, ELU bound and mutants of the forward-GEMM shape tests (tests/fwd_gemm_reference.py), and the
refusals of lsim_linear_elu_forward / lsim_linear_masked_forward through the HIP library on host pointers (they answer before any HIP call, so no device
is needed; only refused calls are made)."""
import math

import numpy as np
import pytest

import fwd_gemm_reference as R

CUS = (64, 256, 304)


# ---- coverage ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cus", CUS)
def test_cases_reach_every_class(cus):
    """the table is built from the plan for the device's CU count: on 64, 256 and 304 CUs it reaches every source class of the operand loads under
    both tile configs and both epilogues, every k_in, n_out and batch of the lists, every tile count and every kind of persistent walk"""
    want = R.classes()
    where = {cls: [] for cls in want}
    for name, c in R.cases(cus).items():
        for cls in R.case_classes(c, cus) & want:
            where[cls].append(name)
    for cls in sorted(where):
        print(cus, cls, where[cls][:3])
        assert where[cls], "no case reaches %s at %d CUs" % (cls, cus)
    assert "total:1/wide" not in want          # more than 128 features are at least two feature tiles


@pytest.mark.parametrize("cus", CUS)
def test_cases_stay_small(cus):
    for name, c in R.cases(cus).items():
        p = R.case_plan(c, cus)
        assert c["ldx"] > c["k_in"], name
        assert c["batch"] * (c["ldx"] + c["ldo"] + c["ldm"]) * 4 < 90e6, name
        if p["total"] >= 8 * 8:
            assert c["k_in"] <= 40, name


def test_plan_of_the_update_shapes():
    """the restated plan on the shapes the learner runs, by hand: 102 400 x 512 -> 256 is 640 x 2 wide tiles on 512 blocks, 2 or 3 tiles per block"""
    p = R.plan(102400, 512, 256, 512, 0, 0, 256)
    assert (p["config"], p["n_tiles"], p["m_tiles"], p["total"], p["blocks"], p["per_xcd"], p["stride"], p["chunks"], p["launched"]) == ("wide", 2, 640, 1280, 512, 160, 64, 16, 2)
    assert sorted({len(w) for w in p["walks"]}) == [2, 3]
    p = R.plan(20000, 60, 1024, 60, 0, 0, 256)
    assert (p["total"], p["launched"], p["source"]) == (125 * 8, 2, (2, 2))
    p = R.plan(1, 3, 4, 3, 0, 0, 256)
    assert (p["blocks"], p["total"], p["launched"]) == (8, 1, 0) and [len(w) for w in p["walks"]] == [1, 0, 0, 0, 0, 0, 0, 0]
    assert R.plan(5, 8, 6, 8, 0, 0, 256) is None and R.plan(0, 8, 8, 8, 0, 0, 256) is None
    # the demotions
    assert R.plan(5, 8, 8, 8, 0, 2, 256)["launched"] == 1 and R.plan(5, 8, 8, 10, 0, 0, 256)["launched"] == 1 and R.plan(5, 8, 8, 8, 1, 0, 256)["launched"] == 0
    assert R.plan(5, 8, 8, 8, 0, 1, 256)["launched"] == 0 and R.plan(5, 6, 8, 6, 0, 0, 256)["launched"] == 1 and R.plan(5, 7, 8, 8, 0, 0, 256)["launched"] == 0


def test_elu_bound_derivation():
    """three terms: one ulp of the hardware 2^y at results <= 1, the rounding of x * log2(e) (and of the constant) scaled by sup |x| e^x, half an ulp for
    the subtraction.  1.17e-7, not the 2e-7 the header used to state; emulated in numpy with a correctly rounded exp2 the error stays inside it"""
    assert 1.16e-7 < R.ELU_BOUND < 1.17e-7
    assert R.elu_exp_bound(0.5) < R.ELU_BOUND and R.elu_exp_bound(50.0) == R.ELU_BOUND
    assert abs(R.LOG2E_F32_RELERR - 1.335e-8) < 1e-10
    x = -np.concatenate([np.linspace(0, 2, 20001), np.linspace(2, 40, 20001), 2.0 ** -np.arange(1, 40.0)]).astype(np.float32)
    y = (x * np.float32(math.log2(math.e))).astype(np.float32)
    got = (np.exp2(y.astype(np.float64)).astype(np.float32) - np.float32(1)).astype(np.float64)       # a 1/2-ulp exp2: inside the 1-ulp term
    err = np.abs(got - np.expm1(x.astype(np.float64)))
    print("emulated __expf(x) - 1: largest error", err.max(), "bound", R.ELU_BOUND)
    assert err.max() <= R.ELU_BOUND
    assert (got[x <= -30] == -1.0).all() and got[0] == 0.0


# ---- the reference against itself --------------------------------------------------------------------------------------------------------------
NAMES = list(R.cases(256))


@pytest.mark.parametrize("name", NAMES)
def test_structured_equals_the_statement_and_mutants_are_seen(name):
    """the output formed block by block from the restated walks equals the fp64 statement (every tile stored once, the columns between n_out and ldo
    untouched), the exact scene holds what the GPU test relies on, and every mutant that reaches the case moves its expected output by more than the
    case's tolerance (0 for the mask and for positive pre-activations, the exponential's bound for the others); the one mutant that cannot change a
    value changes none"""
    cus = 256
    c = R.cases(cus)[name]
    sc = R.exact_scene(c)
    ref = R.reference(c, *sc)
    want = R.expected_flat(c, ref["out"])
    assert not R.differs(R.structured(c, cus, *sc), want, 0.0), name
    assert (ref["pre"] == 0).any(), "no pre-activation of exactly 0"
    if c["act"] == "elu":
        assert (ref["pre"] <= -30).any() and (ref["pre"] > 0).any()
        tol = R.ELU_BOUND
    else:
        m = sc[3]
        neg0 = (m == 0) & np.signbit(m)
        assert ((m == 0) & ~np.signbit(m)).any() and neg0.any() and (m == np.finfo(np.float32).tiny).any() and (m < 0).any()
        assert ref["pre"][0, 0] != 0 and m[0, 0] == 0
        tol = 0.0
    seen = []
    for mutant, kind in R.MUTANTS.items():
        if not R.mutant_touches(mutant, c, cus):
            continue
        changed = R.differs(R.structured(c, cus, *sc, mutant=mutant), want, tol)
        if kind.startswith("nothing"):
            assert not changed, (name, mutant)
        else:
            assert changed, (name, mutant, "not seen")
            seen.append(mutant)
    print(name, "seen:", ", ".join(seen))
    assert seen, name


def test_every_mutant_reaches_some_case():
    for cus in CUS:
        for mutant in R.MUTANTS:
            assert any(R.mutant_touches(mutant, c, cus) for c in R.cases(cus).values()), (mutant, cus)


@pytest.mark.parametrize("name", R.GENERAL)
def test_general_tolerance_is_tight_and_separates_the_mutants(name):
    """the twins' tolerance on the general scenes: a few 1e-7 to 1e-6 for O(1) outputs, and the value mutants are outside it"""
    c = R.cases(256)[name]
    g = R.general_case(name)
    print(name, "twin distance", g["twin_dist"], "tolerance", g["base"], "scale", g["scale"])
    assert g["base"] <= 64 * 2.0 ** -23 * max(g["scale"], 1.0) * max(1.0, math.sqrt(c["k_in"] / 16.0)), (name, g["base"])
    want = R.expected_flat(c, g["ref"]["out"])
    tol = float(g["tol"].max())
    for mutant in ("half_chunk_dropped", "mask_ge_0", "elu_on_positives", "xcd_last_tile_dropped", "bias_at_n_minus_n0"):
        if R.mutant_touches(mutant, c, 256):
            assert R.differs(R.structured(c, 256, *g["scene"], mutant=mutant), want, tol), (name, mutant)


# ---- refusals: host checks, before any HIP call ------------------------------------------------------------------------------------------------
def test_entries_refuse_on_host_pointers():
    from isaacgymloco_amd import abi, lib
    L = lib.load()
    for name, entry, edits, code in R.REFUSALS:
        keep = []

        def address(floats):
            a = np.full(floats + 8, np.nan, dtype=np.float32)
            off = (-a.ctypes.data % 16) // 4
            keep.append(a)
            return a.ctypes.data + 4 * off

        rc = R.refusal_call(L, entry, edits, address)
        assert rc == getattr(abi, code), (name, entry, rc)
        assert all(np.isnan(a).all() for a in keep), name
