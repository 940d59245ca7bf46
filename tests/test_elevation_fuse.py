"""lsim_elevation_map_fused and lsim_map_rows_fused on the CPU: the shim tests/emu/emu_elevation_fuse.cpp (the kernel's own per-lane
functions) against the numpy reference written from include/lsim.h (elevation_fuse_reference: what is exact, the bound, the mutants)."""
import ctypes

import numpy as np
import pytest

import elevation_fuse_reference as FR
import elevation_fuse_scenes as FS
import elevation_map_emu_binding as EB
import elevation_map_reference as ER
import elevation_map_scenes as ES
import emu_binding
from helpers import abi

F = np.float32
INVALID = abi.E_INVALID - (1 << 32) if abi.E_INVALID > 0x7FFFFFFF else abi.E_INVALID
IDENTITY = {"band": 0.0, "gate2": 0.0}


def test_the_header_declares_both_entry_points():
    ef, mf = abi.LsimElevationMapFused, abi.LsimMapRowsFused
    assert abi.PROTOTYPES["lsim_elevation_map_fused"] == (ctypes.c_int, [ctypes.POINTER(ef), ctypes.c_void_p])
    assert abi.PROTOTYPES["lsim_map_rows_fused"] == (ctypes.c_int, [ctypes.POINTER(mf), ctypes.c_void_p])
    assert ef.em.offset == 0 and ef.em.size == ctypes.sizeof(abi.LsimElevationMap) and mf.mr.offset == 0
    assert [n for n, _ in ef._fields_][1:] == ["var", "scan_var", "sigma0", "sigma2", "range_z2", "band", "var_floor", "var_growth", "var_max", "gate2",
                                               "count_cap", "var_stride"]


@pytest.mark.parametrize("name", sorted(FS.SCENES))
def test_scene_within_the_bound_and_independent_of_ray_order(name):
    worst, fwd, ref = FS.run(FR.fused_rig(), name)
    print(f"{name}: worst miss {worst:.3f} of the bound")
    assert worst <= 1.0
    _, rev, _ = FS.run(FR.fused_rig(), name, reverse=True)
    for a, b in zip(fwd, rev):
        for k in ("height", "var", "stamp", "cell", "scan", "scan_var", "known"):
            np.testing.assert_array_equal(ER.bits(a[k]), ER.bits(b[k]), err_msg=f"{name}: {k} depends on the order of the rays")
    assert np.isfinite(fwd[-1]["scan_var"]).all() and np.isfinite(fwd[-1]["scan"]).all()


def test_scenes_cover_what_they_are_named_for():
    _, reads, ref = FS.run(FR.fused_rig(), "counts")
    counts = sorted(n for _, n in ref.sums.values())
    assert counts == [1, 1, 1, 2, 2, 2, 5, 5, 5], "count_cap = 4 reached in one cell and not in the others"
    _, reads, ref = FS.run(FR.fused_rig(), "spread")
    assert sorted(n for _, n in ref.sums.values())[-1] == 3, "two of the five points of cell A lie below the band"
    _, reads, ref = FS.run(FR.fused_rig(), "clamps")
    v = np.concatenate([r["var"][r["stamp"] >= 0] for r in reads])
    assert (v == F(3e-5)).any() and (v == F(2.5e-5)).any(), "the variance meets both clamps"
    _, reads, ref = FS.run(FR.fused_rig(), "steps")
    assert any(ref.fused.values()), "the last capture of the steps scene fuses"
    _, reads, ref = FS.run(FR.fused_rig(), "gate_edge")
    assert not any(ref.fused.values()), "d^2 == gate2 S: the strict gate stays shut"
    _, reads, ref = FS.run(FR.fused_rig(), "lifecycle")
    assert (reads[-1]["stamp"][1:3] == -1).all() and (reads[-1]["var"][1:3] == F(333.0)).all(), "envs that are not visited keep their arrays"
    assert (reads[4]["stamp"][0][reads[4]["stamp"][0] >= 0] == 4).all(), "a new episode holds its first capture only"
    assert (reads[5]["stamp"][3] == 5).any() and not (reads[5]["stamp"][0] == 5).any(), "RESETS_ONLY inserts the reset env only"


@pytest.mark.parametrize("mutant", FR.MUTANTS)
def test_every_mutant_misses_the_bound_by_more_than_ten(mutant):
    worst, _, _ = FS.run(FR.fused_rig(), FS.CATCHES[mutant], mutant=mutant)
    print(f"{mutant} on {FS.CATCHES[mutant]}: {worst:.3g} times the bound")
    assert worst > 10.0


PLAIN_SCENES = [("exact_basic", {}), ("exact_basic", {"reverse": True}), ("window_edges", {}), ("negative_coordinates", {}), ("scrolling", {}),
                ("due_sets", {}), ("due_sets", {"flags": ER.RESETS_ONLY}), ("due_sets", {"stagger": 1, "env_stride": 3}), ("invalid_rays", {}),
                ("nonfinite_pose", {}), ("scan_frame", {}), ("big_ticks", {})]


@pytest.mark.parametrize("scene, kw", PLAIN_SCENES, ids=[f"{s}-{'-'.join(map(str, k.values()))}" for s, k in PLAIN_SCENES])
def test_band_zero_gate_zero_is_the_plain_map_bit_for_bit(scene, kw):
    """every scene of elevation_map_scenes through the fused launch: each compares with the plain map's reference bit for bit itself, and
    what it returns equals what the plain shim returns"""
    plain = getattr(ES, scene)(EB.Rig, **kw)
    fused = getattr(ES, scene)(FR.fused_rig(IDENTITY), **kw)
    plain, fused = (plain if isinstance(plain, list) else [plain]), (fused if isinstance(fused, list) else [fused])
    for a, b in zip(plain, fused):
        for k in ("height", "stamp", "cell", "scan", "known"):
            np.testing.assert_array_equal(ER.bits(a[k]), ER.bits(b[k]), err_msg=k)
        assert np.isfinite(b["scan_var"][b["known"] != 0]).all()


@pytest.mark.parametrize("seed", (0, 1))
def test_identity_on_general_poses(seed):
    """a pitched camera over bumpy ground, any roll, pitch and yaw, one env 190 m out: the fused launch with band = 0, gate2 = 0 passes the
    plain map's own comparison rule and writes the plain shim's bits"""
    plain, share = ES.random_poses(EB.Rig, seed=seed)
    fused, _ = ES.random_poses(FR.fused_rig(IDENTITY), seed=seed)
    print(f"ambiguous share of the scene: {share:.4f}")
    for k in ("height", "stamp", "cell", "scan", "known"):
        np.testing.assert_array_equal(ER.bits(plain[k]), ER.bits(fused[k]), err_msg=k)
    kn = fused["stamp"] >= 0
    assert (fused["var"][kn] >= F(2.5e-5)).all() and (fused["var"][kn] <= F(0.25)).all() and np.isfinite(fused["scan_var"][:, :]).all()


@pytest.mark.parametrize("kw", [dict(seed=0), dict(seed=1), dict(seed=2, N=3, G=64, width=193, height=1, labels=True), dict(seed=3, N=4, G=16, width=64, height=8, env_stride=3),
                                dict(FR.DENSE, fusion=FR.DENSE_FUSION)], ids=str)
def test_general_poses_with_a_band_inside_the_references_bracket(kw):
    """the banded mean, the count and vm on non-dyadic points against the float64 reference's extremes over the ambiguous choices
    (elevation_fuse_reference.check_fused_bracket); the ambiguous share, from the reference alone, is printed and at most 1 %"""
    kw = dict(kw)
    fusion = kw.pop("fusion", None)
    got, share = FR.general_poses(FR.fused_rig(fusion), fusion=fusion, **kw)
    print(f"{kw}: ambiguous share {share:.4%}, {int((got['stamp'] >= 0).sum())} cells")
    assert (got["stamp"] >= 0).sum() >= 3


@pytest.mark.parametrize("wrong", [{"band": 0.5}, {"band": 0.003}, {"band": 0.012}, {"band": 0.0}, {"band": 0.006, "count_cap": 1}], ids=str)
def test_the_bracket_rejects_a_launch_with_another_band_or_cap(wrong):
    """the dense scene (64 x 48 rays, a band of 6 mm that cuts through most cells): a launch that averages everything, takes the maximum,
    uses half or twice the band or another cap leaves the reference's bracket -- the rule has teeth where the band matters"""
    with pytest.raises(AssertionError):
        FR.general_poses(FR.fused_rig(wrong), fusion=FR.DENSE_FUSION, **FR.DENSE)


def _rig():
    rig = FR.FusedRig(2, 16, FS.DIRS, FS.PTS, res=FS.RES)
    rig.put("depth", 0.5)
    return rig


BAD = [("var", 0), ("scan_var", 0), ("var", "odd"), ("scan_var", "odd"), ("var_stride", 4)] + \
      [(k, v) for k in FR.FIELDS for v in (-1e-3, float("nan"), float("inf"))] + [("band", 0.500001), ("var_floor", 0.3), ("count_cap", 0), ("count_cap", -2)]


@pytest.mark.parametrize("field, value", BAD, ids=[f"{f}-{v}" for f, v in BAD])
def test_refusals_of_the_fused_launch(field, value):
    rig = _rig()
    before = rig.read()

    def edit(ef):
        setattr(ef, field, (getattr(ef, field) or 0) + 2 if value == "odd" else value)
    assert rig.launch(1, 0, edit_fused=edit) == INVALID
    after = rig.read()
    for k in ("height", "stamp", "cell", "scan", "known", "var", "scan_var"):
        np.testing.assert_array_equal(ER.bits(before[k]), ER.bits(after[k]), err_msg=f"a refused launch wrote {k}")
    assert rig.launch(1, 0) == 0


@pytest.mark.parametrize("field, value", [("size", 48), ("res", 0.0), ("height", 0), ("tick", -1), ("period", 0), ("num_points", 0), ("scan_stride", 2),
                                          ("flags", 3), ("flags", 4), ("env_stride", 0), ("t_hi", 0.0)])
def test_the_fused_launch_refuses_what_the_plain_one_refuses(field, value):
    rig = _rig()
    assert rig.launch(1, 0, edit=lambda em: setattr(em, field, value)) == INVALID
    assert lib_null() == INVALID


def lib_null():
    return FR.lib().emu_elevation_map_fused(None, None)


def test_the_library_refuses_on_the_host_too():
    """the HIP library's entry points check before any launch: refusals need no GPU"""
    from isaacgymloco_amd import lib
    L = lib.load()
    rig = _rig()
    rig._fused_entry = L.lsim_elevation_map_fused
    for field, value in (("var", 0), ("band", 0.6), ("gate2", float("nan")), ("count_cap", 0), ("var_stride", 1), ("var_floor", 1.0)):
        assert rig.launch(1, 0, edit_fused=lambda ef: setattr(ef, field, value)) == INVALID, field
    assert rig.launch(1, 0, edit=lambda em: setattr(em, "size", 8)) == INVALID
    assert L.lsim_elevation_map_fused(None, None) == INVALID and L.lsim_map_rows_fused(None, None) == INVALID
    mf = abi.LsimMapRowsFused()
    assert L.lsim_map_rows_fused(ctypes.byref(mf), None) == INVALID


# ---------------------------------------------------------------------------------------------------- map rows with a confidence
def _rows_case(N=5, P=7, stride=3, seed=0):
    g = np.random.RandomState(seed)
    al = emu_binding.aligned
    a = {"scan": al((N, P + 1), F), "known": al((N, P + 2), np.uint8), "pose": al((N, 13), F), "scan_var": al((N, P + 3), F), "rows": al((N * (2 * P + 2) + 16,), F)}
    a["scan"][:] = g.uniform(-0.5, 0.5, a["scan"].shape)
    a["known"][:] = g.randint(0, 2, a["known"].shape) * g.randint(1, 255, a["known"].shape)
    a["pose"][:] = g.uniform(0.2, 0.6, a["pose"].shape)
    a["scan_var"][:] = 10.0 ** g.uniform(-6, 0, a["scan_var"].shape)
    a["scan_var"][0, 0], a["scan_var"][0, 1], a["scan_var"][0, 2], a["scan_var"][0, 3] = np.nan, np.inf, -1.0, 0.0
    a["known"][0, :4] = 1
    a["scan"][1, 0], a["pose"][2, 2] = np.nan, np.inf
    a["rows"][:] = -9.5
    mf = abi.LsimMapRowsFused()
    mr = mf.mr
    mr.scan, mr.known, mr.pose, mr.rows = (a[k].ctypes.data for k in ("scan", "known", "pose", "rows"))
    mr.num_points, mr.channels, mr.scan_stride, mr.known_stride, mr.ld, mr.num_envs, mr.env_stride = P, 2, P + 1, P + 2, 2 * P + 2, N, stride
    mr.z_offset, mr.scale = 0.5, 5.0
    mf.scan_var, mf.var_stride, mf.var_ref = a["scan_var"].ctypes.data, P + 3, 4e-4
    return a, mf


def test_map_rows_fused_is_exact():
    N, P = 5, 7
    a, mf = _rows_case(N, P)
    assert FR.lib().emu_map_rows_fused(ctypes.byref(mf), None) == 0
    rows = a["rows"][:N * (2 * P + 2)].reshape(N, 2 * P + 2)
    want = FR.rows_fused(a["scan"][:, :P], a["known"][:, :P], a["pose"][:, 2], a["scan_var"][:, :P], 0.5, 5.0, 4e-4)
    for e in range(N):
        if e % 3 == 0:
            np.testing.assert_array_equal(ER.bits(rows[e, :2 * P]), ER.bits(want[e]))
        else:
            assert (rows[e] == F(-9.5)).all(), "rows of envs that are not visited are not touched"
    assert (rows[:, 2 * P:] == F(-9.5)).all() and (a["rows"][N * (2 * P + 2):] == F(-9.5)).all() and np.isfinite(rows).all()
    conf = rows[::3, P:2 * P]
    assert (conf >= 0).all() and (conf <= 1).all() and (conf[a["known"][::3, :P] == 0] == 0).all()
    assert list(rows[0, P:P + 4]) == [0.0, 0.0, 0.0, 1.0], "NaN, inf and a negative variance read as no confidence; variance 0 as 1"
    # one channel: lsim_map_rows's own block and nothing else
    a["rows"][:] = -9.5
    mf.mr.channels, mf.scan_var = 1, None
    assert FR.lib().emu_map_rows_fused(ctypes.byref(mf), None) == 0
    np.testing.assert_array_equal(ER.bits(rows[0, :P]), ER.bits(want[0, :P]))
    assert (rows[0, P:] == F(-9.5)).all()


@pytest.mark.parametrize("field, value", [("var_ref", 0.0), ("var_ref", -1.0), ("var_ref", float("nan")), ("var_ref", float("inf")), ("scan_var", 0),
                                          ("var_stride", 6), ("mr.scan", 0), ("mr.rows", 0), ("mr.known", 0), ("mr.channels", 3), ("mr.num_points", 0),
                                          ("mr.ld", 13), ("mr.scale", float("nan")), ("mr.num_envs", 0), ("mr.env_stride", 0), ("mr.known_stride", 6)])
def test_refusals_of_map_rows_fused(field, value):
    a, mf = _rows_case()
    obj = mf.mr if field.startswith("mr.") else mf
    setattr(obj, field.split(".")[-1], value)
    assert FR.lib().emu_map_rows_fused(ctypes.byref(mf), None) == INVALID
    assert (a["rows"] == F(-9.5)).all()
