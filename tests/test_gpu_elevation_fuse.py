"""GPU: lsim_elevation_map_fused and lsim_map_rows_fused (isaacgymloco_amd/csrc/ls_elevation_fuse.h) on a real device: the dyadic scenes
of tests/elevation_fuse_scenes.py against the numpy reference's bound and against the CPU build of the same source, the band = 0,
gate2 = 0 identity against the library's own lsim_elevation_map, and general poses against the CPU build.  Every GPU step is one launch
over at most 257 envs."""
import ctypes

import numpy as np
import pytest

import elevation_fuse_reference as FR
import elevation_fuse_scenes as FS
import elevation_map_emu_binding as EB
import elevation_map_reference as ER
import elevation_map_scenes as ES

pytestmark = pytest.mark.gpu
F = np.float32
IDENTITY = {"band": 0.0, "gate2": 0.0}
ALL = ("height", "var", "stamp", "cell", "scan", "scan_var", "known")
# (N, G, width, height, env_stride): R = 1 (one lane), 193 (a partial wave) and 513 (three trips of the lane loop)
SHAPES = [(1, 64, 1, 1, 1), (3, 16, 193, 1, 1), (3, 64, 513, 1, 1), (257, 16, 193, 1, 3), (257, 64, 513, 1, 1)]


def _lib():
    from isaacgymloco_amd import lib
    return lib.load()


def hip_fused(fusion=None):
    return FR.fused_rig(fusion, device="cuda:0", entry=_lib().lsim_elevation_map_fused)


def hip_plain(*a, **kw):
    return EB.Rig(*a, device="cuda:0", entry=_lib().lsim_elevation_map, **kw)


@pytest.mark.parametrize("G", [16, 64])
@pytest.mark.parametrize("name", sorted(FS.SCENES))
def test_dyadic_scenes_on_the_device(name, G):
    """inside the reference's bound, the integers exact; against the CPU build both lie within the same bound of the same float64 numbers"""
    worst, hip, ref = FS.run(hip_fused(), name, G=G)
    print(f"{name} G {G}: worst miss {worst:.3f} of the bound")
    assert worst <= 1.0
    _, emu, _ = FS.run(FR.fused_rig(), name, G=G)
    for a, b in zip(hip, emu):
        for k in ("stamp", "cell", "known"):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_side_stream_ray_order_and_repeated_launch():
    import torch
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        _, fwd, _ = FS.run(hip_fused(), "steps")
        _, rev, _ = FS.run(hip_fused(), "steps", reverse=True)
        _, again, _ = FS.run(hip_fused(), "steps")
    torch.cuda.synchronize()
    for a, b, c in zip(fwd, rev, again):
        for k in ALL:
            np.testing.assert_array_equal(ER.bits(a[k]), ER.bits(b[k]), err_msg=f"{k} depends on the order of the rays")
            np.testing.assert_array_equal(ER.bits(a[k]), ER.bits(c[k]), err_msg=f"{k} differs between two runs")


@pytest.mark.parametrize("scene", ["exact_basic", "window_edges", "negative_coordinates", "scrolling", "due_sets", "invalid_rays", "nonfinite_pose",
                                   "scan_frame", "big_ticks"])
def test_identity_against_the_librarys_plain_map_on_the_exact_scenes(scene):
    plain, fused = getattr(ES, scene)(hip_plain), getattr(ES, scene)(hip_fused(IDENTITY))
    plain, fused = (plain if isinstance(plain, list) else [plain]), (fused if isinstance(fused, list) else [fused])
    for a, b in zip(plain, fused):
        for k in ("height", "stamp", "cell", "scan", "known"):
            np.testing.assert_array_equal(ER.bits(a[k]), ER.bits(b[k]), err_msg=k)


@pytest.mark.parametrize("N,G,width,height,env_stride", SHAPES)
def test_general_poses_identity_and_the_references_bracket(N, G, width, height, env_stride):
    """band = 0, gate2 = 0: the plain map's own comparison rule (the reference's bracket, EPS) holds for the fused launch, and its arrays are
    the library's lsim_elevation_map's.  With the default fusion (band 0.0625 m): every cell's banded mean and variance lie between the
    float64 reference's extremes over the ambiguous choices (elevation_fuse_reference.check_fused_bracket), the ambiguous share at most 1 %"""
    kw = dict(N=N, G=G, width=width, height=height, seed=N + G + width, env_stride=env_stride, labels=width == 193)
    ident, _ = ES.random_poses(hip_fused(IDENTITY), **kw)
    plain, _ = ES.random_poses(hip_plain, **kw)
    for k in ("height", "stamp", "cell", "scan", "known"):
        np.testing.assert_array_equal(ER.bits(ident[k]), ER.bits(plain[k]), err_msg=k)
    hip, share = FR.general_poses(hip_fused(), **kw)
    print(f"fused map N {N} G {G} R {width * height}: {int((hip['stamp'] >= 0).sum())} cells inside the bracket; ambiguous share {share:.4%}")
    lo, hi = F(FR.DEFAULTS["var_floor"]), F(FR.DEFAULTS["var_max"])
    visited = slice(None, None, env_stride)
    assert np.isfinite(hip["scan_var"][visited]).all() and (hip["scan_var"][visited] >= lo).all() and (hip["scan_var"][visited] <= hi).all()


def test_the_dense_scene_where_the_band_cuts_through_cells():
    """R = 3072 (twelve trips of the lane loop), a band of 6 mm: the device inside the reference's bracket, and a launch with twice the band outside"""
    hip, share = FR.general_poses(hip_fused(FR.DENSE_FUSION), fusion=FR.DENSE_FUSION, **FR.DENSE)
    print(f"dense scene: {int((hip['stamp'] >= 0).sum())} cells inside the bracket; ambiguous share {share:.4%}")
    with pytest.raises(AssertionError):
        FR.general_poses(hip_fused({"band": 0.012}), fusion=FR.DENSE_FUSION, **FR.DENSE)


def test_refusals_on_device_memory():
    rig = hip_fused()(2, 16, FS.DIRS, FS.PTS, res=FS.RES)
    rig.put("depth", 0.5)
    before = rig.read()
    for field, value in (("var", 0), ("scan_var", 0), ("band", 0.6), ("gate2", float("nan")), ("count_cap", 0), ("var_stride", 1), ("var_floor", 1.0)):
        assert rig.launch(1, 0, edit_fused=lambda ef: setattr(ef, field, value)) != 0, field
    assert rig.launch(1, 0, edit=lambda em: setattr(em, "size", 8)) != 0
    after = rig.read()
    for k in ALL:
        np.testing.assert_array_equal(ER.bits(before[k]), ER.bits(after[k]), err_msg=f"a refused launch wrote {k}")
    assert rig.launch(1, 0) == 0


def test_map_rows_fused_on_the_device():
    import torch
    from helpers import abi
    g = np.random.RandomState(3)
    N, P = 257, 104
    scan, known = g.uniform(-0.5, 0.5, (N, P)).astype(F), (g.randint(0, 2, (N, P)) * 7).astype(np.uint8)
    pose, sv = g.uniform(0.2, 0.6, (N, 13)).astype(F), (10.0 ** g.uniform(-6, 0, (N, P))).astype(F)
    sv[0, :3], known[0, :3] = (np.nan, np.inf, -1.0), 1
    t = {k: torch.from_numpy(v).cuda() for k, v in (("scan", scan), ("known", known), ("pose", pose), ("sv", sv))}
    rows = torch.full((N, 2 * P + 3), -9.5, device="cuda")
    mf = abi.LsimMapRowsFused()
    mr = mf.mr
    mr.scan, mr.known, mr.pose, mr.rows = t["scan"].data_ptr(), t["known"].data_ptr(), t["pose"].data_ptr(), rows.data_ptr()
    mr.num_points, mr.channels, mr.scan_stride, mr.known_stride, mr.ld, mr.num_envs, mr.env_stride = P, 2, P, P, 2 * P + 3, N, 1
    mr.z_offset, mr.scale = 0.5, 5.0
    mf.scan_var, mf.var_stride, mf.var_ref = t["sv"].data_ptr(), P, 4e-4
    assert _lib().lsim_map_rows_fused(ctypes.byref(mf), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    got = rows.cpu().numpy()
    np.testing.assert_array_equal(ER.bits(got[:, :2 * P]), ER.bits(FR.rows_fused(scan, known, pose[:, 2], sv, 0.5, 5.0, 4e-4)))
    assert (got[:, 2 * P:] == F(-9.5)).all()
    mf.var_ref = 0.0
    assert _lib().lsim_map_rows_fused(ctypes.byref(mf), None) != 0
