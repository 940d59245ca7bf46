"""lsim_elevation_map_cleanup on the CPU: the shim tests/emu/emu_elevation_cleanup.cpp (the kernel's own per-lane functions) against the
float64 reference written from include/lsim.h (elevation_cleanup_reference: the bracket, where its margins come from, the mutants) on the
scenes of elevation_cleanup_scenes."""
import ctypes

import numpy as np
import pytest

import elevation_cleanup_reference as CR
import elevation_cleanup_scenes as CS
import elevation_map_reference as ER
import elevation_map_scenes as EMS
from helpers import abi

F = np.float32
make_rig = CR.cleanup_rig()


@pytest.mark.parametrize("G", [16, 64])
@pytest.mark.parametrize("scene", sorted(CS.EXACT))
def test_dyadic_scene(scene, G):
    CS.EXACT[scene](make_rig, G=G)


def test_dyadic_scene_with_the_rays_reversed_is_bit_equal():
    a, b = CS.planted_block(make_rig), CS.planted_block(make_rig, reverse=True)
    for k in ("stamp", "cleared", "height", "cell"):
        np.testing.assert_array_equal(ER.bits(a[k]), ER.bits(b[k]))


@pytest.mark.parametrize("flags,stagger,env_stride", [(0, 0, 1), (0, 1, 1), (0, 1, 2), (ER.FILL_ALL, 0, 1), (ER.RESETS_ONLY, 1, 3)])
def test_due_sets(flags, stagger, env_stride):
    out = CS.due_sets(make_rig, flags, stagger, env_stride)
    if flags:
        assert all((o["stamp"] >= 0).all() for o in out), "FILL_ALL and RESETS_ONLY forget nothing"


@pytest.mark.parametrize("mutant", CR.MUTANTS)
def test_the_scenes_catch_the_mutant(mutant):
    with pytest.raises(AssertionError):
        CS.CATCHES[mutant](make_rig, mutant=mutant)


@pytest.mark.parametrize("shape", [(1, 64, 1), (3, 16, 193), (3, 64, 513), (257, 16, 193)])
@pytest.mark.parametrize("var", [False, True])
def test_general_poses_inside_the_bracket(shape, var):
    """CR.check asserts what is never written (height, cell, var, scan, known and their padding, bit for bit), that envs that are not
    worked on keep every stamp, and the bracket; the rig's read() asserts every guard"""
    after, share, gone, fresh = CS.general(make_rig, *shape, var=var)
    if shape[2] >= 193:
        assert gone.sum() > 0, "the scene has phantoms the rays cross"
    if fresh is not None:
        assert gone[fresh] == 0 and after["cleared"][fresh] == 0, "that env starts an episode"


def test_general_poses_with_the_rays_reversed_are_bit_equal():
    a = CS.general(make_rig, 3, 64, 513, var=True)[0]
    b = CS.general(make_rig, 3, 64, 513, var=True, reverse=True)[0]
    for k in ("stamp", "cleared"):
        np.testing.assert_array_equal(a[k], b[k])


def test_refusals():
    rig = CS.start(make_rig, 2, np.array([CS.DOWN, CS.DOWN], F), var=True)
    for e in range(2):
        CS.plant(rig, e, {(2, 0): 0.25})
    before = rig.read()
    assert CR.lib().emu_elevation_map_cleanup(None, None) == abi.E_INVALID

    def refused(edit=None, edit_cleanup=None):
        assert rig.launch(5, 0, edit=edit, edit_cleanup=edit_cleanup) == abi.E_INVALID, (edit, edit_cleanup)

    def setter(name, value):
        return lambda s: setattr(s, name, value)
    for name in ("root_states", "assumed_mount", "dirs", "depth", "pts", "height", "stamp", "cell", "scan", "known", "episode_length", "state"):
        refused(setter(name, None))
    for name in ("root_states", "height", "stamp", "cell", "scan", "episode_length", "state"):
        refused(lambda s, name=name: setattr(s, name, getattr(s, name) + 2))
    for name, bad in (("size", 8), ("size", 48), ("res", 0.0), ("res", float("nan")), ("a", float("inf")), ("unknown_drop", float("nan")), ("t_lo", -1.0),
                      ("t_hi", 0.0), ("num_points", 0), ("num_rays", 0), ("depth_stride", 1), ("scan_stride", 0), ("known_stride", 0), ("period", 0),
                      ("stagger", 2), ("env_stride", 0), ("num_envs", 0)):
        refused(setter(name, bad))
    assert rig.launch(-1, 0) == abi.E_INVALID and rig.launch(5, 4) == abi.E_INVALID and rig.launch(5, ER.FILL_ALL | ER.RESETS_ONLY) == abi.E_INVALID
    refused(edit_cleanup=setter("cleared", None))
    refused(edit_cleanup=lambda s: setattr(s, "cleared", s.cleared + 2))
    refused(edit_cleanup=lambda s: setattr(s, "var", s.var + 1))
    for name in ("clear_margin", "clear_slope", "clear_sigma", "end_gap"):
        for bad in (-2.0 ** -10, float("nan"), float("inf")):
            refused(edit_cleanup=setter(name, bad))
    for bad in (0, -1):
        refused(edit_cleanup=setter("min_rays", bad))
    after = rig.read()
    for k in before:
        np.testing.assert_array_equal(ER.bits(np.asarray(after[k])) if k != "state" else after[k], ER.bits(np.asarray(before[k])) if k != "state" else before[k])
    assert rig.launch(5, 0, edit_cleanup=setter("var", None)) == 0, "var is optional"


def test_the_point_routine_is_the_maps_own_bit_for_bit():
    """ls_ec_point at the ray's own range against ls_em_point on the non-dyadic poses of elevation_map_scenes.random_poses' rig: wherever
    the map keeps the ray, the same z bits and the slot of the same (x, y)"""
    N, G = 5, 16
    rig = EMS.random_rig(make_rig, N, G, 16, 12, 0)
    s = type(rig.struct).from_buffer_copy(rig.struct)
    rinv = F(1.0 / float(F(s.em.res)))
    kept_n = 0
    xyz, kept, slot, z = (ctypes.c_float * 3)(), ctypes.c_int(), ctypes.c_int(), ctypes.c_float()
    for e in range(N):
        for r in range(rig.R):
            rv = CR.lib().emu_elevation_cleanup_point(ctypes.addressof(s), e, r, xyz, ctypes.byref(kept), ctypes.byref(slot), ctypes.byref(z))
            assert rv in (0, 1)
            if not kept.value:
                continue
            assert rv == 0, "a ray the map keeps passes the range and label tests"
            kept_n += 1
            assert F(xyz[2]).view(np.uint32) == F(z.value).view(np.uint32), (e, r)
            ix, iy = int(np.floor(F(xyz[0]) * rinv)), int(np.floor(F(xyz[1]) * rinv))
            assert (ix & (G - 1)) * G + (iy & (G - 1)) == slot.value, (e, r)
    assert kept_n > 0.5 * N * rig.R


def _plane_depths(rig, slope):
    """the stored z-depth of every ray's meeting with the plane z = slope * x, in float64, 1e9 where it has none ahead"""
    rs, mt = rig.get("root_states").astype(np.float64), rig.get("mount").astype(np.float64)
    dirs, inv = rig.get("dirs").astype(np.float64), rig.get("inv_scale").astype(np.float64)
    d = ER.rot(rs[:, None, 3:7], ER.rot(mt[:, None, 3:7], dirs[None]))
    o = rs[:, None, :3] + ER.rot(rs[:, None, 3:7], mt[:, None, :3])
    with np.errstate(all="ignore"):
        den = d[..., 2] - slope * d[..., 0]
        t = np.where(den < -1e-3, (slope * o[..., 0] - o[..., 2]) / den, 1e9)
    return np.where((t > 0) & (t < 1e8), t / inv[None], 1e9).astype(F)


@pytest.mark.parametrize("slope", [0.0, 0.25])
def test_a_true_surface_is_never_forgotten(slope):
    """the static invariant: clean depths of a plane, the true pose, the default option (margin 0.05, slope 0.05, min_rays 2, end_gap 1.5
    cells, a plain map) -- over 20 captures of a moving, rolling and pitching pose the clean-up forgets nothing"""
    res = 0.0625
    assert CR.DEFAULTS["clear_margin"] > np.sqrt(2.0) * res * 0.25, "the header's condition on the margin, for the steeper plane"
    dirs, inv_scale = EMS.camera_dirs(32, 24)
    pts = np.array([[0.0, 0.0], [0.5, 0.0]], F)
    N, G = 2, 32
    rig = CR.CleanupRig(N, G, dirs, pts, res=res, inv_scale=inv_scale, t_lo=0.05, t_hi=4.9, cleanup=dict(CR.DEFAULTS, end_gap=1.5 * res))
    h = np.radians(50.0) / 2.0
    rig.put("mount", np.broadcast_to(np.array([0.3, 0.0, 0.05, 0.0, np.sin(h), 0.0, np.cos(h)], F), (N, 7)))
    rig.put("cleared", 0)
    g = np.random.RandomState(3)
    inserted = 0
    for k in range(20):
        rs = rig.get("root_states")
        for e in range(N):
            x, y = 0.3 + 0.07 * k * (1 - 2 * e), -0.2 + 0.031 * k
            roll, pitch, yaw = g.uniform(-0.1, 0.1), g.uniform(-0.1, 0.1), 0.02 * k * (1 - 2 * e)
            cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
            rs[e, :3] = (x, y, slope * x + 0.4)
            rs[e, 3:7] = (sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy)
        rig.put("root_states", rs)
        rig.put("depth", _plane_depths(rig, slope))
        before = rig.read()
        assert rig.launch(10 + k, 0) == 0
        after = rig.read()
        np.testing.assert_array_equal(after["stamp"], before["stamp"], err_msg=f"capture {k}: a cell of the true surface was forgotten")
        assert (after["cleared"] == 0).all()
        assert rig.map_launch(10 + k, 0) == 0
        inserted = int((rig.read()["stamp"] >= 0).sum())
    assert inserted > 200, "the captures do fill the map"
