"""The odometry launch (lsim_odometry_step, isaacgymloco_amd/csrc/ls_odometry.h) on the CPU: the kernel's own per-env code, compiled by g++
(tests/emu/emu_odometry.cpp), through the scenarios of tests/odometry_scenes.py against the numpy reference written from the header's
comment (tests/odometry_reference.py, which derives the bound of the general scene and names the five mutants the scene must catch)."""
import ctypes

import numpy as np

import odometry_emu_binding as OB
import odometry_reference as OR
import odometry_scenes as OS
from helpers import ROOT, abi


def test_header_declares_the_launch_additively():
    assert abi.RNG_TAGS["odometry"] == 18 and abi.ABI_VERSION == 7
    od = OB.LsimOdometry
    assert abi.PROTOTYPES["lsim_odometry_step"] == (ctypes.c_int, [ctypes.POINTER(od), ctypes.c_void_p])
    assert [f for f, _ in od._fields_][-6:] == list(OR.RANGE_NAMES)
    doc = open(ROOT + "/INTEGRATION.md").read()
    assert "lsim_odometry_step" in doc and "lsim_map_rows" in doc


def test_zero_ranges_leave_the_pose_bit_for_bit():
    OS.zero_ranges(OB.Rig)


def test_second_launch_on_the_same_tick_changes_nothing():
    OS.same_tick_again(OB.Rig)


def test_fresh_env_resets_only_and_fill_all():
    OS.fresh_env(OB.Rig)
    OS.fresh_env(OB.Rig, tick=0)


def test_env_stride_leaves_the_rows_in_between():
    OS.strided(OB.Rig)


def test_nan_pose_and_the_step_after():
    OS.nan_pose(OB.Rig)


def test_general_scene_within_the_derived_bound_and_mutants_fail():
    """N = 5, K = 40, all six ranges non-zero, a reset in the middle.  The bound is OR.bounds, derived in the docstring of
    tests/odometry_reference.py from the operation count: u (a K L_max (1 + R) + b |p|_inf) with a = 13 (dx, dy), 6 (dz), one more for est,
    b = 1; the reference's own fp32 twin must stay below half of it, and each of the five mutants must leave it."""
    got = OS.general(OB.Rig)
    odo, est = got[-1]
    assert (np.abs(odo[:, 0:3]) > 1e-5).all() and (np.abs(odo[:, 0:3]) < 2 * OS.L_MAX).all()
    OS.general(OB.Rig, N=7, K=12, env_stride=3, tick0=OS.BIG_TICK)


def test_draws_depend_on_tick_stream_seed_and_rank():
    rs = OS.walk(3, 1)

    def run(tick=4, **kw):
        rig = OS.start(OB.Rig, rs[0], tick=tick, **kw)
        return rig.read()[0][:, 4:7]
    base = run()
    np.testing.assert_array_equal(OS.bits(run(tick=4 + 2 ** 32)), OS.bits(base))
    for other in (run(tick=5), run(stream_id=4), run(seed=8), run(rank=3)):
        assert (OS.bits(other) != OS.bits(base)).all()
    assert len({r.tobytes() for r in base}) == 3


def test_refusals_through_the_shim_and_through_the_library():
    OS.refusals(OB.Rig, lambda: OB.lib().emu_odometry_step(None, None))
    from isaacgymloco_amd import lib
    L = lib.load()             # loading needs no GPU; a refused launch never reaches one
    OS.refusals(lambda *a, **kw: _host_rig_on_the_library(L, *a, **kw), lambda: L.lsim_odometry_step(None, None), launches=False)


def _host_rig_on_the_library(L, *a, **kw):
    rig = OB.Rig(*a, **kw)
    rig._entry = L.lsim_odometry_step
    return rig
