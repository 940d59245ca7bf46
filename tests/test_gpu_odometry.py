"""GPU: the odometry launch (lsim_odometry_step, isaacgymloco_amd/csrc/ls_odometry.h) on a real device: the scenarios of
tests/odometry_scenes.py against the numpy reference (tests/odometry_reference.py derives the bound), against the CPU build of the same
source, on a side stream, and the refusals on device memory.  Every GPU step is one launch over at most 257 envs."""
import numpy as np
import pytest

import odometry_emu_binding as OB
import odometry_reference as OR
import odometry_scenes as OS

pytestmark = pytest.mark.gpu


def hip_rig(*a, **kw):
    from isaacgymloco_amd import lib
    return OB.Rig(*a, device="cuda:0", entry=lib.load().lsim_odometry_step, **kw)


@pytest.mark.parametrize("N", [1, 3, 257])
def test_the_exact_scenes_on_the_device(N):
    """all-zero ranges, and a fresh env's row: exact against the reference on either build, so the two builds agree in them bit for bit"""
    OS.zero_ranges(hip_rig, N=N, K=10 if N == 3 else 4)
    if N >= 3:
        OS.fresh_env(hip_rig, N=N)


@pytest.mark.parametrize("N,K,env_stride", [(1, 6, 1), (5, 40, 1), (257, 6, 1), (257, 6, 3)])
def test_the_general_scene_on_the_device_and_against_the_cpu_build(N, K, env_stride):
    """each of the two fp32 evaluations lies within OR.bounds of the float64 reference: at most two bounds apart"""
    hip = OS.general(hip_rig, N=N, K=K, env_stride=env_stride, tick0=OS.BIG_TICK)
    emu = OS.general(OB.Rig, N=N, K=K, env_stride=env_stride, tick0=OS.BIG_TICK)
    rs = OS.walk(N, K, reset=(K // 2, env_stride if N > env_stride else 0))
    worst = 0.0
    for t in range(K + 1):
        for h, e, tol in zip(hip[t], emu[t], OR.bounds(max(t, 1), OS.L_MAX, OS.RANGES, rs[t])):
            d = np.abs(h.astype(np.float64) - e)
            assert (d <= 2.0 * tol).all()
            worst = max(worst, float((d[tol > 0] / tol[tol > 0]).max()))
    print(f"odometry N {N} K {K} stride {env_stride}: hip vs emu largest distance {worst:.3f} of the reference's bound")


def test_a_scene_on_a_side_stream():
    import torch
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        OS.general(hip_rig, N=257, K=4, stream=side.cuda_stream)
        OS.same_tick_again(hip_rig)
    torch.cuda.synchronize()


def test_same_tick_stride_guards_and_a_nan_pose_on_the_device():
    OS.same_tick_again(hip_rig)
    OS.strided(hip_rig)
    OS.strided(hip_rig, N=257, env_stride=3)
    hip, emu = OS.nan_pose(hip_rig), OS.nan_pose(OB.Rig)
    for h, e in zip(hip[:4], emu[:4]):          # the envs whose pose was not finite, up to the step after: exact parts only
        np.testing.assert_array_equal(OS.bits(h[1:3]), OS.bits(e[1:3]))


def test_refusals_on_device_memory_leave_everything_untouched():
    from isaacgymloco_amd import lib
    L = lib.load()
    OS.refusals(hip_rig, lambda: L.lsim_odometry_step(None, None))
