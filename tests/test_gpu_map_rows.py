"""GPU: the map-rows launch (lsim_map_rows, isaacgymloco_amd/csrc/ls_odometry.h) on a real device: the cases of tests/map_rows_scenes.py bit
for bit against fp32 numpy and against the CPU build of the same source (the expression has nothing a compiler can fuse), at sizes that
cross a block, on a side stream, and the refusals on device memory.  Every GPU step is one launch over at most 257 envs."""
import numpy as np
import pytest

import map_rows_scenes as MS
import odometry_emu_binding as OB

pytestmark = pytest.mark.gpu


def hip_rig(*a, **kw):
    from isaacgymloco_amd import lib
    return OB.RowsRig(*a, device="cuda:0", entry=lib.load().lsim_map_rows, **kw)


@pytest.mark.parametrize("N,P,channels", MS.CASES + [(257, 187, 1), (257, 99, 2), (257, 256, 2)])
def test_rows_on_the_device_equal_the_reference_and_the_cpu_build(N, P, channels):
    hip = MS.case(hip_rig, N, P, channels)
    np.testing.assert_array_equal(MS.bits(hip), MS.bits(MS.case(OB.RowsRig, N, P, channels)))


def test_env_stride_non_finite_pose_and_dense_strides_on_the_device():
    MS.case(hip_rig, 257, 99, 2, env_stride=3)
    MS.case(hip_rig, 7, 187, 1, env_stride=4)
    for bad in (np.nan, np.inf, -np.inf):
        got = MS.case(hip_rig, 3, 99, 2, bad_z=bad)
        assert (got[2, :99] == 0).all()
    MS.case(hip_rig, 3, 187, 2, scan_pad=0, known_pad=0, ld_pad=0, z_offset=0.25, scale=-2.5)


def test_a_case_on_a_side_stream():
    import torch
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        MS.case(hip_rig, 257, 187, 2, stream=side.cuda_stream)
    torch.cuda.synchronize()


def test_refusals_on_device_memory_leave_the_rows_untouched():
    from isaacgymloco_amd import lib
    L = lib.load()
    MS.refusals(hip_rig, lambda: L.lsim_map_rows(None, None))
