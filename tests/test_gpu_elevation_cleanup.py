"""GPU: lsim_elevation_map_cleanup (isaacgymloco_amd/csrc/ls_elevation_cleanup.h) on a real device: the dyadic scenes of
tests/elevation_cleanup_scenes.py against the float64 reference and against the CPU build of the same source, general poses inside the
reference's bracket, and ray order / repeated launches on a side stream.  Every GPU step is one launch over at most 257 envs."""
import numpy as np
import pytest

import elevation_cleanup_reference as CR
import elevation_cleanup_scenes as CS
import elevation_map_reference as ER

pytestmark = pytest.mark.gpu


def _lib():
    from isaacgymloco_amd import lib
    return lib.load()


def hip_rig(cleanup=None):
    return CR.cleanup_rig(cleanup, device="cuda:0", entry=_lib().lsim_elevation_map_cleanup, map_entry=_lib().lsim_elevation_map)


def _as_list(x):
    return x if isinstance(x, list) else [x]


@pytest.mark.parametrize("G", [16, 64])
@pytest.mark.parametrize("scene", sorted(CS.EXACT))
def test_dyadic_scenes_on_the_device(scene, G):
    """each launch inside the reference's rule (no slot of these scenes is ambiguous), and stamps and cleared equal to the CPU build's"""
    hip, emu = _as_list(CS.EXACT[scene](hip_rig(), G=G)), _as_list(CS.EXACT[scene](CR.cleanup_rig(), G=G))
    for a, b in zip(hip, emu):
        for k in ("stamp", "cleared"):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.parametrize("flags,stagger,env_stride", [(0, 1, 2), (ER.FILL_ALL, 0, 1), (ER.RESETS_ONLY, 1, 3)])
def test_due_sets_on_the_device(flags, stagger, env_stride):
    hip, emu = CS.due_sets(hip_rig(), flags, stagger, env_stride), CS.due_sets(CR.cleanup_rig(), flags, stagger, env_stride)
    for a, b in zip(hip, emu):
        for k in ("stamp", "cleared"):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.parametrize("shape", sorted(CS.SHAPES))
def test_general_poses_inside_the_bracket(shape):
    """the reference's bracket, what is never written, the guards; the ambiguous share (printed) at most 1 %"""
    after, share, gone, fresh = CS.general(hip_rig(), *shape, var=shape[1] == 64)
    if shape[2] >= 193:
        assert gone.sum() > 0
    if fresh is not None:
        assert gone[fresh] == 0 and after["cleared"][fresh] == 0


def test_side_stream_ray_order_and_repeated_launch():
    import torch
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        fwd = CS.general(hip_rig(), 3, 64, 513, var=True, stream=side)[0]
        rev = CS.general(hip_rig(), 3, 64, 513, var=True, stream=side, reverse=True)[0]
        again = CS.general(hip_rig(), 3, 64, 513, var=True, stream=side)[0]
    torch.cuda.synchronize()
    for k in ("stamp", "cleared"):
        np.testing.assert_array_equal(fwd[k], rev[k], err_msg=f"{k} depends on the order of the rays")
        np.testing.assert_array_equal(fwd[k], again[k], err_msg=f"{k} differs between two runs")


def test_refusals_on_device_memory():
    rig = CS.start(hip_rig(), 2, np.array([CS.DOWN, CS.DOWN], np.float32), var=True)
    for e in range(2):
        CS.plant(rig, e, {(2, 0): 0.25})
    before = rig.read()
    for field, value in (("cleared", 0), ("clear_margin", -1.0), ("clear_slope", float("nan")), ("clear_sigma", float("inf")), ("end_gap", -0.5), ("min_rays", 0)):
        assert rig.launch(5, 0, edit_cleanup=lambda ec: setattr(ec, field, value)) != 0, field
    assert rig.launch(5, 0, edit=lambda em: setattr(em, "size", 8)) != 0
    after = rig.read()
    for k in ("height", "stamp", "cell", "scan", "known", "cleared", "var"):
        np.testing.assert_array_equal(ER.bits(before[k]), ER.bits(after[k]), err_msg=f"a refused launch wrote {k}")
    assert rig.launch(5, 0) == 0
