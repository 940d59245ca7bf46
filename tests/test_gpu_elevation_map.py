"""GPU: the elevation-map launch (lsim_elevation_map, isaacgymloco_amd/csrc/ls_elevation_map.h) on a real device: the scenes of
tests/elevation_map_scenes.py against the numpy reference (tests/elevation_map_reference.py derives EPS and the comparison rule) and against
the CPU build of the same source.  Every GPU step is one launch over at most 257 envs."""
import numpy as np
import pytest

import elevation_map_emu_binding as EB
import elevation_map_reference as ER
import elevation_map_scenes as ES

pytestmark = pytest.mark.gpu
# (N, G, width, height, env_stride): R = 1, 193 (not a multiple of the block) and 3072 (the lanes loop twelve times); N = 257 with R = 193
# keeps the reference's per-ray loop short
SHAPES = [(1, 64, 1, 1, 1), (3, 64, 64, 48, 1), (257, 16, 193, 1, 1), (257, 64, 193, 1, 3), (3, 16, 64, 48, 2)]


def hip_rig(*a, **kw):
    from isaacgymloco_amd import lib
    return EB.Rig(*a, device="cuda:0", entry=lib.load().lsim_elevation_map, **kw)


def _same_bits(a, b):
    for k in ("height", "stamp", "cell", "scan", "known"):
        np.testing.assert_array_equal(ER.bits(a[k]), ER.bits(b[k]), err_msg=k)
    assert a["state"] == b["state"]


@pytest.mark.parametrize("N,G,width,height,env_stride", SHAPES)
def test_random_poses_on_the_device_and_against_the_cpu_build(N, G, width, height, env_stride):
    """each build lies inside the reference's bracket; where both know a cell their heights are two evaluations of points within EPS of
    the fp64 ones, so at most 2 EPS apart unless an ambiguous point separates them (at most the scene's ambiguous share of the cells)"""
    kw = dict(N=N, G=G, width=width, height=height, seed=N + G + width, env_stride=env_stride, labels=width == 193)
    hip, share = ES.random_poses(hip_rig, **kw)
    emu, _ = ES.random_poses(EB.Rig, **kw)
    both = (hip["stamp"] >= 0) & (emu["stamp"] >= 0)
    one = (hip["stamp"] >= 0) != (emu["stamp"] >= 0)
    eps = ER.eps(np.array([190.0, 190.0, 0.5]), np.array([0.3, 0.0, 0.05]), 4.9)
    far = np.abs(hip["height"][both].astype(np.float64) - emu["height"][both]) > 2.0 * eps
    cells = max(int(both.sum()), 1)
    print(f"elevation map N {N} G {G} R {width * height}: {int(both.sum())} cells known to both, {int(one.sum())} to one, {int(far.sum())} more than 2 EPS apart; "
          f"ambiguous share {share:.4%}")
    assert one.sum() <= 0.01 * cells + 2 and far.sum() <= 0.01 * cells + 2


def test_the_exact_scenes_bit_for_bit_on_a_side_stream():
    import torch
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        hip = ES.exact_basic(hip_rig)
        _same_bits(hip, ES.exact_basic(hip_rig, reverse=True))
        _same_bits(hip, ES.exact_basic(EB.Rig))
        _same_bits(ES.window_edges(hip_rig), ES.window_edges(EB.Rig))
        _same_bits(ES.negative_coordinates(hip_rig), ES.negative_coordinates(EB.Rig))
        _same_bits(ES.scan_frame(hip_rig), ES.scan_frame(EB.Rig))
        _same_bits(ES.invalid_rays(hip_rig), ES.invalid_rays(EB.Rig))
        _same_bits(ES.big_ticks(hip_rig), ES.big_ticks(EB.Rig))
    torch.cuda.synchronize()


@pytest.mark.parametrize("G", [16, 64])
def test_scrolling_on_the_device(G):
    for h, e in zip(ES.scrolling(hip_rig, G), ES.scrolling(EB.Rig, G)):
        _same_bits(h, e)


@pytest.mark.parametrize("flags,stagger,env_stride", [(0, 1, 1), (ER.RESETS_ONLY, 0, 3), (ER.FILL_ALL, 0, 1)])
def test_the_due_set_on_the_device(flags, stagger, env_stride):
    for h, e in zip(ES.due_sets(hip_rig, flags, stagger, env_stride), ES.due_sets(EB.Rig, flags, stagger, env_stride)):
        _same_bits(h, e)


def test_non_finite_poses_on_the_device():
    _same_bits(ES.nonfinite_pose(hip_rig), ES.nonfinite_pose(EB.Rig))


def test_refusals_on_the_device_leave_memory_untouched():
    from isaacgymloco_amd import lib
    from test_elevation_map import refusals
    L = lib.load()
    refusals(hip_rig, lambda: L.lsim_elevation_map(None, None))
