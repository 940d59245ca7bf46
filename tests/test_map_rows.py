"""The map-rows launch (lsim_map_rows, isaacgymloco_amd/csrc/ls_odometry.h) on the CPU: the kernel's own per-element code, compiled by g++
(tests/emu/emu_map_rows.cpp), bit for bit against fp32 numpy (tests/map_rows_scenes.py), and on the emulated env against the privileged
observation's own height-scan block."""
import ctypes

import numpy as np
import pytest
import torch

import map_rows_scenes as MS
import odometry_emu_binding as OB
from helpers import C, abi


def test_header_declares_the_launch():
    assert abi.PROTOTYPES["lsim_map_rows"] == (ctypes.c_int, [ctypes.POINTER(OB.LsimMapRows), ctypes.c_void_p])
    assert abi.LsimMapRows is OB.LsimMapRows


@pytest.mark.parametrize("N,P,channels", MS.CASES)
def test_rows_bit_for_bit_with_padding_and_guards(N, P, channels):
    MS.case(OB.RowsRig, N, P, channels)


def test_dense_strides_a_negative_scale_and_an_offset():
    MS.case(OB.RowsRig, 3, 187, 2, scan_pad=0, known_pad=0, ld_pad=0, z_offset=0.25, scale=-2.5)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_pose_writes_zeros_and_still_the_known_block(bad):
    got = MS.case(OB.RowsRig, 3, 99, 2, bad_z=bad)
    assert (got[2, :99] == 0).all() and (got[2, 99:198] == 1).any() and (got[0, :99] != 0).any()


def test_env_stride_leaves_the_rows_in_between():
    MS.case(OB.RowsRig, 7, 99, 2, env_stride=3)
    MS.case(OB.RowsRig, 3, 187, 1, env_stride=4)


def test_refusals_through_the_shim_and_through_the_library():
    MS.refusals(OB.RowsRig, lambda: OB.rows_lib().emu_map_rows(None, None))
    from isaacgymloco_amd import lib
    L = lib.load()             # loading needs no GPU; a refused launch never reaches one

    def on_the_library(*a, **kw):
        rig = OB.RowsRig(*a, **kw)
        rig._entry = L.lsim_map_rows
        return rig
    MS.refusals(on_the_library, lambda: L.lsim_map_rows(None, None), launches=False)


def test_fed_the_envs_own_heights_the_rows_are_the_privileged_scan_block_bit_for_bit():
    """the pin: z_offset 0.5 and scale obs_scales.height_measurements are ph_build_obs' expression (csrc/ls_post.h)"""
    from emu_env import EmuLeggedRobot
    from isaacgymloco_amd.learn.evaluate import play_cfg
    from isaacgymloco_amd.learn.vision import height_scan_block
    cfg = play_cfg(C.aliengo_cfg())                 # add_noise off -- which the height block's noise ignores (csrc/ls_post.h, LR:400):
    cfg.noise.noise_level = 0.0                     # its scale is what turns that one off
    cfg.env.num_envs = N = 6
    cfg.terrain.num_rows, cfg.terrain.num_cols = 2, 2
    cfg.terrain.terrain_proportions = [0.0, 0.0, 0.0, 0.0, 0.5, 0.5]
    env = EmuLeggedRobot(cfg, seed=3)
    env.reset()
    off, P = height_scan_block(env.cfg)
    rows = torch.full((N, P + 3), 555.0)
    mr = OB.LsimMapRows()
    mr.scan, mr.pose, mr.rows = env.measured_heights.data_ptr(), env.root_states.data_ptr(), rows.data_ptr()
    mr.num_points, mr.channels, mr.scan_stride, mr.ld = P, 1, env.measured_heights.stride(0), P + 3
    mr.num_envs, mr.env_stride, mr.z_offset, mr.scale = N, 1, 0.5, float(env.lcfg.obs_scale_height)
    g = torch.Generator().manual_seed(1)
    seen = set()
    for _ in range(4):
        env.step_device(torch.randn(N, 12, generator=g) * 0.4)
        assert OB.rows_lib().emu_map_rows(ctypes.byref(mr), None) == 0
        priv = env.get_privileged_observations()
        np.testing.assert_array_equal(MS.bits(rows[:, :P].numpy()), MS.bits(priv[:, off:off + P].numpy()))
        assert (rows[:, P:] == 555.0).all()
        seen.update(np.unique(rows[:, :P].numpy()).tolist())
    assert len(seen) > 20, "the scene has a terrain under it"
