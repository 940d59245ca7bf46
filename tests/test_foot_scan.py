"""The foot-scan launch (lsim_foot_scan, isaacgymloco_amd/csrc/ls_foot_scan.h) on the CPU: the kernel's own per-lane code, compiled by g++
(tests/emu/emu_foot_scan.cpp), against the float64 reference written from the header (tests/foot_scan_reference.py) on the scenes of
tests/foot_scan_scenes.py -- bit for bit on the exact scenes, by the reference's ambiguity rule on the general ones -- and against the
simulator's own reference-pinned height sampler."""
import ctypes

import numpy as np
import pytest

import foot_scan_emu_binding as FB
import foot_scan_reference as FR
import foot_scan_scenes as FS
from helpers import C, abi

F = np.float32


def test_header_declares_the_launch_and_its_constants():
    assert abi.PROTOTYPES["lsim_foot_scan"] == (ctypes.c_int, [ctypes.POINTER(FB.LsimFootScan), ctypes.c_void_p])
    assert abi.LsimFootScan is FB.LsimFootScan
    assert (FB.MAX_POINTS, FB.TERRAIN, FB.MAP) == (64, 0, 1) and (FR.TERRAIN, FR.MAP) == (FB.TERRAIN, FB.MAP)


@pytest.mark.parametrize("source,N,K,G,stride", FS.EXACT_CASES)
def test_exact_scenes_bit_for_bit(source, N, K, G, stride):
    sc = FS.exact_scene(source, N, K, G=G, env_stride=stride)
    got, ref, _ = FS.run(FB.Rig, sc, exact=True, label=f"source {source} N {N} K {K} G {G} stride {stride}")
    cat = ref["category"][ref["visited"]]
    if source == FR.MAP:
        # the three states of a slot under the first three feet: known, left over from a cell that scrolled out (must read unknown), never written
        assert (cat[:, 0] == 0).all() and (cat[:, K] == 2).all() and (cat[:, 2 * K] == 1).all()
        assert (got["known"][ref["visited"]][:, K] == 0).all() and (got["known"][ref["visited"]][:, 0] == 1).all()
    elif K >= 7:
        assert (cat == 3).any() and (cat == 0).any(), "a point outside the grid, which the sampler clips, and points inside"
    assert len(np.unique(got["heights"][ref["visited"]][:, :4 * K])) > 1 or K == 1


def test_one_channel_rows_only_and_the_plane():
    for source in (FR.TERRAIN, FR.MAP):
        sc = FS.exact_scene(source, 5, 7, channels=1)
        FS.run(FB.Rig, sc, exact=True, label=f"one channel, source {source}")
        rig = FB.Rig(sc, outputs=False)              # heights and known NULL: only rows and state are written
        assert rig.launch() == 0
        np.testing.assert_array_equal(FR.bits(rig.read()["rows"][:, :28]), FR.bits(FR.reference(sc)["rows"]))
    sc = FS.exact_scene(FR.TERRAIN, 5, 7, mesh_type=0)
    got, ref, _ = FS.run(FB.Rig, sc, exact=True, label="plane")
    assert (got["heights"][:, :28] == 0).all() and (got["known"][:, :28] == 1).all()
    z = np.repeat(ref["centres"][:, :, 2], 7, axis=1).astype(F)
    np.testing.assert_array_equal(got["rows"][:, :28], np.clip(z - F(sc["z_offset"]), -1, 1) * F(sc["scale"]))


@pytest.mark.parametrize("source,K,G", FS.GENERAL_CASES)
def test_general_scenes_two_robots_in_one_launch(source, K, G):
    sc = FS.general_scene(source, 33, K, G=G)
    got, ref, share = FS.run(FB.Rig, sc, exact=False, label=f"general source {source} K {K} G {G}")
    assert set(sc["env_robot"].tolist()) == {0, 1}
    if source == FR.MAP:
        assert {0, 1, 2} <= set(ref["category"].reshape(-1).tolist())
    assert np.abs(got["rows"][:, :4 * K]).max() == 5.0 and (np.abs(got["rows"][:, :4 * K]) < 5.0).any(), "values on and inside the clamp"


def test_the_two_tables_give_different_feet_and_env_robot_chooses():
    sc = dict(FS.general_scene(FR.TERRAIN, 33, 7))
    ref = FR.reference(sc)
    sc["env_robot"] = 1 - sc["env_robot"]
    other = FR.reference(sc)
    assert np.abs(ref["centres"] - other["centres"]).max() > 0.01
    FS.run(FB.Rig, sc, exact=False, ref=other, label="robots swapped")


@pytest.mark.parametrize("source", [FR.TERRAIN, FR.MAP])
def test_bad_envs_write_zeros_are_counted_and_leave_their_neighbours(source):
    base = FS.general_scene(source, 9, 7)
    clean = FS.run(FB.Rig, base, exact=False, label="clean")[0]
    sc = dict(base, pose=base["pose"].copy(), dof_pos=base["dof_pos"].copy())
    sc["pose"][1, 1] = np.nan
    sc["pose"][3, 4] = np.inf
    sc["dof_pos"][5, 7] = np.nan
    sc["pose"][7, 5:7] = 0.0
    rig = FB.Rig(sc)
    got = rig.run()
    ref = FR.reference(sc)
    assert ref["bad"].tolist() == [e in (1, 3, 5, 7) for e in range(9)]
    FR.check(sc, ref, got, exact=False, label="bad envs")
    for e in (1, 3, 5, 7):
        assert (got["rows"][e, :56] == 0).all() and (got["heights"][e, :28] == 0).all() and (got["known"][e, :28] == 0).all()
    for e in (0, 2, 4, 6, 8):
        for k in ("rows", "heights", "known"):
            np.testing.assert_array_equal(got[k][e], clean[k][e])
    assert got["state"] == 4
    assert rig.launch() == 0 and rig.read()["state"] == 8, "cumulative"
    assert not np.isnan(rig.read()["rows"]).any()


def test_refusals_through_the_shim_and_through_the_library():
    FS.refusals(FB.Rig, lambda: FB.lib().emu_foot_scan(None, None))
    from isaacgymloco_amd import lib
    L = lib.load()             # loading needs no GPU; a refused launch never reaches one

    def on_the_library(sc, **kw):
        rig = FB.Rig(sc, **kw)
        rig._entry = L.lsim_foot_scan
        return rig
    FS.refusals(on_the_library, lambda: L.lsim_foot_scan(None, None), launches=False)


def test_the_terrain_source_is_the_simulators_own_height_sampler_bit_for_bit():
    """the pin: with every leg offset zeroed each "foot" is the base, and a pattern of the first 64 measured points then samples what
    LSIM_BUF_MEASURED_HEIGHTS[:, :64] holds -- the sampler that is itself pinned to the reference (csrc/ls_post.h, ls_sample_height_min3)"""
    from emu_env import EmuLeggedRobot
    from isaacgymloco_amd.learn.evaluate import play_cfg
    cfg = play_cfg(C.aliengo_cfg())
    cfg.env.num_envs = N = 6
    cfg.terrain.num_rows, cfg.terrain.num_cols = 2, 2
    cfg.terrain.terrain_proportions = [0.0, 0.5, 0.25, 0.25, 0.0, 0.0]
    env = EmuLeggedRobot(cfg, seed=3)
    env.reset()
    t = env.cfg.terrain
    pattern = np.array([[x, y] for x in t.measured_points_x for y in t.measured_points_y][:64], F)
    import torch
    g = torch.Generator().manual_seed(1)
    seen = set()
    for _ in range(4):
        env.step_device(torch.randn(N, 12, generator=g) * 0.4)
        if bool(env.reset_buf.any()):
            continue
        sc = dict(source=FR.TERRAIN, pose=env.root_states.numpy().copy(), dof_pos=env.dof_pos.numpy().copy(), tables=[FS.dyadic_table(zero_legs=True)],
                  env_robot=None, pattern=pattern, env_stride=1, channels=1, z_offset=0.5, scale=float(env.lcfg.obs_scale_height), mesh_type=1,
                  height_grid=env.height_samples.numpy().copy(), hs=t.horizontal_scale, vs=t.vertical_scale, border=t.border_size)
        got = FB.Rig(sc).run()
        want = np.tile(env.measured_heights.numpy()[:, :64], (1, 4))
        np.testing.assert_array_equal(FR.bits(got["heights"][:, :256]), FR.bits(want))
        seen.update(np.unique(want).tolist())
    assert len(seen) > 20, "the scene has a terrain under it"
