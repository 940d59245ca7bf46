"""CPU: the elevation-map source (isaacgymloco_amd/csrc/ls_elevation_map.h) compiled by g++ under LS_EMU, against the numpy reference of
tests/elevation_map_reference.py (written from include/lsim.h; its docstring derives EPS and the comparison rule).  The same scenes run on
the HIP launch in tests/test_gpu_elevation_map.py."""
import math

import numpy as np
import pytest

import elevation_map_emu_binding as EB
import elevation_map_reference as ER
import elevation_map_scenes as ES
from helpers import abi


def test_exact_scene_bit_for_bit_and_the_same_with_the_rays_reversed():
    fwd, rev = ES.exact_basic(EB.Rig), ES.exact_basic(EB.Rig, reverse=True)
    for k in ("height", "stamp", "cell", "scan", "known"):
        np.testing.assert_array_equal(ER.bits(fwd[k]), ER.bits(rev[k]))


def test_window_edges():
    ES.window_edges(EB.Rig)


def test_negative_coordinates_take_a_true_floor():
    ES.negative_coordinates(EB.Rig)


@pytest.mark.parametrize("G", [16, 32, 64])
def test_scrolling_keeps_what_stays_in_the_window(G):
    ES.scrolling(EB.Rig, G)


@pytest.mark.parametrize("flags,stagger,env_stride", [(0, 0, 1), (0, 1, 1), (ER.FILL_ALL, 1, 1), (ER.RESETS_ONLY, 0, 1), (0, 1, 3), (ER.RESETS_ONLY, 1, 3)])
def test_the_due_set_is_the_captures(flags, stagger, env_stride):
    ES.due_sets(EB.Rig, flags, stagger, env_stride)


def test_invalid_rays_insert_nothing():
    ES.invalid_rays(EB.Rig)


def test_a_non_finite_pose_gives_zero_rows_and_a_count():
    ES.nonfinite_pose(EB.Rig)


def test_the_scan_turns_with_the_yaw_only():
    ES.scan_frame(EB.Rig)


MUTANT_SCENES = {"last_ray_wins": ES.exact_basic, "truncate": ES.negative_coordinates, "upper_edge_inclusive": ES.window_edges,
                 "clear_when_due": ES.due_sets, "scan_full_quat": ES.scan_frame}


@pytest.mark.parametrize("mutant", ER.MUTANTS)
def test_a_mutant_of_the_reference_fails(mutant):
    with pytest.raises(AssertionError):
        MUTANT_SCENES[mutant](EB.Rig, mutant=mutant)


@pytest.mark.parametrize("seed", [0, 1])
def test_random_poses_under_the_comparison_rule(seed):
    """roll and pitch up to 0.4 rad, a 16 x 12 camera, N = 5, one env 190 m from the origin; the ambiguous share is a condition on the scene"""
    _, worst = ES.random_poses(EB.Rig, N=5, G=16, width=16, height=12, seed=seed)
    print(f"random poses seed {seed}: largest ambiguous share {worst:.4%}")
    _, worst = ES.random_poses(EB.Rig, N=5, G=64, width=16, height=12, seed=seed + 10, labels=True, env_stride=2)
    print(f"random poses G 64 seed {seed + 10}: largest ambiguous share {worst:.4%}")


def test_the_ambiguous_share_at_190_m_is_what_the_reference_derives():
    """a condition, not a measurement: the reference alone, on a dense camera, one env at the origin and one 190 m from it"""
    rig = ES.random_rig(EB.Rig, 2, 64, 64, 48, seed=3)
    par, inp = ER.Params.of(rig), rig.inputs()
    for e in (0, 1):
        _, E, amb, n = ER.bracket(par, inp, e)
        assert n > 1000 and amb / n <= 0.01 and E < 7e-5
        print(f"env {e}: EPS {E:.2e} m, ambiguous share {amb / n:.4%} of {n}")


def _edits():
    nan, inf = math.nan, math.inf

    def s(name, value):
        return lambda em: setattr(em, name, value)

    def off(name, by):
        return lambda em: setattr(em, name, getattr(em, name) + by)

    edits = {f"{n} NULL": s(n, None) for n in ("root_states", "assumed_mount", "dirs", "depth", "pts", "height", "stamp", "cell", "scan", "known",
                                               "episode_length", "state")}
    edits.update({f"{n} misaligned": off(n, 2) for n in ("root_states", "assumed_mount", "dirs", "depth", "pts", "height", "stamp", "cell", "scan", "inv_scale")})
    edits.update({"episode_length misaligned": off("episode_length", 4), "state misaligned": off("state", 4)})
    edits.update({f"size {g}": s("size", g) for g in (0, 8, 24, 48, 128, -16)})
    for n in ("res", "a", "b", "unknown_drop"):
        edits.update({f"{n} nan": s(n, nan), f"{n} inf": s(n, inf)})
    edits.update({"res 0": s("res", 0.0), "res < 0": s("res", -0.0625), "t_lo < 0": s("t_lo", -0.5), "t_lo == t_hi": s("t_lo", 4.0), "t_lo > t_hi": s("t_lo", 5.0),
                  "t_lo nan": s("t_lo", nan), "t_hi nan": s("t_hi", nan),
                  "P 0": s("num_points", 0), "P 257": s("num_points", 257), "R 0": s("num_rays", 0), "R too large": s("num_rays", abi.DEFINES["LSIM_RAYCAST_MAX_RAYS"] + 1),
                  "depth_stride < R": s("depth_stride", 7), "label_stride < R": s("label_stride", 7), "scan_stride < P": s("scan_stride", 9),
                  "known_stride < P": s("known_stride", 9), "tick < 0": s("tick", -1), "period 0": s("period", 0), "stagger 2": s("stagger", 2),
                  "stagger < 0": s("stagger", -1), "env_stride 0": s("env_stride", 0), "num_envs 0": s("num_envs", 0),
                  "unknown flag": s("flags", 4), "both flags": s("flags", ER.FILL_ALL | ER.RESETS_ONLY)})
    return edits


def refusals(make_rig, null_call):
    """every refusal of the header returns LSIM_E_INVALID and writes nothing: the written arrays keep their initial values and their guards"""

    def rig_():
        rig = make_rig(3, 16, ES.DIRS8, ES.PTS, res=ES.RES, labels=True, inv_scale=np.ones(8, np.float32), t_hi=4.0)
        rig.put("depth", ES.exact_depths(3, 8) * np.float32(0.25))
        rig.put("episode_length", 0)
        return rig

    def untouched(got):
        return all((got[k] == np.array(EB.INITIAL[k]).astype(EB.WRITTEN[k])).all() for k in EB.WRITTEN) and got["state"] == 0

    rig = rig_()
    assert rig.launch(3) == 0 and not untouched(rig.read())
    assert null_call() == abi.E_INVALID
    for what, edit in _edits().items():
        rig = rig_()
        assert rig.launch(3, 0, edit) == abi.E_INVALID, what
        assert untouched(rig.read()), what
    for edit in (lambda em: setattr(em, "num_points", 10), lambda em: setattr(em, "inv_scale", None), lambda em: setattr(em, "labels", None),
                 lambda em: setattr(em, "tick", 2 ** 40), lambda em: setattr(em, "t_lo", 0.0)):
        assert rig_().launch(3, 0, edit) == 0
    for G in (32, 64):
        assert make_rig(2, G, ES.DIRS8, ES.PTS).launch(0, ER.FILL_ALL) == 0


def test_every_invalid_argument_is_refused_and_nothing_is_written():
    L = EB.lib()
    refusals(EB.Rig, lambda: L.emu_elevation_map(None, None))


def test_the_library_refuses_the_same_arguments_before_any_launch():
    """through lib.load(): the argument check runs on the host before any HIP call, so host arrays serve and no device is needed"""
    from isaacgymloco_amd import lib
    L = lib.load()
    assert L.lsim_elevation_map(None, None) == abi.E_INVALID
    for what, edit in _edits().items():
        rig = EB.Rig(3, 16, ES.DIRS8, ES.PTS, labels=True, inv_scale=np.ones(8, np.float32), t_hi=4.0)
        rig._entry = L.lsim_elevation_map
        assert rig.launch(3, 0, edit) == abi.E_INVALID, what
        got = rig.read()
        assert all((got[k] == np.array(EB.INITIAL[k]).astype(EB.WRITTEN[k])).all() for k in EB.WRITTEN), what


def test_the_big_tick_stamps_its_low_word():
    rig = EB.Rig(1, 16, ES.DIRS8, ES.PTS)
    rig.put("depth", ES.exact_depths(1, 8) * np.float32(0.25))
    assert rig.launch(2 ** 40 + 9, ER.FILL_ALL) == 0
    st = rig.read()["stamp"]
    assert set(np.unique(st)) == {-1, 9}


def test_a_tick_with_bit_31_set_still_stamps_known_cells():
    """the stamp is the tick's low 31 bits: never negative, so the cells of such a capture are known, as the reference says bit for bit"""
    ES.big_ticks(EB.Rig)
