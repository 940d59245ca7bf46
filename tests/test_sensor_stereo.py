"""lsim_sensor_stereo on the CPU shim (tests/emu/emu_sensor_stereo.cpp: the kernel's own per-lane functions under g++) against the numpy
reference of tests/sensor_stereo_reference.py on the scenes of tests/sensor_stereo_scenes.py.  Every comparison is exact equality of hist
and state: the contract is defined on the stored bits of depth."""
import ctypes

import numpy as np
import pytest

import sensor_stereo_emu_binding as B
import sensor_stereo_reference as REF
import sensor_stereo_scenes as SC
from helpers import abi

FLT_MAX = float(np.finfo(np.float32).max)
SCENES = SC.scenes()
IDS = [s["name"] for s in SCENES]
# (name, flags, period, tick, the episode lengths of envs 0, 1, 2)
MODES = (("fill", REF.FILL_ALL, 1, 5, (1, 1, 1)), ("due", 0, 1, 5, (1, 1, 1)), ("not_due", 0, 7, 5, (1, 1, 1)), ("resets_only", REF.RESETS_ONLY, 1, 5, (0, 1, 0)),
          ("one_reset", 0, 7, 5, (1, 1, 0)))


def rig_of(scene, **kw):
    return B.Rig(scene["width"], scene["height"], scene["depth"], scene["labels"], scene["inv_scale"], scene["inst"], **dict(scene["params"], **kw))


def run(rig, mode, mutant=None, launches=1):
    """the rig launched under `mode`; returns (what the launch left, what the reference -- or its mutant -- expects)"""
    _, flags, period, tick, lengths = mode
    rig.put("episode_length", np.array(lengths, np.int64))
    before, inp = rig.read(), rig.inputs()
    p = dict(rig.p, period=period)

    def edit(st):
        st.period = period
    for _ in range(launches):
        assert rig.launch(tick, flags, edit) == 0
    want = REF.apply(before["hist"], before["state"], inp["depth"], inp["labels"], inp["inv_scale"], inp["episode_length"], inp["inst"], p, tick, flags, mutant)
    return before, inp, rig.read(), want


def same(a, b):
    return a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()


@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("scene", SCENES, ids=IDS)
def test_scene_matches_the_reference_bit_for_bit(scene, mode):
    rig = rig_of(scene)
    before, inp, got, (hist, state, codes) = run(rig, mode)
    assert same(got["hist"], hist), f"{int((got['hist'].view(np.uint32) != hist.view(np.uint32)).sum())} elements differ"
    assert (got["state"] == state).all(), (got["state"], state)
    assert same(got["hist_pad"], before["hist_pad"]), "the padding of a slot was written"
    assert same(rig.inputs()["depth"], inp["depth"]), "depth was written"
    if inp["labels"] is not None:
        assert (rig.inputs()["labels"] == inp["labels"]).all(), "labels were written"
    due, _ = REF.SR.due_sets(rig.N, rig.p["env_stride"], mode[3], mode[2], rig.p["stagger"], mode[1], inp["episode_length"])
    assert same(got["hist"][~due], before["hist"][~due]), "an env that is not due was written"
    if mode[0] == "not_due":
        assert not due.any() and (got["state"] == before["state"]).all()
    if scene["holes"] is not None:                  # the band, stated by hand
        holes = scene["holes"].reshape(rig.N, -1) & due[:, None]
        assert ((codes == REF.HOLE) == holes).all()
        yh = REF.y_hole(rig.p)
        changed = got["hist"][:, rig.K - 1].view(np.uint32) != before["hist"][:, rig.K - 1].view(np.uint32)
        assert (changed == holes).all() and (got["hist"][:, rig.K - 1][holes] == yh).all()
        assert got["state"][0] - before["state"][0] == holes.sum() and got["state"][1] == before["state"][1]


def test_scenes_cover_what_they_should():
    """the scene list itself: holes and fattened pixels occur, and a fattened pixel's foreground is itself rewritten somewhere"""
    seen = {"hole": 0, "fatten": 0, "fg_rewritten": 0}
    for scene in SCENES:
        rig = rig_of(scene)
        inp = rig.inputs()
        for e in range(0, rig.N, rig.p["env_stride"]):
            code, fg = REF.decide(inp["depth"][e], None if inp["labels"] is None else inp["labels"][e], inp["inv_scale"],
                                  None if inp["inst"] is None else inp["inst"][e], rig.p, e, 5)
            seen["hole"] += int((code == REF.HOLE).sum())
            seen["fatten"] += int((code == REF.FATTEN).sum())
            seen["fg_rewritten"] += int((code[fg[fg >= 0]] != REF.KEEP).sum())
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("mutant", REF.MUTANTS)
def test_every_mutant_of_the_reference_is_told_apart(mutant):
    """a reference with one line restated wrongly must differ from the shim on at least one scene and mode"""
    for scene in SCENES:
        for mode in MODES[:2] + MODES[3:]:
            _, _, got, (hist, state, _) = run(rig_of(scene), mode, mutant)
            if not same(got["hist"], hist) or (got["state"] != state).any():
                return
    pytest.fail(f"no scene tells the mutant {mutant!r} from the contract")


@pytest.mark.parametrize("scene", SCENES, ids=IDS)
def test_identity_writes_nothing(scene):
    """fb = 0, no minimum range, both probabilities 0: nothing is written and the state stays"""
    rig = rig_of(scene, fb=0.0, max_disparity=FLT_MAX, p_edge_hole=0.0, p_edge_cum=0.0)
    for mode in MODES:
        before, _, got, _ = run(rig, mode)
        assert same(got["hist"], before["hist"]) and (got["state"] == before["state"]).all(), mode[0]


@pytest.mark.parametrize("scene", [SCENES[0], SCENES[8], SCENES[-1]], ids=[IDS[0], IDS[8], IDS[-1]])
def test_two_launches_write_the_same_bits(scene):
    """a second launch on the same inputs (the rewritten hist included: depth is what it decides from) leaves hist as the first did, when no
    pixel is fattened from a rewritten one; and two rigs launched once agree bit for bit"""
    a, b = rig_of(scene), rig_of(scene)
    _, _, got_a, _ = run(a, MODES[1])
    _, _, got_b, _ = run(b, MODES[1])
    assert same(got_a["hist"], got_b["hist"]) and (got_a["state"] == got_b["state"]).all()
    before, _, again, want = run(a, MODES[1])
    assert same(again["hist"], want[0]) and (again["state"] == want[1]).all()
    assert (again["state"] - before["state"] == got_a["state"]).all()


def test_sizes():
    L = B.lib()
    n = ctypes.c_size_t()
    assert L.emu_sensor_stereo_sizes(64, 48, ctypes.byref(n)) == 0 and n.value == 16 + 13 * 3072
    assert L.emu_sensor_stereo_sizes(20, 5, ctypes.byref(n)) == 0 and n.value == 16 + 12 * 100 + 100
    assert L.emu_sensor_stereo_sizes(7, 3, ctypes.byref(n)) == 0 and n.value == 16 + 12 * 21 + 24
    limit = abi.DEFINES["LSIM_STEREO_MAX_LDS_BYTES"]
    assert L.emu_sensor_stereo_sizes(12601, 1, ctypes.byref(n)) == 0 and n.value <= limit
    assert L.emu_sensor_stereo_sizes(6301, 2, ctypes.byref(n)) == abi.DEFINES["LSIM_E_INVALID"]
    for w, h in ((0, 4), (4, 0), (-1, 4), (2 ** 30, 2 ** 30), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert L.emu_sensor_stereo_sizes(w, h, ctypes.byref(n)) == abi.DEFINES["LSIM_E_INVALID"], (w, h)
    assert L.emu_sensor_stereo_sizes(4, 4, None) == abi.DEFINES["LSIM_E_INVALID"]


def _set(**kw):
    def edit(st):
        for k, v in kw.items():
            setattr(st, k, v)
    return edit


def _bump(name, by):
    def edit(st):
        setattr(st, name, (getattr(st, name) or 0) + by)
    return edit


NAN, INF = float("nan"), float("inf")
REFUSALS = [(f"{k}_null", _set(**{k: None})) for k in ("depth", "episode_length", "hist", "state")]
REFUSALS += [("depth_misaligned", _bump("depth", 2)), ("hist_misaligned", _bump("hist", 4)), ("inv_scale_misaligned", _bump("inv_scale", 1)),
             ("inst_misaligned", _bump("inst", 8)), ("episode_length_misaligned", _bump("episode_length", 4)), ("state_misaligned", _bump("state", 4))]
REFUSALS += [(f"{k}={v}", _set(**{k: v})) for k, v in (
    ("width", 0), ("height", 0), ("width", -16), ("height", 12602), ("window", 0), ("window", 129), ("edge_radius", -1), ("edge_radius", 4),
    ("fb", -1.0), ("fb", NAN), ("fb", INF), ("edge_rel", -0.1), ("edge_rel", NAN), ("edge_rel", 1.0), ("p_edge_hole", -0.1), ("p_edge_hole", NAN),
    ("p_edge_cum", NAN), ("p_edge_cum", 1.5), ("max_disparity", 0.0), ("max_disparity", -1.0), ("max_disparity", NAN), ("t_lo", -0.5), ("t_lo", NAN),
    ("t_hi", NAN), ("t_hi", 0.0625), ("depth_stride", 95), ("label_stride", 95), ("hist_stride", 92), ("hist_stride", 98), ("latency", -1), ("frames", 0),
    ("latency", 8), ("num_envs", 0), ("env_stride", 0), ("tick", -1), ("stream_id", 65536), ("period", 0), ("stagger", 2), ("stagger", -1), ("flags", 4),
    ("flags", 3), ("drop_value", NAN), ("clip_lo", INF), ("clip_hi", NAN), ("clip_lo", 9.0), ("offset", NAN), ("gain", INF))]
REFUSALS += [("p_edge_cum_below_hole", _set(p_edge_hole=0.5, p_edge_cum=0.25)), ("null_struct", None)]


@pytest.mark.parametrize("name,edit", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_write_nothing(name, edit):
    scene = SCENES[7]                           # per_pixel, every pixel at an edge a hole: a launch that went through would write
    rig = B.Rig(scene["width"], scene["height"], scene["depth"], scene["labels"], np.ones(96, np.float32), np.tile(np.array([[1, 1, 0, 0, 1, 0, 0, 0]], np.float32), (3, 1)),
                **scene["params"])
    before = rig.read()
    if edit is None:
        rc = B.lib().emu_sensor_stereo(None, None)
    else:
        rc = rig.launch(5, 0, edit)
    assert rc == abi.DEFINES["LSIM_E_INVALID"], name
    got = rig.read()
    assert same(got["hist"], before["hist"]) and (got["state"] == before["state"]).all()
    assert rig.launch(5, 0) == 0 and rig.read()["state"][0] > 0          # the unedited struct goes through and writes


def test_optional_pointers_may_be_null_and_infinite_disparity_is_no_minimum_range():
    scene = SCENES[6]
    rig = rig_of(scene, max_disparity=INF)
    assert rig.st.inv_scale is None and rig.st.inst is None
    _, _, got, (hist, state, codes) = run(rig, MODES[1])
    assert same(got["hist"], hist) and (got["state"] == state).all()
    assert codes[0].reshape(6, 16)[4, 12] == REF.KEEP and codes[0].reshape(6, 16)[4, 11] == REF.HOLE     # not too near, and it still occludes
