"""GPU: lsim_sensor_stereo (isaacgymloco_amd/csrc/ls_sensor_stereo.h) on a real device against the numpy reference of
tests/sensor_stereo_reference.py, exact: the scenes of tests/sensor_stereo_scenes.py, images of R = 96, 100, 3072 and the largest the LDS
plan takes (12 601 pixels, 163 832 B), N = 1 and 257, the image one past the limit refused.  Every GPU step is one launch."""
import ctypes

import numpy as np
import pytest

import sensor_stereo_emu_binding as B
import sensor_stereo_reference as REF
import sensor_stereo_scenes as SC
from helpers import abi
from test_sensor_stereo import MODES, run, same

pytestmark = pytest.mark.gpu
F = np.float32
SCENES = SC.scenes()


def _entry():
    from isaacgymloco_amd import lib
    return lib.load().lsim_sensor_stereo


def hip_rig(scene, **kw):
    return B.Rig(scene["width"], scene["height"], scene["depth"], scene["labels"], scene["inv_scale"], scene["inst"], device="cuda:0", entry=_entry(),
                 **dict(scene["params"], **kw))


def check(rig, mode):
    before, inp, got, (hist, state, _) = run(rig, mode)
    assert same(got["hist"], hist), f"{int((got['hist'].view(np.uint32) != hist.view(np.uint32)).sum())} elements differ"
    assert (got["state"] == state).all(), (got["state"], state)
    assert same(got["hist_pad"], before["hist_pad"])
    return got


@pytest.mark.parametrize("scene", SCENES, ids=[s["name"] for s in SCENES])
def test_scenes_on_the_device(scene):
    rig = hip_rig(scene)
    for mode in MODES:                     # one rig through every mode: each launch starts from what the last one left
        check(rig, mode)


def random_image(N, W, H, seed):
    """a floor whose depth falls towards the bottom rows, a few nearer boxes per env, a few misses; labels"""
    rng = np.random.default_rng(seed)
    d = np.broadcast_to((1.0 + 3.0 * (1.0 - np.arange(H) / max(H, 2)))[None, :, None], (N, H, W)).astype(F).copy()
    lab = np.ones((N, H, W), np.uint8)
    for e in range(N):
        for _ in range(3):
            y, x, h, w = rng.integers(0, H), rng.integers(0, W), rng.integers(1, max(H // 2, 2)), rng.integers(1, max(W // 4, 2))
            d[e, y:y + h, x:x + w] = F(rng.uniform(0.2, 1.0))
        miss = rng.random((H, W)) < 0.02
        d[e][miss], lab[e][miss] = 9.0, 0
    return d.reshape(N, -1), lab.reshape(N, -1)


# (N, width, height, env_stride, latency, frames): R = 96, 100 (no multiple of 4), 3072 and 12 601, the largest image _sizes accepts
SHAPES = [(1, 16, 6, 1, 0, 1), (257, 16, 6, 1, 1, 2), (257, 20, 5, 3, 0, 3), (3, 64, 48, 1, 2, 6), (2, 12601, 1, 1, 0, 2), (2, 101, 124, 1, 1, 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=[f"N{s[0]}_{s[1]}x{s[2]}_s{s[3]}_K{s[4] + s[5]}" for s in SHAPES])
def test_shapes_on_the_device(shape):
    N, W, H, stride, latency, frames = shape
    d, lab = random_image(N, W, H, seed=W * H + N)
    inst = np.zeros((N, 8), F)
    inst[:, 0], inst[:, 1], inst[:, 4] = np.arange(N) % (latency + 1), 1.0, np.array([0.98, 1.0, 1.02], F)[np.arange(N) % 3]
    rig = B.Rig(W, H, d, lab, None, inst, device="cuda:0", entry=_entry(), fb=2.0, window=min(W - 1, 128) if W > 1 else 1, env_stride=stride, latency=latency,
                frames=frames, max_disparity=8.0, t_hi=8.0, edge_radius=2, p_edge_hole=0.3, p_edge_cum=F(0.6), drop_value=-1.0, clip_lo=0.125, clip_hi=8.0,
                offset=4.0625, gain=0.125, period=2, stagger=1)
    lengths = np.ones(N, np.int64)
    lengths[::5] = 0
    rig.put("episode_length", lengths)
    for tick, flags in ((0, REF.FILL_ALL), (3, 0), (4, 0), (5, REF.RESETS_ONLY)):
        before, inp = rig.read(), rig.inputs()
        assert rig.launch(tick, flags) == 0
        hist, state, codes = REF.apply(before["hist"], before["state"], inp["depth"], inp["labels"], None, lengths, inst, rig.p, tick, flags)
        got = rig.read()
        assert same(got["hist"], hist) and (got["state"] == state).all(), (tick, flags)
        assert same(got["hist_pad"], before["hist_pad"])
    assert got["state"][0] > 0 and got["state"][1] > 0


def test_the_image_one_past_the_lds_limit_is_refused():
    from isaacgymloco_amd import lib
    n = ctypes.c_size_t()
    L = lib.load()
    assert L.lsim_sensor_stereo_sizes(12601, 1, ctypes.byref(n)) == 0 and n.value == 163832 <= abi.DEFINES["LSIM_STEREO_MAX_LDS_BYTES"]
    assert L.lsim_sensor_stereo_sizes(12602, 1, ctypes.byref(n)) == abi.DEFINES["LSIM_E_INVALID"]
    d, lab = random_image(1, 12601, 1, seed=1)
    rig = B.Rig(12601, 1, d, lab, device="cuda:0", entry=_entry(), fb=2.0, p_edge_hole=1.0, p_edge_cum=1.0)
    before = rig.read()

    def wider(st):
        st.width, st.depth_stride, st.hist_stride, st.label_stride = 12602, 12608, 12608, 12608      # only the image itself is at fault
    assert rig.launch(3, 0, wider) == abi.DEFINES["LSIM_E_INVALID"]
    got = rig.read()
    assert same(got["hist"], before["hist"]) and (got["state"] == before["state"]).all()


def test_two_launches_and_a_side_stream_write_the_same_bits():
    import torch
    scene = SCENES[-1]
    a, b = hip_rig(scene), hip_rig(scene)
    got_a = check(a, MODES[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got_b = check(b, MODES[1])
    assert same(got_a["hist"], got_b["hist"]) and (got_a["state"] == got_b["state"]).all()
    check(a, MODES[1])                      # the second launch on the same depth: the reference from what the first left
