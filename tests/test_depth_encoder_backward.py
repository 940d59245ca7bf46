"""CPU: the depth encoder's backward source (isaacgymloco_amd/csrc/ls_depth_encoder_bwd.h) compiled by g++ under LS_EMU, against the numpy fp64
reference of tests/depth_encoder_backward_reference.py (written from include/lsim.h; its docstring derives the per-entry error bound), and
that reference against torch's fp64 autograd of DepthEncoder.forward.  The same shapes x grid_limit matrix runs on the HIP launches in
tests/test_gpu_depth_encoder_backward.py."""
import ctypes

import numpy as np
import pytest
import torch

import depth_encoder_backward_emu_binding as BB
import depth_encoder_backward_reference as RB
import depth_encoder_emu_binding as DB
from helpers import abi


@pytest.mark.parametrize("name", sorted(DB.SHAPES))
def test_reference_equals_torch_autograd_in_fp64(name):
    """pins the layouts and the flatten order of the header's formulas to torch's"""
    s, params, hist, g, want, _, _ = BB.case(name)
    mod = DB.module(s, 0).double()
    out = mod(torch.from_numpy(DB.frames_of(s, hist).copy()).double())
    (out * torch.from_numpy(g.copy()).double()).sum().backward()
    for k, p in zip(("gw1", "gb1", "gw2", "gb2", "gw3", "gb3"), mod.device_params()):
        got = p.grad.numpy()
        assert got.shape == want[k].shape
        assert np.abs(got - want[k]).max() <= 1e-12 * max(1.0, np.abs(want[k]).max()), k


def test_the_bound_is_tight_enough_to_see_a_wrong_da1():
    """conditions on the test's own inputs (shape A), not measurements of the code under test: ky / kx of w2 swapped in the da1 step only"""
    s, params, hist, g, want, bound, _ = BB.case("A")
    wrong, _, _ = RB.backward(DB.frames_of(s, hist), params, g, s["s1"], s["s2"], True, swap_w2_in_da1=True)
    missed = np.abs(wrong["gw1"] - want["gw1"]) > bound["gw1"]
    print(f"w2 with ky / kx swapped in da1: {100 * missed.mean():.1f} % of gw1's entries miss the bound")
    assert missed.mean() > 0.5
    for k in ("gw2", "gb2", "gw3", "gb3"):
        assert (wrong[k] == want[k]).all()


@pytest.mark.parametrize("name", sorted(DB.SHAPES))
def test_largest_bound_relative_to_rms(name):
    _, _, _, _, want, bound, _ = BB.case(name)
    rel = {k: float(bound[k].max() / np.sqrt((want[k] ** 2).mean())) for k in RB.NAMES}
    print(f"shape {name}: largest bound / rms of the gradient = " + ", ".join(f"{k} {v:.2e}" for k, v in rel.items()))
    assert all(np.isfinite(bound[k]).all() and (bound[k] > 0).all() for k in RB.NAMES)


@pytest.mark.parametrize("name,grid_limit", BB.MATRIX)
def test_shim_within_the_bound_of_the_reference(name, grid_limit):
    BB.check_shape(name, grid_limit)


def test_sample_split():
    """A's seven samples over three workgroups: three, two and two"""
    rig = BB.make("A", grid_limit=3)
    assert rig.launch() == 0
    s = rig.shape
    # the plan is the header's: read it back through _sizes at two grid limits (the partial sums scale with the workgroups)
    NP = s["c1"] * s["frames"] * s["k1"] ** 2 + s["c1"] + s["c2"] * s["c1"] * s["k2"] ** 2 + s["c2"]

    def ws(gl):
        db = abi.LsimDepthEncoderBwd.from_buffer_copy(rig.db)
        db.grid_limit = gl
        return rig.sizes(db)[1]

    assert ws(3) - ws(2) == 4 * NP and ws(2) - ws(1) == 4 * NP
    L = BB.lib()
    assert [(L.emu_deb_first(k, 7, 3), L.emu_deb_count(k, 7, 3)) for k in range(3)] == [(0, 3), (3, 2), (5, 2)]
    for B, G in ((1, 1), (8, 3), (4096, 256), (4097, 256), (300, 256)):
        spans = [(L.emu_deb_first(k, B, G), L.emu_deb_count(k, B, G)) for k in range(G)]
        assert spans[0][0] == 0 and all(a + n == b for (a, n), (b, _) in zip(spans, spans[1:])) and sum(spans[-1]) == B
        assert max(n for _, n in spans) - min(n for _, n in spans) <= 1 and min(n for _, n in spans) >= 1


def test_sizes():
    rig = BB.make("C")
    db = abi.LsimDepthEncoderBwd.from_buffer_copy(rig.db)
    lds, ws = rig.sizes(db)
    args = lds - 4 * (2 * 48 * 64 + 16 * 22 * 30 + 32 * 10 * 14 + 64 + (2 * 25 + 16 * 9 + 22 * 30 + 10 * 14 + 3) // 4 * 4)
    assert 0 < args <= 512 and lds <= abi.DEFINES["LSIM_DEPTH_ENC_MAX_LDS_BYTES"]           # the planned regions plus the launch's own arguments
    # requirement (a): the workspace grows with B by the a2 and dz rows only -- nothing of the size of a1
    row = 4 * (32 * 10 * 14 + 64)
    prev = None
    for B in (1, 2, 3, 7, 255, 256, 257, 4096, 4097):
        db.batch = B
        n = rig.sizes(db)[1]
        if prev is not None:
            assert 0 <= n - prev[1] <= row * (B - prev[0]) + 12, (B, n, prev)
        prev = (B, n)
    db.batch = 4096
    assert rig.sizes(db)[1] < 4096 * row + (32 << 20) + 16 and rig.sizes(db)[1] < 4 * 4096 * 16 * 22 * 30
    L = BB.lib()
    a, b = ctypes.c_size_t(7), ctypes.c_size_t(7)
    for edit in (("batch", 0), ("grid_limit", -1), ("height", 200), ("k2", 0)):
        bad = abi.LsimDepthEncoderBwd.from_buffer_copy(rig.db)
        setattr(bad, *edit)
        assert L.emu_depth_encode_backward_sizes(ctypes.byref(bad), ctypes.byref(a), ctypes.byref(b)) == abi.E_INVALID and (a.value, b.value) == (7, 7)
    assert L.emu_depth_encode_backward_sizes(None, ctypes.byref(a), ctypes.byref(b)) == abi.E_INVALID
    assert L.emu_depth_encode_backward_sizes(ctypes.byref(rig.db), None, ctypes.byref(b)) == abi.E_INVALID
    assert L.emu_depth_encode_backward_sizes(ctypes.byref(rig.db), ctypes.byref(a), None) == abi.E_INVALID


def invalid_edits():
    """{what: edit(db)} of every argument error include/lsim.h lists for lsim_depth_encode_backward (shape A)"""
    def f(name, value):
        return lambda db: setattr(db, name, value)

    def off(name, by):
        return lambda db: setattr(db, name, getattr(db, name) + by)

    edits = {"batch 0": f("batch", 0), "batch < 0": f("batch", -3), "grid_limit < 0": f("grid_limit", -1), "workspace short": off("workspace_bytes", -4),
             "frames > slots": f("frames", 4), "frames 0": f("frames", 0), "slots 9": f("hist_slots", 9),
             "H * W > hist_stride": f("hist_stride", 220), "hist_stride odd": f("hist_stride", 222), "height 0": f("height", 0), "width 0": f("width", 0),
             "k1 > height": f("k1", 14), "k1 > 8": f("k1", 9), "k1 0": f("k1", 0), "s1 0": f("s1", 0), "s1 5": f("s1", 5), "c1 0": f("c1", 0), "c1 65": f("c1", 65),
             "k2 > h1": f("k2", 7), "k2 0": f("k2", 0), "s2 0": f("s2", 0), "s2 5": f("s2", 5), "c2 0": f("c2", 0), "c2 65": f("c2", 65),
             "latent_dim 0": f("latent_dim", 0), "latent_dim 257": f("latent_dim", 257), "final_act 2": f("final_act", 2),
             "g_stride short": f("g_stride", 32), "latent_stride short": f("latent_stride", 32),
             "hist misaligned": off("hist", 8), "workspace misaligned": off("workspace", 8)}
    ptrs = BB.PARAMS + ("g", "latent") + tuple("g" + p for p in BB.PARAMS)
    for p in ("hist", "workspace") + ptrs:
        edits[p + " NULL"] = f(p, None)
    for p in ptrs:
        edits[p + " misaligned"] = off(p, 2)
    return edits


def test_every_invalid_argument_is_refused_and_nothing_is_written():
    rig = BB.make("A")
    assert BB.lib().emu_depth_encode_backward(None, None) == abi.E_INVALID
    before = rig.get("workspace").view(np.uint32)
    for what, edit in invalid_edits().items():
        assert rig.launch(edit) == abi.E_INVALID, what
        assert rig.untouched() and (rig.get("workspace").view(np.uint32) == before).all(), what
    # the limits themselves are accepted
    assert rig.launch(lambda db: setattr(db, "grid_limit", 1000)) == 0 and rig.launch(lambda db: setattr(db, "g_stride", 33)) == 0
    big = dict(DB.SHAPES["B"], latent_dim=256)
    params, hist = DB.params_of(DB.module(big)), DB.images(big)
    g = np.ones((big["N"], 256), np.float32)
    assert BB.Rig(big, params, hist, g, g).launch() == 0


@pytest.mark.parametrize("grid_limit", (0, 2))
def test_two_calls_are_bit_identical_and_parameters_are_read_per_call(grid_limit):
    rig = BB.make("A", grid_limit=grid_limit)
    assert rig.launch() == 0
    one = rig.bits()
    for k in rig.extent:
        rig.put(k, np.array([BB.Rig.PREFILL], np.uint32).view(np.float32)[0])
    assert rig.launch() == 0
    two = rig.bits()
    for k in one:
        np.testing.assert_array_equal(one[k], two[k])
    w2 = rig.get("w2")
    w2[3, 1, 2, 0] += 0.25
    rig.put("w2", w2)
    assert rig.launch() == 0
    three = rig.grads()
    first = {k: one[k][:rig.extent[k]].view(np.float32) for k in one}
    assert (three["gw1"].ravel() != first["gw1"]).mean() > 0.5 and (three["gb1"].ravel() != first["gb1"]).any()
    np.testing.assert_array_equal(three["gb3"].ravel(), first["gb3"])           # dz does not depend on w2


def test_forward_device_needs_the_entry_point():
    from isaacgymloco_amd import lib as L
    enc = DB.module(DB.SHAPES["B"])
    frames = torch.zeros(2, 1, 12, 16)

    class Old:
        """a library from before the backward pass"""
        lsim_depth_encode = lsim_depth_encode_sizes = staticmethod(lambda *a: 0)

    with pytest.raises(L.LsimError, match="lsim_depth_encode_backward"):
        enc.forward_device(frames, api=Old())

    class New(Old):
        lsim_depth_encode_backward = lsim_depth_encode_backward_sizes = staticmethod(lambda *a: 0)

    with pytest.raises(ValueError, match="requires_grad"):
        enc.forward_device(frames.clone().requires_grad_(), api=New())
