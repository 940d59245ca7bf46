"""GPU: the depth encoder's backward launches (lsim_depth_encode_backward, isaacgymloco_amd/csrc/ls_depth_encoder_bwd.h) on a real device: the
shape x grid_limit matrix of tests/depth_encoder_backward_emu_binding.py against the numpy fp64 reference within its derived bound
(tests/depth_encoder_backward_reference.py), repeat launches bit for bit, the sizes against the CPU build's, the argument errors, and
DepthEncoder.forward_device with torch's autograd and an Adam step around it.  Every test is a few launches on at most 48 x 64 x 2, B <= 7."""
import ctypes

import numpy as np
import pytest

import depth_encoder_backward_emu_binding as BB
import depth_encoder_backward_reference as RB
import depth_encoder_emu_binding as DB
import depth_encoder_reference as R
from helpers import abi

pytestmark = pytest.mark.gpu


def hip_kw():
    from isaacgymloco_amd import lib
    L = lib.load()
    return dict(device="cuda:0", entry=L.lsim_depth_encode_backward, sizes=L.lsim_depth_encode_backward_sizes)


@pytest.mark.parametrize("name,grid_limit", BB.MATRIX)
def test_shape_on_the_device_within_the_bound_of_the_reference(name, grid_limit):
    BB.check_shape(name, grid_limit, hip_kw())


def test_repeat_launches_are_bit_identical():
    rig = BB.make("C", hip_kw(), grid_limit=2)
    assert rig.launch() == 0
    one = rig.bits()
    for k in rig.extent:
        rig.a[k].fill_(float("nan"))
    assert rig.launch() == 0 and rig.launch() == 0          # the second of these starts from the first one's partial sums in the workspace
    two = rig.bits()
    for k in one:
        np.testing.assert_array_equal(one[k][:rig.extent[k]], two[k][:rig.extent[k]])


def test_sizes_on_the_device_library_equal_the_cpu_builds():
    from isaacgymloco_amd import lib
    L, E = lib.load(), BB.lib()
    for name in sorted(DB.SHAPES):
        rig = BB.make(name)
        for B, gl in ((1, 0), (7, 3), (300, 0), (4096, 0), (4096, 16)):
            db = abi.LsimDepthEncoderBwd.from_buffer_copy(rig.db)
            db.batch, db.grid_limit = B, gl
            dev = (ctypes.c_size_t(), ctypes.c_size_t())
            emu = (ctypes.c_size_t(), ctypes.c_size_t())
            assert L.lsim_depth_encode_backward_sizes(ctypes.byref(db), ctypes.byref(dev[0]), ctypes.byref(dev[1])) == 0
            assert E.emu_depth_encode_backward_sizes(ctypes.byref(db), ctypes.byref(emu[0]), ctypes.byref(emu[1])) == 0
            assert (dev[0].value, dev[1].value) == (emu[0].value, emu[1].value)


def test_argument_errors_leave_the_device_buffers_untouched():
    from isaacgymloco_amd import lib
    from test_depth_encoder_backward import invalid_edits
    rig = BB.make("A", hip_kw())
    assert lib.load().lsim_depth_encode_backward(None, None) == abi.E_INVALID
    before = rig.get("workspace").view(np.uint32)
    for what, edit in invalid_edits().items():
        assert rig.launch(edit) == abi.E_INVALID, what
    assert rig.untouched() and (rig.get("workspace").view(np.uint32) == before).all()


@pytest.mark.parametrize("name", ["C", "D"])
def test_forward_device_with_autograd_and_an_adam_step(name):
    """C: the default network, frames read in place; D: no final activation, height * width and the flattened length no multiples of 4, so
    the frames go through the padded copy"""
    import torch
    s, _, hist, _, _, _, _ = BB.case(name)
    act = s.get("final_act", True)
    x = DB.frames_of(s, hist).copy()
    enc = DB.module(s, 0).to("cuda:0")
    params = DB.params_of(enc)
    frames = torch.from_numpy(x).to("cuda:0")
    out = enc.forward_device(frames)
    assert out.shape == (s["N"], s["latent_dim"]) and out.requires_grad
    out.square().sum().backward()
    got = out.detach().cpu().numpy()
    want, bound = R.encode(x, params, s["s1"], s["s2"], act)
    assert (np.abs(got - want) <= bound).all()
    # d (sum of squares) / d latent = 2 * latent, exact in fp32: the reference runs on the g the launch was given
    grads, gbound, _ = RB.backward(x, params, 2.0 * got, s["s1"], s["s2"], act)
    for k, p in zip(("gw1", "gb1", "gw2", "gb2", "gw3", "gb3"), enc.device_params()):
        assert p.grad is not None and p.grad.shape == p.shape, k
        worst = float((np.abs(p.grad.cpu().numpy() - grads[k]) / gbound[k]).max())
        print(f"shape {name} through forward_device: {k} worst |difference| / bound = {worst:.2e}")
        assert worst <= 1.0, k
    torch.optim.Adam(enc.parameters(), lr=1e-2).step()
    with torch.no_grad():
        again = enc.forward_device(frames).cpu().numpy()
    assert not np.array_equal(again, got)
    want2, bound2 = R.encode(x, DB.params_of(enc), s["s1"], s["s2"], act)
    assert (np.abs(again - want2) <= bound2).all() and np.abs(want2 - want).max() > 10 * bound.max()       # the step is seen: no packing step


def test_frames_that_ask_for_a_gradient_raise():
    import torch
    s = DB.SHAPES["B"]
    enc = DB.module(s, 0).to("cuda:0")
    frames = torch.zeros(2, s["frames"], s["height"], s["width"], device="cuda:0")
    assert enc.forward_device(frames).shape == (2, s["latent_dim"])
    with pytest.raises(ValueError, match="requires_grad"):
        enc.forward_device(frames.clone().requires_grad_())
