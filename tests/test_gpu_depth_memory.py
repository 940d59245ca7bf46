"""GPU: the depth-memory launches (lsim_depth_memory_step, lsim_gru_sequence_forward / _backward, isaacgymloco_amd/csrc/ls_depth_memory.h) on a real
device: the shapes and checks of tests/depth_memory_emu_binding.py against the numpy fp64 reference within its bounds
(tests/depth_memory_reference.py), again after an in-place weight change, on a non-default stream, and DepthMemory.sequence_device under
autograd next to the torch loop.  Every GPU step is one or two launches."""
import numpy as np
import pytest

import depth_memory_emu_binding as MB
import depth_memory_reference as R

pytestmark = pytest.mark.gpu


def hip_step_rig(*a, **kw):
    from isaacgymloco_amd import lib
    return MB.StepRig(*a, device="cuda:0", entry=lib.load().lsim_depth_memory_step, **kw)


def hip_seq_rig(*a, **kw):
    from isaacgymloco_amd import lib
    L = lib.load()
    return MB.SeqRig(*a, device="cuda:0", entries=(L.lsim_gru_sequence_forward, L.lsim_gru_sequence_backward), **kw)


@pytest.mark.parametrize("name", sorted(MB.SHAPES))
def test_step_on_the_device_within_the_bound_and_after_a_weight_change(name):
    MB.check_step(name, hip_step_rig, weight_edit=MB.scale_weights)


@pytest.mark.parametrize("name", sorted(MB.SHAPES))
def test_sequence_on_the_device_within_the_bounds(name):
    MB.check_sequence(name, hip_seq_rig)


def test_sequence_after_an_in_place_weight_change():
    """W_hh is read where it is at every launch: scaled in place, the next forward follows the new weights"""
    s, c = MB.SHAPES["B"], MB.sequence_case("B")
    rig = hip_seq_rig(s, c["prm"], c["gi"], c["h0"], c["reset"], c["dhs"])
    prm = list(c["prm"])
    prm[1] = (prm[1] * np.float32(-1.5)).astype(np.float32)
    import torch
    rig.a["weight_hh"][:prm[1].size].mul_(-1.5)
    assert rig.forward() == 0
    want = R.sequence(c["gi"], c["h0"], c["reset"], prm)
    got = rig.get("hs")
    assert (np.abs(got - want["hs"]) <= want["e_hs"]).all()
    assert (np.abs(got - c["fwd"]["hs"]) > c["fwd"]["e_hs"]).any()


def test_launches_on_a_non_default_stream():
    import torch
    s = MB.SHAPES["B"]
    prm, z, p, h, el = MB.step_case(s)
    rig = hip_step_rig(s, prm, z, p, h, el)
    c = MB.sequence_case("B")
    seq = hip_seq_rig(s, c["prm"], c["gi"], c["h0"], c["reset"], c["dhs"])
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert rig.launch(0, stream=side) == 0 and seq.forward(stream=side) == 0 and seq.backward(stream=side) == 0
    side.synchronize()
    want, bound = R.step(z, p, h, el == 0, prm)
    assert (np.abs(rig.h() - want) <= bound).all() and rig.guards_intact()
    assert (np.abs(seq.get("hs") - c["fwd"]["hs"]) <= c["fwd"]["e_hs"]).all()
    assert np.abs(seq.get("dgi") - c["bwd"]["dgi"]).max() <= c["tol"]["dgi"] and seq.guards_intact()


def test_sequence_device_gradients_against_the_reference():
    """DepthMemory.sequence_device under autograd: hs within the bound (gi formed by the library GEMM: its error is part of the bound), the four
    parameter gradients and dh0 within 4 x the distance of the torch fp32 loop on the same device from the fp64 reference"""
    import torch
    from isaacgymloco_amd.learn.depth_memory import DepthMemory
    s, c = MB.SHAPES["B"], MB.sequence_case("B")
    mem = DepthMemory(s["L"], s["P"], s["H"]).to("cuda:0")
    with torch.no_grad():
        for p, v in zip(mem.device_params(), c["prm"]):
            p.copy_(torch.from_numpy(v))
    x, reset = torch.from_numpy(c["x"]).cuda(), torch.from_numpy(c["reset"]).cuda()
    dhs = torch.from_numpy(c["dhs"]).cuda()
    gi, e_gi, s_gi = R.project(c["x"], c["prm"])
    fwd = R.sequence(gi, c["h0"], c["reset"], c["prm"], e_gi, s_gi)
    want = R.param_grads(c["x"], fwd, R.backward(c["dhs"], fwd, c["h0"], c["reset"], c["prm"]), c["h0"], c["reset"])
    grads = {}
    for which in ("sequence", "sequence_device"):
        mem.zero_grad()
        h0 = torch.from_numpy(c["h0"]).cuda().requires_grad_()
        hs = getattr(mem, which)(x, h0, reset)
        if which == "sequence_device":
            assert (np.abs(hs.detach().cpu().numpy() - fwd["hs"]) <= fwd["e_hs"]).all()
        (hs * dhs).sum().backward()
        grads[which] = [p.grad.cpu().numpy().astype(np.float64) for p in mem.device_params()] + [h0.grad.cpu().numpy().astype(np.float64)]
    want = list(want) + [R.backward(c["dhs"], fwd, c["h0"], c["reset"], c["prm"])["dh0"]]
    for k, (w, twin, got) in enumerate(zip(want, grads["sequence"], grads["sequence_device"])):
        dist = np.abs(twin - w).max()
        print(f"gradient {k}: torch loop distance {dist:.3e}, sequence_device distance {np.abs(got - w).max():.3e}")
        assert np.abs(got - w).max() <= 4 * dist
