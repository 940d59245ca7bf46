"""The depth-memory launches on the CPU: tests/emu/emu_depth_memory.cpp (ls_depth_memory.h's own validation, plan, tile split and index arithmetic
under LS_EMU) against the numpy fp64 reference and its error bound; the reference against torch; the argument checks through the shim and
through the HIP library (which refuses before any HIP call, so without a device)."""
import ctypes

import numpy as np
import pytest
import torch

import depth_memory_emu_binding as MB
import depth_memory_reference as R
from helpers import abi

SHAPES = sorted(MB.SHAPES)


def _torch_cell(s, prm, dtype):
    cell = torch.nn.GRUCell(s["L"] + s["P"], s["H"]).to(dtype)
    with torch.no_grad():
        for p, v in zip((cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh), prm):
            p.copy_(torch.tensor(v, dtype=dtype))
    return cell


@pytest.mark.parametrize("name", ["A", "B"])
def test_reference_agrees_with_torch_fp64_forward_and_autograd(name):
    """layout and gate order: the fp64 forward and the analytic backward against autograd through an nn.GRUCell loop"""
    s, c = MB.SHAPES[name], MB.sequence_case(name)
    cell = _torch_cell(s, c["prm"], torch.float64)
    x = torch.tensor(c["x"], dtype=torch.float64)
    h0 = torch.tensor(c["h0"], dtype=torch.float64, requires_grad=True)
    keep = torch.tensor(c["reset"] == 0, dtype=torch.float64)
    gi, e_gi, s_gi = R.project(c["x"], c["prm"])
    fwd = R.sequence(gi, c["h0"], c["reset"], c["prm"], e_gi, s_gi)
    h, hs = h0, []
    for t in range(s["T"]):
        h = cell(x[t], h * keep[t][:, None])
        hs.append(h)
    hs = torch.stack(hs)
    np.testing.assert_allclose(hs.detach().numpy(), fwd["hs"], rtol=0, atol=1e-12)
    (hs * torch.tensor(c["dhs"], dtype=torch.float64)).sum().backward()
    bwd = R.backward(c["dhs"], fwd, c["h0"], c["reset"], c["prm"])
    got = R.param_grads(c["x"], fwd, bwd, c["h0"], c["reset"])
    for a, b in zip(got, (cell.weight_ih.grad, cell.weight_hh.grad, cell.bias_ih.grad, cell.bias_hh.grad)):
        np.testing.assert_allclose(a, b.numpy(), rtol=0, atol=1e-10)
    np.testing.assert_allclose(bwd["dh0"], h0.grad.numpy(), rtol=0, atol=1e-12)


def test_step_reference_agrees_with_torch_and_its_bound_covers_torch_fp32():
    s = MB.SHAPES["B"]
    prm, z, p, h, el = MB.step_case(s)
    want, bound = R.step(z, p, h, el == 0, prm)
    x = np.concatenate((z, p), axis=1)
    hp = h * (el != 0)[:, None]
    got64 = _torch_cell(s, prm, torch.float64)(torch.tensor(x, dtype=torch.float64), torch.tensor(hp, dtype=torch.float64)).detach().numpy()
    np.testing.assert_allclose(got64, want, rtol=0, atol=1e-13)
    got32 = _torch_cell(s, prm, torch.float32)(torch.tensor(x), torch.tensor(hp)).detach().numpy()
    assert (np.abs(got32 - want) <= bound).all()


@pytest.mark.parametrize("mutant", ["swap", "inside"])
def test_the_bound_sees_a_wrong_cell(mutant):
    """r / z blocks swapped, and W_hn (r * h) in place of r * (W_hn h + b_hn): each misses the bound by more than 10 x on most outputs of shape A"""
    s = MB.SHAPES["A"]
    prm, z, p, h, el = MB.step_case(s)
    fresh = np.zeros(s["N"], bool)                  # with h_prev = 0 the second mutant IS the cell: every env carries a state here
    want, bound = R.step(z, p, h, fresh, prm)
    wrong, _ = R.step(z, p, h, fresh, prm, mutant=mutant)
    assert (np.abs(wrong - want) > 10 * bound).mean() > 0.5
    c = MB.sequence_case("A")
    wrong = R.sequence(c["gi"], c["h0"], c["reset"], c["prm"], mutant=mutant)["hs"]
    assert (np.abs(wrong - c["fwd"]["hs"]) > 10 * c["fwd"]["e_hs"]).mean() > 0.5


@pytest.mark.parametrize("name", SHAPES)
def test_step_shapes_through_the_shim(name):
    MB.check_step(name, MB.StepRig, weight_edit=MB.scale_weights)


@pytest.mark.parametrize("name", SHAPES)
def test_sequence_shapes_through_the_shim(name):
    MB.check_sequence(name, MB.SeqRig)


def test_sizes_accept_the_required_cells_and_refuse_the_rest():
    from isaacgymloco_amd import lib
    for L in (MB.lib().emu_depth_memory_sizes, lib.load().lsim_depth_memory_sizes):
        a, b, c = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        for H in (16, 32, 48, 64, 80, 96):
            assert L(H, 109, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0, H
            assert a.value == 4 * 16 * (112 + 2 + H + 2) and b.value == 4 * (3 * H + 32) * (H + 2) and c.value == 4 * (H + 32) * (3 * H + 2)
            assert max(a.value, b.value, c.value) <= abi.DEFINES["LSIM_GRU_MAX_LDS_BYTES"]
        assert L(64, 512, ctypes.byref(a), None, None) == 0 and L(64, 1, None, None, None) == 0
        a.value = 7
        for H, I in ((0, 8), (8, 8), (24, 8), (112, 8), (128, 8), (144, 8), (-16, 8), (64, 0), (64, 513)):
            assert L(H, I, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == abi.E_INVALID and a.value == 7, (H, I)


def _step_edits():
    f = lambda name, value: (lambda d: setattr(d, name, value))
    off = lambda name, by: (lambda d: setattr(d, name, getattr(d, name) + by))
    edits = {"flag 4": f("flags", 4), "both flags": f("flags", 3), "num_envs 0": f("num_envs", 0), "latent_dim 0": f("latent_dim", 0),
             "proprio_dim < 0": f("proprio_dim", -1), "I > 512": f("proprio_dim", 508), "latent_dim huge": f("latent_dim", 2 ** 31 - 1),
             "hidden 0": f("hidden", 0), "hidden 24": f("hidden", 24), "hidden 112": f("hidden", 112), "hidden 128": f("hidden", 128), "hidden 144": f("hidden", 144),
             "z_ld short": f("z_ld", 4), "p_ld short": f("p_ld", 2), "h_ld short": f("h_ld", 15), "rows_ld short": f("rows_ld", 20),
             "episode_length misaligned": off("episode_length", 4), "P > 0 without p": f("p", None)}
    for p in ("z", "episode_length", "weight_ih", "weight_hh", "bias_ih", "bias_hh", "h"):
        edits[p + " NULL"] = f(p, None)
    for p in ("z", "p", "h", "rows", "weight_ih", "weight_hh", "bias_ih", "bias_hh"):
        edits[p + " misaligned"] = off(p, 2)
    return edits


def _sequence_edits():
    f = lambda name, value: (lambda d: setattr(d, name, value))
    off = lambda name, by: (lambda d: setattr(d, name, getattr(d, name) + by))
    both = {"steps 0": f("steps", 0), "num_envs 0": f("num_envs", 0), "hidden 8": f("hidden", 8), "hidden 112": f("hidden", 112), "hidden 128": f("hidden", 128),
            "reset NULL": f("reset", None), "h0 NULL": f("h0", None), "hs NULL": f("hs", None), "weight_hh NULL": f("weight_hh", None),
            "h0 misaligned": off("h0", 4), "hs misaligned": off("hs", 8), "weight_hh misaligned": off("weight_hh", 2), "save misaligned": off("save", 4)}
    fwd = dict(both, **{"gi NULL": f("gi", None), "gi misaligned": off("gi", 4), "bias_hh NULL": f("bias_hh", None), "bias_hh misaligned": off("bias_hh", 2)})
    bwd = dict(both, **{"save NULL": f("save", None), "dhs NULL": f("dhs", None), "dgi NULL": f("dgi", None), "dghn NULL": f("dghn", None),
                        "dhs misaligned": off("dhs", 4), "dgi misaligned": off("dgi", 8), "dghn misaligned": off("dghn", 4), "dh0 misaligned": off("dh0", 4)})
    return fwd, bwd


@pytest.mark.parametrize("through", ["shim", "library"])
def test_every_invalid_argument_is_refused_and_nothing_is_written(through):
    """through the shim, and through the HIP library on host pointers: it returns LSIM_E_INVALID before any HIP call, so no device is needed"""
    from isaacgymloco_amd import lib
    s = MB.SHAPES["A"]
    if through == "shim":
        L = MB.lib()
        step, fwd, bwd = L.emu_depth_memory_step, L.emu_gru_sequence_forward, L.emu_gru_sequence_backward
    else:
        L = lib.load()
        step, fwd, bwd = L.lsim_depth_memory_step, L.lsim_gru_sequence_forward, L.lsim_gru_sequence_backward
    rig = MB.StepRig(s, *MB.step_case(s))
    before = rig.outputs_bits()
    assert step(None, None) == abi.E_INVALID
    for what, edit in _step_edits().items():
        dm = MB.LsimDepthMemory.from_buffer_copy(rig.dm)
        edit(dm)
        assert step(ctypes.byref(dm), None) == abi.E_INVALID, what
    np.testing.assert_array_equal(rig.outputs_bits(), before)
    c = MB.sequence_case("A")
    seq = MB.SeqRig(s, c["prm"], c["gi"], c["h0"], c["reset"], c["dhs"])
    before = seq.output_bits()
    e_fwd, e_bwd = _sequence_edits()
    for fn, edits in ((fwd, e_fwd), (bwd, e_bwd)):
        assert fn(None, None) == abi.E_INVALID
        for what, edit in edits.items():
            gs = MB.LsimGruSequence.from_buffer_copy(seq.gs)
            edit(gs)
            assert fn(ctypes.byref(gs), None) == abi.E_INVALID, what
    np.testing.assert_array_equal(seq.output_bits(), before)
    if through == "shim":       # the limits themselves are accepted
        assert rig.launch(MB.FILL_ALL) == 0 and rig.launch(MB.RESETS_ONLY) == 0
        assert rig.launch(0, lambda d: setattr(d, "rows_ld", s["L"] + s["H"])) == 0
