"""GPU: the second half of csrc/ls_amp.h through the C ABI at the small shapes of tests/amp_update_reference.py -- lsim_relu_head_backward and
lsim_masked_colsum at every admitted width and the batches around one pass of the row lanes, one slice and the floor of the rows per slice;
lsim_running_moments_update against a longdouble reference within a derived bound; lsim_amp_pair_rows bit for bit against a numpy float32 twin.
Every launch reads operands whose padding is NaN, writes between NaN guard bands, gets a NaN-filled workspace of exactly the queried size, leaves its
operands unchanged to the bit and repeats its bits on a second call."""
import ctypes

import numpy as np
import pytest
import torch

import amp_update_reference as R
import mlp_shapes_rig as G
from launch_rig import NanDevice as _Device, bits32 as _bits32, current_stream as _stream, device_lib as _lib

pytestmark = pytest.mark.gpu
DEV = G.DEV


def _up(flat):
    t = torch.from_numpy(flat).to(DEV)
    assert t.data_ptr() % 16 == 0
    return t


def _same(t, flat):
    return torch.equal(G.bits(t) if t.dtype == torch.float32 else t.view(torch.int64), G.bits(_up(flat)) if flat.dtype == np.float32 else _up(flat).view(torch.int64))


def _workspace(c):
    p = R.colk_plan(c["batch"], c["n"])
    need = ctypes.c_size_t(0)
    rc = _lib().lsim_relu_cols_workspace(c["batch"], c["n"], ctypes.byref(need))
    assert (rc, need.value) == (0, p["bytes"]), ("the launch plan changed: re-derive the batches of tests/amp_update_reference.py", c["name"], rc, need.value, p)
    return G.guarded((p["bytes"] // 4,)), p


def _head(c, scene):
    """lsim_relu_head_backward twice -> (grad_pre, grad_bias, grad_head) numpy"""
    L = _lib()
    a, gd, w3 = scene
    B, n = c["batch"], c["n"]
    host = {"a": R.padded(a, 0, c["ld"]), "gd": np.concatenate([gd, np.full(4, np.nan, dtype=np.float32)]), "w3": np.concatenate([w3, np.full(4, np.nan, dtype=np.float32)])}
    dev = {k: _up(v) for k, v in host.items()}
    (ws, wflat), p = _workspace(c)
    outs = [G.guarded((B, n)), G.guarded((n,)), G.guarded((n + 4,))]

    def call():
        rc = L.lsim_relu_head_backward(dev["a"].data_ptr(), c["ld"], dev["gd"].data_ptr(), dev["w3"].data_ptr(), B, n, outs[0][0].data_ptr(), outs[1][0].data_ptr(),
                                       outs[2][0].data_ptr(), ws.data_ptr(), p["bytes"], _stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert G.guards_intact(wflat, p["bytes"] // 4), "a write outside the workspace"
        for (t, flat), cnt in zip(outs, (B * n, n, n + 4)):
            assert G.guards_intact(flat, cnt), "a write outside an output"
            assert bool(torch.isfinite(t).all()), "an unwritten output element, or NaN padding in a sum"
        assert bool(torch.isfinite(ws).all()), "a partial row nobody wrote"
        for k in dev:
            assert _same(dev[k], host[k]), "operand %s changed" % k
        return [t.clone() for t, _ in outs]

    first = call()
    for t, _ in outs:
        t.fill_(float("nan"))
    ws.fill_(float("nan"))
    for x, y in zip(first, call()):
        assert torch.equal(G.bits(x), G.bits(y)), "two calls on the same inputs differ"
    return [t.cpu().numpy() for t in first]


def _colsum(c, scene):
    L = _lib()
    v, m = scene
    B, n = c["batch"], c["n"]
    host = {"v": R.padded(v, 0, c["ldv"]), "m": R.padded(m, 0, c["ldm"])}
    dev = {k: _up(x) for k, x in host.items()}
    (ws, wflat), p = _workspace(c)
    used = p["slices"] * n
    out, oflat = G.guarded((n,))

    def call():
        rc = L.lsim_masked_colsum(dev["v"].data_ptr(), c["ldv"], dev["m"].data_ptr(), c["ldm"], B, n, out.data_ptr(), ws.data_ptr(), p["bytes"], _stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert G.guards_intact(wflat, p["bytes"] // 4) and G.guards_intact(oflat, n), "a write outside the workspace or out"
        assert bool(torch.isfinite(out).all()), "NaN in out: the NaN under a non-positive mask (or the padding) reached a sum"
        assert bool(torch.isfinite(ws[:used]).all()) and bool(torch.isnan(ws[used:]).all()), "the partial rows: [slices, n] and nothing behind them"
        for k in dev:
            assert _same(dev[k], host[k]), "operand %s changed" % k
        return out.clone()

    first = call()
    out.fill_(float("nan"))
    ws.fill_(float("nan"))
    assert torch.equal(G.bits(first), G.bits(call())), "two calls on the same inputs differ"
    return first.cpu().numpy()


@pytest.mark.parametrize("name", list(R.COLK_CASES))
def test_relu_head_backward(name):
    """exact scene: grad_pre, grad_bias and grad_head bit for bit (+0.0 and -0.0 in relu_out count as masked); general scene: grad_pre bit for bit -- one
    product per element -- and the three column sums within 4 x the twins' distance"""
    c = R.COLK_CASES[name]
    n = c["n"]
    sc = R.head_scene(c, True)
    ref = R.head_reference(*sc)
    g2, db2, dh = _head(c, sc)
    assert np.array_equal(g2.view(np.int32), ref["g2"].view(np.int32)), (name, "grad_pre")
    assert np.array_equal(_bits32(db2), _bits32(ref["db2"])) and np.array_equal(_bits32(dh[:n + 1]), _bits32(ref["dhead"][:n + 1])), name
    assert (dh[n + 1:].view(np.int32) == 0).all(), (name, "grad_head[n + 1 .. n + 3]")
    sc = R.head_scene(c, False)
    ref = R.head_reference(*sc)
    g2, db2, dh = _head(c, sc)
    assert np.array_equal(g2.view(np.int32), ref["g2"].view(np.int32)), (name, "grad_pre, general scene")
    assert (dh[n + 1:].view(np.int32) == 0).all()
    for vals, want, got, out in zip(R.head_addends(sc[0], sc[1], ref), (ref["db2"], ref["dhead"][:n], ref["dhead"][n:n + 1]), (db2, dh[:n], dh[n:n + 1]),
                                    ("grad_bias", "d_head_weight", "d_head_bias")):
        tol, dist = R.twin_tolerance(vals, want, c)
        err = float(np.abs(got.astype(np.float64) - want).max())
        print("head", name, out, "twin distance", dist, "tolerance", tol, "max |device - fp64|", err, "device / tolerance", err / tol if tol else 0.0,
              "scale", float(np.abs(want).max()))
        assert err <= tol, (name, out, err, tol)


@pytest.mark.parametrize("name", list(R.COLK_CASES))
def test_masked_colsum(name):
    """v is NaN exactly where mask_src is not positive (+0.0, -0.0, negatives): the sums stay finite because the kernel selects"""
    c = R.COLK_CASES[name]
    sc = R.colsum_scene(c, True)
    assert np.array_equal(_bits32(_colsum(c, sc)), _bits32(R.colsum_reference(*sc))), name
    v, m = sc = R.colsum_scene(c, False)
    want = R.colsum_reference(v, m)
    tol, dist = R.twin_tolerance(np.where(m > 0, v, np.float32(0)), want, c)
    err = float(np.abs(_colsum(c, sc).astype(np.float64) - want).max())
    print("colsum", name, "out", "twin distance", dist, "tolerance", tol, "max |device - fp64|", err, "device / tolerance", err / tol if tol else 0.0,
          "scale", float(np.abs(want).max()))
    assert err <= tol, (name, err, tol)


def test_column_entries_refuse_before_any_launch():
    from isaacgymloco_amd import abi
    L = _lib()
    for name, entry, edits, code in R.COLK_REFUSALS:
        d = _Device()
        rc = R.colk_refusal_call(L, entry, edits, d.address)
        assert rc == getattr(abi, code), (name, entry, rc)
        assert d.untouched(), (name, entry)


# ---- running moments ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.MOM_CASES))
def test_running_moments(name):
    """three updates in a row on one state, each within the derived bound of the longdouble reference; the count is count + n exactly; the merged
    variance is never negative (constant columns); workspace slots beyond the slices in use stay untouched"""
    L = _lib()
    c = R.MOM_CASES[name]
    xs, state, kinds = R.mom_scene(c)
    need = ctypes.c_size_t(0)
    assert L.lsim_running_moments_workspace(ctypes.byref(need)) == 0
    ws, wflat = G.guarded((need.value // 8,), dtype=torch.float64)
    dev = [G.guarded((c["dim"],), dtype=torch.float64), G.guarded((c["dim"],), dtype=torch.float64), G.guarded((1,), dtype=torch.float64)]
    for (t, _), s in zip(dev, state):
        t.copy_(torch.from_numpy(s))
    ref, err, count = state, None, state[2][0]
    p = R.mom_plan(c["batch"])
    for i, x in enumerate(xs):
        ws.fill_(float("nan"))
        host = R.padded(x, 0, c["ldx"])
        xd = _up(host)
        rc = L.lsim_running_moments_update(xd.data_ptr(), c["ldx"], c["batch"], c["dim"], dev[0][0].data_ptr(), dev[1][0].data_ptr(), dev[2][0].data_ptr(), ws.data_ptr(),
                                           need.value, _stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert G.guards_intact(wflat, need.value // 8) and all(G.guards_intact(f, t.numel()) for t, f in dev), "a write outside the workspace or the state"
        assert _same(xd, host), "x changed"
        slots = ws.view(R.MOM_SLICES, 2, R.MOM_MAX_DIM)
        assert bool(torch.isfinite(slots[:p["slices"], :, :c["dim"]]).all()) and bool(torch.isnan(slots[p["slices"]:]).all()) and bool(torch.isnan(slots[:, :, c["dim"]:]).all())
        ref, err = R.mom_reference(x, ref, err)
        count = count + float(c["batch"])
        mean, var, cnt = (t.cpu().numpy() for t, _ in dev)
        dm, dv = np.abs(mean - ref[0].astype(np.float64)), np.abs(var - ref[1].astype(np.float64))
        print("moments", name, "update", i, "mean: device distance", dm.max(), "bound", err[0].max(), "| var: device distance", dv.max(), "bound", err[1].max(),
              "| largest distance / bound", max((dm / err[0]).max(), (dv / err[1]).max()))
        assert (dm <= err[0]).all() and (dv <= err[1]).all(), name
        assert cnt[0] == count and (var >= 0).all()
        for j, k in enumerate(kinds):
            if k in R.CONSTANTS and k != "const98765.43":
                assert var[j] + R.NORMALIZER_EPS > 0
            if k in R.CONSTANTS and c["start"] == "count0":
                assert abs(var[j]) <= err[1][j], (name, k, var[j])


def test_running_moments_refuses_dim_65():
    from isaacgymloco_amd import abi
    L = _lib()
    d = _Device()
    x, mean, var, count = d.address(5 * 68), d.address(136), d.address(136), d.address(4)
    ws = d.address(R.MOM_SLICES * 2 * R.MOM_MAX_DIM * 2)
    assert L.lsim_running_moments_update(x, 68, 5, 65, mean, var, count, ws, R.MOM_SLICES * 2 * R.MOM_MAX_DIM * 8, _stream()) == abi.E_UNSUPPORTED
    assert d.untouched()


# ---- pair rows -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.PAIR_CASES))
def test_amp_pair_rows(name):
    """normalised and identity forms, three different pitches: bit for bit the float32 twin; the columns between 2 dim and ld_out are left alone"""
    from isaacgymloco_amd import abi
    L = _lib()
    c = R.PAIR_CASES[name]
    B, D = c["batch"], c["dim"]
    s, ns, mean, var = R.pair_scene(c)
    host = {"s": R.padded(s, 0, c["lds"]), "ns": R.padded(ns, 0, c["ldn"])}
    dev = {k: _up(v) for k, v in host.items()}
    md, vd = torch.from_numpy(mean).to(DEV), torch.from_numpy(var).to(DEV)
    out, oflat = G.guarded((B, c["ldo"]))
    for norm in (True, False):
        want = R.pair_twin(s, ns, mean, var) if norm else np.concatenate([s, ns], axis=1)
        got = []
        for _ in range(2):
            out.fill_(float("nan"))
            rc = L.lsim_amp_pair_rows(dev["s"].data_ptr(), c["lds"], dev["ns"].data_ptr(), c["ldn"], md.data_ptr() if norm else None, vd.data_ptr() if norm else None,
                                      R.PAIR_EPS, R.PAIR_CLIP, B, D, out.data_ptr(), c["ldo"], _stream())
            assert rc == 0, rc
            torch.cuda.synchronize()
            assert G.guards_intact(oflat, B * c["ldo"]) and bool(torch.isnan(out[:, 2 * D:]).all()), "a write outside the 2 dim columns of a row"
            for k in dev:
                assert _same(dev[k], host[k]), "operand %s changed" % k
            got.append(out[:, :2 * D].cpu().numpy())
        assert np.array_equal(got[0].view(np.int32), got[1].view(np.int32))
        bad = got[0].view(np.int32) != want.view(np.int32)
        assert not bad.any(), (name, "normalised" if norm else "identity", int(bad.sum()), "elements differ from the float32 twin")
    out.fill_(float("nan"))
    assert L.lsim_amp_pair_rows(dev["s"].data_ptr(), c["lds"], dev["ns"].data_ptr(), c["ldn"], md.data_ptr(), None, R.PAIR_EPS, R.PAIR_CLIP, B, D, out.data_ptr(), c["ldo"],
                                _stream()) == abi.E_INVALID
    assert L.lsim_amp_pair_rows(dev["s"].data_ptr(), c["lds"], dev["ns"].data_ptr(), c["ldn"], None, vd.data_ptr(), R.PAIR_EPS, R.PAIR_CLIP, B, D, out.data_ptr(), c["ldo"],
                                _stream()) == abi.E_INVALID
    torch.cuda.synchronize()
    assert bool(torch.isnan(oflat).all())
