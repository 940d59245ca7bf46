"""GPU: lsim_k_linear_fwd<TM, TN, BK, VX, VW, ACT> (csrc/ls_gemm.h) through lsim_linear_elu_forward and lsim_linear_masked_forward of the C ABI, at the
small shapes of tests/fwd_gemm_reference.py built for THIS device's CU count: both tile configs and both epilogues under every source class of the
operand loads, every tile count from 1 to a few more than the grid and the persistent walk of two and three tiles, against the fp64 numpy statement.
Exact scenes bit for bit (the ELU's negative side within the exponential's derived bound); general scenes within 4 x the distance of the statement's
fp32 twins.  Every launch reads operands whose unused columns and trailing rows are NaN and writes between NaN guard bands into rows whose columns
n_out .. ldo are NaN and must stay so."""
import numpy as np
import pytest
import torch

import fwd_gemm_reference as R
import mlp_shapes_rig as G
from launch_rig import NanDevice as _Device, bits32 as _bits32, device_lib as _lib

pytestmark = pytest.mark.gpu
DEV = G.DEV
KEYS = list(R.by_key(256))
GENERAL_KEYS = [c["key"] for c in R.cases(256).values() if c["general"] and c["name"] in R.GENERAL]


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _case(key):
    return R.by_key(_cus())[key]


def _flat_w(W, off):
    flat = np.full(off + W.size + 8, np.nan, dtype=np.float32)
    flat[off:off + W.size] = W.reshape(-1)
    return flat


class Launch:
    """one case's buffers on the device and its call"""

    def __init__(self, c, scene):
        self.c, self.L = c, _lib()
        x, W, b, mask = scene
        self.host = {"x": R.padded(x, c["xo"], c["ldx"]), "w": _flat_w(W, c["wo"])}
        off = {"x": c["xo"], "w": c["wo"]}
        if b is not None:
            self.host["b"], off["b"] = _flat_w(b, 4), 4
        if mask is not None:
            self.host["mask"], off["mask"] = R.padded(mask, 0, c["ldm"]), 0
        self.dev = {k: torch.from_numpy(v).to(DEV) for k, v in self.host.items()}
        for t in self.dev.values():
            assert t.data_ptr() % 16 == 0
        self.ptr = {k: self.dev[k].data_ptr() + 4 * off[k] for k in self.dev}
        self.out, self.flat = G.guarded((c["batch"], c["ldo"]))
        assert self.out.data_ptr() % 16 == 0

    def call(self):
        c, s = self.c, torch.cuda.current_stream().cuda_stream
        if c["act"] == "elu":
            return self.L.lsim_linear_elu_forward(self.ptr["x"], c["ldx"], self.ptr["w"], self.ptr.get("b"), c["batch"], c["k_in"], c["n_out"], self.out.data_ptr(), c["ldo"], s)
        return self.L.lsim_linear_masked_forward(self.ptr["x"], c["ldx"], self.ptr["w"], self.ptr["mask"], c["ldm"], c["batch"], c["k_in"], c["n_out"], self.out.data_ptr(),
                                                 c["ldo"], s)

    def check_memory(self):
        c = self.c
        assert G.guards_intact(self.flat, c["batch"] * c["ldo"]), "a write outside out"
        assert bool(torch.isnan(self.out[:, c["n_out"]:]).all()), "a write into the columns between n_out and ldo"
        assert bool(torch.isfinite(self.out[:, :c["n_out"]]).all()), "NaN or Inf in out: an unwritten element, or an operand's NaN padding reached a sum"
        for k, t in self.dev.items():
            assert torch.equal(G.bits(t), G.bits(torch.from_numpy(self.host[k]).to(DEV))), "operand %s changed" % k

    def run(self):
        """the entry twice: checks memory and that both calls agree to the bit -> out [batch, n_out] numpy"""
        assert self.call() == 0
        torch.cuda.synchronize()
        self.check_memory()
        first = self.out.clone()
        self.out.fill_(float("nan"))
        assert self.call() == 0
        torch.cuda.synchronize()
        self.check_memory()
        assert torch.equal(G.bits(first), G.bits(self.out)), "two calls on the same inputs differ"
        return self.out[:, :self.c["n_out"]].cpu().numpy()


@pytest.mark.parametrize("key", KEYS)
def test_exact_scene(key):
    """small-integer operands: every partial sum in any order is exact in fp32.  The masked product equals the statement bit for bit, element for
    element, and a masked-out element is the bit pattern of +0.0; the ELU equals it bit for bit where the pre-activation is positive, is 0 where it
    is exactly 0, exactly -1 from -30 down, and within the exponential's derived bound (1.17e-7) in between"""
    c = _case(key)
    p = R.case_plan(c, _cus())
    scene = R.exact_scene(c)
    ref = R.reference(c, *scene)
    got = Launch(c, scene).run()
    if c["act"] == "mask":
        bad = got.view(np.int32) != _bits32(ref["out"])
        assert not bad.any(), (c["name"], int(bad.sum()), "mismatches")
        assert (got.view(np.int32)[~(scene[3] > 0)] == 0).all()
        return
    pos, zero, sat = ref["pre"] > 0, ref["pre"] == 0, ref["pre"] <= -30
    assert np.array_equal(got[pos].view(np.int32), _bits32(ref["out"][pos])), (c["name"], "positive side")
    assert (got[zero].view(np.int32) == 0).all(), (c["name"], "elu(0) is not +0.0")
    assert (got[sat] == -1.0).all(), (c["name"], "saturated side")
    mid = ~pos & ~zero
    err = float(np.abs(got[mid].astype(np.float64) - ref["out"][mid]).max())
    print("fwd exact", c["name"], p["config"], "launched %d%d" % (p["launched"], p["launched"]), "tiles", p["total"], "blocks", p["blocks"],
          "elu negative side: max |device - fp64|", err, "bound", R.ELU_BOUND)
    assert err <= R.ELU_BOUND, (c["name"], err)


@pytest.mark.parametrize("key", GENERAL_KEYS)
def test_general_scene_within_the_twins_tolerance(key):
    c = _case(key)
    p = R.case_plan(c, _cus())
    g = R.general_case(c["name"])
    got = Launch(c, g["scene"]).run()
    err = np.abs(got.astype(np.float64) - g["ref"]["out"])
    if c["act"] == "mask":
        assert (got.view(np.int32)[~(g["scene"][3] > 0)] == 0).all(), (c["name"], "a masked-out element is not +0.0")
    ratio = float((err / g["tol"]).max())
    print("fwd general", c["name"], p["config"], c["act"], "launched %d%d" % (p["launched"], p["launched"]), "twin distance", g["twin_dist"], "tolerance", g["base"],
          "max |device - fp64|", float(err.max()), "device / tolerance", ratio)
    assert ratio <= 1.0, (c["name"], float(err.max()), g["base"])


def test_the_table_reaches_every_class_on_this_device():
    cus = _cus()
    got = set().union(*(R.case_classes(c, cus) for c in R.cases(cus).values()))
    assert R.classes() <= got, sorted(R.classes() - got)


def test_entries_refuse_before_any_launch():
    from isaacgymloco_amd import abi
    L = _lib()
    for name, entry, edits, code in R.REFUSALS:
        d = _Device()
        rc = R.refusal_call(L, entry, edits, d.address)
        assert rc == getattr(abi, code), (name, entry, rc)
        assert d.untouched(), (name, entry)
    # and the same shape, unedited, is accepted
    for act in ("elu", "mask"):
        c = R._case(act, R.REFUSAL_SHAPE["k_in"], R.REFUSAL_SHAPE["n_out"], R.REFUSAL_SHAPE["batch"], "22")
        scene = R.exact_scene(c)
        got, ref = Launch(c, scene).run(), R.reference(c, *scene)
        keep = ref["pre"] > 0 if act == "elu" else np.ones_like(ref["pre"], dtype=bool)
        assert np.array_equal(got[keep].view(np.int32), _bits32(ref["out"][keep]))
