"""GPU: the weight-gradient family of csrc/ls_learn.h -- lsim_k_linear_wgrad<NT, KT>, lsim_k_linear_wgrad_tiled<VX, VG, KG, FZ>, lsim_k_wgrad_reduce and
lsim_k_wgrad_reduce_batch -- through the C ABI at the small shapes of tests/wgrad_shapes_reference.py: all 44 (NT, KT), all 24 <VX, VG, KG, FZ>, every
tile kind, quarter and hand-over, against the fp64 numpy reference.  Exact scenes bit for bit; general scenes within 4 x the distance of the
reference's fp32 twins; grad_pre bit for bit in both.  Every launch reads operands whose unused columns and trailing rows are NaN, writes partial
results into a NaN-filled workspace of exactly the queried size, and writes its outputs between NaN guard bands."""
import ctypes

import numpy as np
import pytest
import torch

import mlp_shapes_rig as G
from launch_rig import NanDevice as _Device, bits32 as _bits32, device_lib as _lib
import wgrad_shapes_reference as R

pytestmark = pytest.mark.gpu
DEV = G.DEV
NAMES = list(R.CASES)


def _guarded_at(shape, off):
    """G.guarded with the view `off` floats behind a 16-byte boundary (a gradient-arena slice starts wherever the previous parameter ended)"""
    n = int(np.prod(shape))
    view, flat = G.guarded((n + off,))
    assert view.data_ptr() % 16 == 0
    return view[off:].view(*shape), (flat, n + off, view[:off])


def _intact(guard):
    flat, n, lead = guard
    return G.guards_intact(flat, n) and bool(torch.isnan(lead).all())


class Launch:
    """one case's buffers on the device and its calls"""

    def __init__(self, c, scene):
        self.c, self.L = c, _lib()
        x, g, z = scene
        self.host = {"x": R.padded(x, c["xo"], c["ldx"]), "g": R.padded(g, c["go"], c["ldg"])}
        if c["fz"]:
            self.host["z"] = R.padded(z, c["zo"], c["ldz"])
        self.dev = {k: torch.from_numpy(v).to(DEV) for k, v in self.host.items()}
        for k, t in self.dev.items():
            assert t.data_ptr() % 16 == 0
        self.ptr = {k: self.dev[k].data_ptr() + 4 * c[k + "o"] for k in self.dev}
        self.p = R.plan(c["batch"], c["k_in"], c["n_out"])
        nbytes, parts = ctypes.c_size_t(0), ctypes.c_int(0)
        rc = self.L.lsim_linear_wgrad_workspace(c["batch"], c["k_in"], c["n_out"], ctypes.byref(nbytes), ctypes.byref(parts))
        assert (rc, parts.value, nbytes.value) == (0, self.p["partials"], self.p["bytes"]), \
            ("the launch plan changed: re-derive the batches and classes of tests/wgrad_shapes_reference.py", c["name"], rc, parts.value, nbytes.value, self.p)
        self.ws, self.ws_flat = G.guarded((self.p["bytes"] // 4,))
        self.dw, self.dw_guard = _guarded_at((c["n_out"], c["k_in"]), c["dw_off"])
        self.db, self.db_guard = _guarded_at((c["n_out"],), 0) if c["db"] else (None, None)
        self.gy, self.gy_guard = _guarded_at((c["batch"], c["n_out"]), 0) if c["gy"] else (None, None)

    def outputs(self):
        return [t for t in (self.dw, self.db, self.gy) if t is not None]

    def args(self):
        c, ptr = self.c, (lambda t: None if t is None else t.data_ptr())
        a = [self.ptr["x"], c["ldx"], self.ptr["g"], c["ldg"]] + ([self.ptr["z"], c["ldz"]] if c["fz"] else [])
        a += [c["batch"], c["k_in"], c["n_out"], ptr(self.dw), ptr(self.db)] + ([ptr(self.gy)] if c["fz"] else [])
        return a + [self.ws.data_ptr(), self.p["bytes"], torch.cuda.current_stream().cuda_stream]

    def call(self, pending=None):
        name = R.ENTRY[self.c["entry"]]
        if pending is not None:
            return getattr(self.L, name + "_deferred")(*self.args(), ctypes.byref(pending))
        return getattr(self.L, name)(*self.args())

    def refill(self):
        for t in self.outputs() + [self.ws]:
            t.fill_(float("nan"))

    def check_memory(self):
        c = self.c
        assert G.guards_intact(self.ws_flat, self.p["bytes"] // 4), "a write outside the workspace"
        assert _intact(self.dw_guard) and (self.db is None or _intact(self.db_guard)) and (self.gy is None or _intact(self.gy_guard)), "a write outside an output"
        for k, t in self.dev.items():
            assert torch.equal(G.bits(t), G.bits(torch.from_numpy(self.host[k]).to(DEV))), "operand %s changed" % k
        used = self.p["partials"] * c["k_in"] * c["n_out"] + (self.p["partials"] * c["n_out"] if c["db"] else 0)
        assert bool(torch.isfinite(self.ws[:used]).all()), "a partial result slot nobody wrote"
        for t in self.outputs():
            assert bool(torch.isfinite(t).all()), "NaN or Inf in an output: an unwritten element, or an operand's NaN padding reached a sum"

    def run(self):
        """the immediate entry, twice: checks memory and that both calls agree to the bit -> dict(dw, db, gy) numpy"""
        assert self.call() == 0
        torch.cuda.synchronize()
        self.check_memory()
        first = [t.clone() for t in self.outputs()]
        self.refill()
        assert self.call() == 0
        torch.cuda.synchronize()
        self.check_memory()
        for a, b in zip(first, self.outputs()):
            assert torch.equal(G.bits(a), G.bits(b)), "two calls on the same inputs differ"
        get = lambda t: None if t is None else t.cpu().numpy()
        return dict(dw=get(self.dw), db=get(self.db), gy=get(self.gy))


@pytest.mark.parametrize("name", NAMES)
def test_exact_scene_bit_for_bit(name):
    """integer operands and activation factors that are multiples of 1/4: every partial sum in any order is exact in fp32, so dw, db and grad_pre
    equal the fp64 reference to the bit -- a dropped, doubled or mis-owned row, a mis-indexed column or an unsummed partial cannot hide"""
    c = R.CASES[name]
    scene = R.exact_scene(c)
    ref = R.reference(c, *scene)
    got = Launch(c, scene).run()
    assert np.array_equal(_bits32(got["dw"]), _bits32(ref["dw"])), (name, "dw", int((got["dw"] != ref["dw"]).sum()))
    if c["db"]:
        assert np.array_equal(_bits32(got["db"]), _bits32(ref["db"])), (name, "db")
    if c["gy"]:
        assert np.array_equal(got["gy"].view(np.int32), ref["gy"].view(np.int32)), (name, "grad_pre")


@pytest.mark.parametrize("name", R.GENERAL)
def test_general_scene_within_the_twins_tolerance(name):
    c = R.CASES[name]
    sc = R.general_case(name)
    got = Launch(c, (sc["x"], sc["g"], sc["z"])).run()
    for i, k in enumerate(("dw", "db")):
        if got[k] is None:
            continue
        err = float(np.abs(got[k].astype(np.float64) - sc["ref"][k]).max())
        print(name, k, "max |device - fp64|", err, "tolerance", sc["tol"][i], "twin distance", sc["twin_dist"][i])
        assert err <= sc["tol"][i], (name, k, err, sc["tol"][i])
    if c["gy"]:
        assert np.array_equal(got["gy"].view(np.int32), sc["ref"]["gy"].view(np.int32)), (name, "grad_pre")


def test_every_instantiation_is_launched():
    """the classes the case table reaches by the restated plan include every template instantiation: with the tripwire in Launch (the library's own
    partial and byte counts), a case that passes above has run the kernel its classes name"""
    got = set().union(*(R.case_classes(c) for c in R.CASES.values()))
    assert len({k for k in got if k.startswith("tiled<")}) == 24 and len({k for k in got if k.startswith("sw<")}) == 44
    assert got == R.CLASSES


def _deferred_cases():
    """26 cases of mixed kinds, the cheapest of each: more than LS_REDUCE_BATCH, so lsim_wgrad_reduce_batch splits its launch"""
    cost = lambda n: R.CASES[n]["batch"] * (R.CASES[n]["k_in"] + R.CASES[n]["n_out"])
    by = {e: sorted((n for n in NAMES if R.CASES[n]["entry"] == e and not R.plan(R.CASES[n]["batch"], R.CASES[n]["k_in"], R.CASES[n]["n_out"])["small"]), key=cost) for e in R.ENTRY}
    small = sorted((n for n in NAMES if R.plan(R.CASES[n]["batch"], R.CASES[n]["k_in"], R.CASES[n]["n_out"])["small"]), key=cost)
    picked = by["plain"][:6] + by["elu"][:7] + by["relu"][:7] + small[:3] + small[-3:]
    return [picked[(7 * i) % len(picked)] for i in range(len(picked))]        # kinds interleaved (7 and 26 are coprime)


def test_deferred_sum_equals_the_immediate_entries_bit_for_bit():
    """every *_deferred entry leaves dw / db untouched and its partial results in its own workspace; one lsim_wgrad_reduce_batch call over 26
    records (two launches) then gives the bits of the immediate entries"""
    from isaacgymloco_amd import abi
    names = _deferred_cases()
    assert len(names) == 26 > R.REDUCE_BATCH and len(set(names)) == 26 and {R.CASES[n]["entry"] for n in names} == set(R.ENTRY)
    assert any(not R.CASES[n]["db"] for n in names) and any(R.CASES[n]["dw_off"] for n in names)
    launches, want, records = [], [], (abi.LsimWgradPending * len(names))()
    for i, n in enumerate(names):
        c = R.CASES[n]
        la = Launch(c, R.exact_scene(c) if i % 2 else R.general_scene(c))
        assert la.call() == 0
        torch.cuda.synchronize()
        want.append([t.clone() for t in la.outputs()])
        la.refill()
        assert la.call(records[i]) == 0
        rec = records[i]
        assert (rec.part, rec.out, rec.num_partials, rec.count) == (la.ws.data_ptr(), la.dw.data_ptr(), la.p["partials"], c["k_in"] * c["n_out"])
        assert (rec.count2, rec.out2) == ((c["n_out"], la.db.data_ptr()) if c["db"] else (0, None))
        launches.append(la)
    torch.cuda.synchronize()
    for la in launches:
        assert bool(torch.isnan(la.dw).all()) and (la.db is None or bool(torch.isnan(la.db).all())), "dw / db hold nothing until the batched sum"
    L = _lib()
    assert L.lsim_wgrad_reduce_batch(records, 0, torch.cuda.current_stream().cuda_stream) == 0
    assert L.lsim_wgrad_reduce_batch(records, len(names), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    for n, la, w in zip(names, launches, want):
        la.check_memory()
        for a, b in zip(w, la.outputs()):
            assert torch.equal(G.bits(a), G.bits(b)), (n, "deferred and immediate sums differ")


def test_entries_refuse_before_any_launch():
    """the refusals of tests/test_wgrad_shapes.py on device buffers: the code, nothing written, no HIP error left behind.  The two alignment
    refusals use pointers 4 and 8 bytes into buffers that are large enough for the whole call"""
    from isaacgymloco_amd import abi
    L = _lib()
    for name, entry, edits, code in R.REFUSALS:
        for deferred in (None, abi.LsimWgradPending()):
            d = _Device()
            rc = R.refusal_call(L, entry, edits, d.address, deferred)
            assert rc == getattr(abi, code), (name, rc)
            assert d.untouched(), name
    # and the same shape, aligned, is accepted
    c = R._case("elu", R.REFUSAL_SHAPE["k_in"], R.REFUSAL_SHAPE["n_out"], R.REFUSAL_SHAPE["batch"])
    scene = R.exact_scene(c)
    got, ref = Launch(c, scene).run(), R.reference(c, *scene)
    assert np.array_equal(_bits32(got["dw"]), _bits32(ref["dw"])) and np.array_equal(got["gy"].view(np.int32), ref["gy"].view(np.int32))
