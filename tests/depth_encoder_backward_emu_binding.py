"""TEST INFRASTRUCTURE -- builds and binds tests/emu/emu_depth_encoder_backward.cpp (the CPU shim of lsim_depth_encode_backward,
isaacgymloco_amd/csrc/ls_depth_encoder_bwd.h compiled by g++ under LS_EMU), and Rig: one lsim_depth_encoder_bwd_t with the arrays it points
to, in host memory for the shim or in device memory for the HIP library.  Shapes, modules and images are depth_encoder_emu_binding's; B is
the shape's N, every row live."""
import ctypes
import functools

import numpy as np

import depth_encoder_backward_reference as RB
import depth_encoder_emu_binding as DB
import emu_binding
from helpers import abi
from launch_rig import EditRig

PARAMS = ("w1", "b1", "w2", "b2", "w3", "b3")
# (shape, grid_limit): 0 = the kernel's own choice (one workgroup per sample at these batches), 2 = several samples per workgroup; A's seven
# samples at 3 = workgroups of three, two and two
MATRIX = [(n, gl) for n in sorted(DB.SHAPES) for gl in (0, 2)] + [("A", 3)]


def lib():
    return emu_binding.shim("depth_encoder_backward")


@functools.lru_cache(maxsize=None)
def case(name, seed=0):
    """(shape, params, hist, g, gradients, bounds, latent fp32) of shape `name`: computed once, shared, never written to"""
    s = DB.SHAPES[name]
    params, hist = DB.params_of(DB.module(s, seed)), DB.images(s, seed + 1)
    g = np.random.default_rng(seed + 2).standard_normal((s["N"], s["latent_dim"])).astype(np.float32)
    grads, bounds, lat = RB.backward(DB.frames_of(s, hist), params, g, s["s1"], s["s2"], s.get("final_act", True))
    for a in list(params) + [hist, g] + list(grads.values()) + list(bounds.values()):
        a.setflags(write=False)
    return s, params, hist, g, grads, bounds, lat.astype(np.float32)


class Rig(EditRig):
    """`shape`: an entry of SHAPES; `params`: (w1 .. b3) numpy; `hist`: images(shape); g [B, L]; latent [B, L] fp32.  `device`: None -- numpy
    arrays and the shim -- or a torch device with `entry` / `sizes` = the library's two functions.  The six gradient buffers start as NaN with
    the bit pattern PREFILL, each with guard words behind it that no launch may touch; the workspace has the size of grid_limit 0, the largest."""
    PREFILL = 0x7FC00ABC

    def __init__(self, shape, params, hist, g, latent, device=None, entry=None, sizes=None, grid_limit=0):
        s = self.shape = shape
        super().__init__(device)
        self.B, self.L = s["N"], s["latent_dim"]
        self.gstride, self.lstride = self.L + 3, (self.L + 3) // 4 * 4 + 4
        for k, v in zip(PARAMS, params):
            self.add(k, np.asarray(v, np.float32))
        self.add("hist", np.asarray(hist, np.float32))
        for k, v, ld in (("g", g, self.gstride), ("latent", latent, self.lstride)):
            rows = np.zeros((self.B, ld), np.float32)
            rows[:, :self.L] = v
            self.add(k, rows)
        self.extent = {"g" + k: int(np.prod(v.shape)) for k, v in zip(PARAMS, params)}
        for k, v in zip(PARAMS, params):
            self.add("g" + k, np.full(v.shape, self.PREFILL, np.uint32).view(np.float32), guard=True)
        db = abi.LsimDepthEncoderBwd()
        db.hist_stride, db.hist_slots, db.batch = hist.shape[2], hist.shape[1], self.B
        for k in ("height", "width", "frames", "c1", "k1", "s1", "c2", "k2", "s2", "latent_dim"):
            setattr(db, k, s[k])
        db.final_act, db.g_stride, db.latent_stride, db.grid_limit = int(s.get("final_act", True)), self.gstride, self.lstride, 0
        self._sizes = sizes if device is not None else lib().emu_depth_encode_backward_sizes
        self.lds_bytes, need = self.sizes(db)
        self.add("workspace", np.zeros(need // 4, np.float32), guard=True)
        self.point(db, list(self.a))
        db.workspace_bytes, db.grid_limit = need, grid_limit
        self.db = self.bind(db, entry if device is not None else lib().emu_depth_encode_backward)

    def sizes(self, db):
        lds, ws = ctypes.c_size_t(), ctypes.c_size_t()
        assert self._sizes(ctypes.byref(db), ctypes.byref(lds), ctypes.byref(ws)) == 0
        return lds.value, ws.value

    def bits(self):
        """{name: uint32 [extent + guard]} of the six gradient buffers, guard included"""
        return {k: self.raw(k).view(np.uint32) for k in self.extent}

    def untouched(self):
        return self.guards_intact() and all((b[:self.extent[k]] == self.PREFILL).all() for k, b in self.bits().items())

    def grads(self):
        """{name: fp32 array of the parameter's shape}; asserts that every guard word still holds its pattern"""
        self.assert_guards()
        return {k: self.get(k) for k in self.extent}


def make(name, cls_kw=None, grid_limit=0):
    s, params, hist, g, _, _, lat = case(name)
    return Rig(s, params, hist, g, lat, grid_limit=grid_limit, **(cls_kw or {}))


def check_shape(name, grid_limit, cls_kw=None):
    """shape `name` at `grid_limit` against the reference within its bound, every buffer fully overwritten at exactly its extent; returns
    {gradient: worst |difference| / bound}"""
    _, _, _, _, want, bound, _ = case(name)
    rig = make(name, cls_kw, grid_limit)
    assert rig.untouched()
    assert rig.launch() == 0
    got, worst = rig.grads(), {}
    for k in RB.NAMES:
        assert np.isfinite(got[k]).all(), f"{k}: an entry still holds the NaN pre-fill"
        worst[k] = float((np.abs(got[k] - want[k]) / bound[k]).max())
    print(f"shape {name}, grid_limit {grid_limit}: worst |difference| / bound = " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    return worst
