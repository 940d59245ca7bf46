"""TEST INFRASTRUCTURE -- builds and binds the CPU shims of tests/emu (the kernel sources compiled by g++ under LS_EMU): the lane emulator of
kernels A / B (emu_lsim.cpp) and the shims of the single launches (emu_eval.cpp, emu_raycast.cpp, emu_raycast_bodies.cpp).  A shim exports
emu_<name> with the signature include/lsim.h declares for lsim_<name>, so abi.bind types it from the header."""
import ctypes
import os
import subprocess

import numpy as np

from helpers import ROOT, abi

CSRC = os.path.join(ROOT, "isaacgymloco_amd", "csrc")
_NP = {abi.DT_F32: np.float32, abi.DT_I64: np.int64, abi.DT_U8: np.uint8, abi.DT_I32: np.int32, abi.DT_I16: np.int16}
_shims = {}
_SENSOR = ["ls_raycast.h", "ls_raycast_bodies.h", "ls_sensor_model.h", "ls_math.h"]
# shim name (tests/emu/emu_<name>.cpp) -> the headers of csrc it is rebuilt for
SHIMS = {
    "raycast": ["ls_raycast.h"], "raycast_bodies": ["ls_raycast.h", "ls_raycast_bodies.h"], "sensor_model": _SENSOR,
    "eval": ["ls_eval.h"], "eval_columns": ["ls_eval.h", "ls_eval_columns.h"], "distill": ["ls_distill.h"],
    **{name: _SENSOR + [f"ls_{name}.h"] for name in ("sensor_stereo", "sensor_instrument", "sensor_mount_jitter", "elevation_map", "odometry",
                                                      "frames_log", "depth_encoder", "depth_memory")},
    "map_rows": _SENSOR + ["ls_odometry.h"], "depth_encoder_backward": _SENSOR + ["ls_depth_encoder.h", "ls_depth_encoder_bwd.h"],
    "elevation_fuse": _SENSOR + ["ls_elevation_map.h", "ls_odometry.h", "ls_elevation_fuse.h"],
}


def build_shim(src, out, deps, defines=()):
    """g++ `src` into the shared library `out` unless it is newer than `src`, `deps` and include/lsim.h"""
    deps = [src, os.path.join(ROOT, "include", "lsim.h")] + list(deps)
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas"] +
                              ["-D" + d for d in defines] + ["-o", out, src])
    return out


def load_shim(what, headers, counters=False):
    """tests/emu/emu_<what>.cpp (depends on csrc/`headers`) built and bound, cached: every emu_<name> it exports for a declared lsim_<name>
    is typed from the header.  `counters`: the -DLS_RAYCAST_COUNTERS variant, a library of its own"""
    if (what, counters) not in _shims:
        out = os.path.join(ROOT, "tests", "_build", f"lib{what}_emu{'_counters' if counters else ''}.so")
        L = ctypes.CDLL(build_shim(os.path.join(ROOT, "tests", "emu", f"emu_{what}.cpp"), out, [os.path.join(CSRC, h) for h in headers],
                                   ("LS_RAYCAST_COUNTERS",) if counters else ()))
        _shims[what, counters] = abi.bind(L, "emu", [n for n in abi.PROTOTYPES if hasattr(L, "emu" + n[len("lsim"):])])
        if hasattr(L, "emu_sizeof_config"):
            abi.check_abi(L, prefix="emu")
    return _shims[what, counters]


def shim(name, counters=False):
    """the shim `name` of SHIMS, built and bound"""
    return load_shim(name, SHIMS[name], counters)


def api(*shims, count=()):
    """EmuApi of exactly the named shims of SHIMS (or libraries already loaded), in that order; counts the calls of the names in `count`"""
    return EmuApi(*(shim(s) if isinstance(s, str) else s for s in shims), count=count)


def lib():
    return load_shim("lsim", [f for f in os.listdir(CSRC) if f.endswith(".h")] + ["../../include/lsim_layout.h"])


def aligned(shape, dtype, align=64):
    """zeroed numpy array whose data pointer is `align`-byte aligned"""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    raw = np.zeros(n + align, np.uint8)
    off = (-raw.ctypes.data) % align
    return raw[off:off + n].view(dtype).reshape(shape)


class EmuApi:
    """lsim_<name> for every declared entry point that one of the shim libraries `libs` exports as emu_<name>, with the library's
    signatures (streams ignored): what LeggedRobot, learn.evaluate.Evaluator(api=...) and envs.sensors.RaySensor(api=...) call.
    `.calls[name]` counts the calls of each name in `count`"""

    def __init__(self, *libs, count=()):
        self.calls = {name: 0 for name in count}
        for L in libs:
            for name in abi.PROTOTYPES:
                fn = getattr(L, "emu" + name[len("lsim"):], None)
                if fn is not None:
                    setattr(self, name, self._counted(name, fn) if name in self.calls else fn)

    def _counted(self, name, fn):
        def call(*a):
            self.calls[name] += 1
            return fn(*a)
        return call


class EmuSim:
    def __init__(self, cfg, model, height_grid=None, terrain_origins=None):
        L = lib()
        self.cfg = cfg
        self._h = ctypes.c_void_p()
        gp = op = None
        if height_grid is not None:
            self._g = np.ascontiguousarray(height_grid, np.int16)
            self._o = np.ascontiguousarray(terrain_origins, np.float32)
            gp, op = self._g.ctypes.data_as(ctypes.c_void_p), self._o.ctypes.data_as(ctypes.c_void_p)
        rc = L.emu_create(ctypes.byref(cfg), ctypes.byref(model), gp, op, None, 0, ctypes.byref(self._h))
        assert rc == 0, rc
        self.buf = {}
        for name, bid in abi.BUFFER_IDS.items():
            ptr, shape, nd, dt = ctypes.c_void_p(), (ctypes.c_int64 * 4)(), ctypes.c_int(), ctypes.c_int()
            assert L.emu_get_buffer(self._h, bid, ctypes.byref(ptr), shape, ctypes.byref(nd), ctypes.byref(dt)) == 0
            shp = tuple(shape[i] for i in range(nd.value))
            npdt = np.dtype(_NP[dt.value])
            raw = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint8)), shape=(int(np.prod(shp)) * npdt.itemsize,))
            self.buf[name] = raw.view(npdt).reshape(shp)

    def step(self, actions, flags=0):
        a = np.ascontiguousarray(actions, np.float32)
        assert lib().emu_step_ex(self._h, a.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(flags), None) == 0

    def reset_all(self):
        assert lib().emu_reset_all(self._h, None) == 0

    def reset_envs(self, mask):
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        assert lib().emu_reset_envs(self._h, m.ctypes.data_as(ctypes.c_void_p), None) == 0

    @property
    def stats_row(self):
        v = ctypes.c_int()
        lib().emu_get_stats_row(self._h, ctypes.byref(v))
        return v.value

    @property
    def step_counter(self):
        v = ctypes.c_int64()
        lib().emu_get_step_counter(self._h, ctypes.byref(v))
        return v.value

    @step_counter.setter
    def step_counter(self, v):
        lib().emu_set_step_counter(self._h, ctypes.c_int64(v))
