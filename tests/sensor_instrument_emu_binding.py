"""TEST INFRASTRUCTURE -- builds and binds tests/emu/emu_sensor_instrument.cpp (the CPU shim of the two instrument launches,
isaacgymloco_amd/csrc/ls_sensor_instrument.h compiled by g++ under LS_EMU), and two rigs, in host memory for the shim or in device memory for
the HIP library, driven launch by launch: DrawRig, one lsim_sensor_instrument with the arrays it points to, and CaptureRig, the Rig of
tests/sensor_model_emu_binding.py with an `inst` array, whose launch() is lsim_sensor_capture_inst and whose plain() is lsim_sensor_capture."""
import ctypes

import numpy as np

import emu_binding
import sensor_model_emu_binding as SB
from helpers import abi

HEADERS = SB.HEADERS + ["ls_sensor_instrument.h"]
GUARD = 16              # floats behind the last row of `inst`, pre-filled and checked
GUARD_VALUE = np.float32(-123.5)
RANGES = ("lat_lo", "lat_hi", "gain_lo", "gain_hi", "scale_range", "quad_range", "fov_range")
NEUTRAL = dict(lat_lo=0, lat_hi=0, gain_lo=1.0, gain_hi=1.0, scale_range=0.0, quad_range=0.0, fov_range=0.0)


def lib():
    return emu_binding.load_shim("sensor_instrument", HEADERS)


def EmuApi():
    """the sensor, encoder, memory and mount-jitter shims plus this one, for envs.sensors.RaySensor(api=...); counts the sensor launches"""
    import depth_memory_emu_binding as GB
    import sensor_mount_jitter_emu_binding as MB
    return GB.EmuApi(MB.lib(), lib(), count=("lsim_raycast", "lsim_raycast_bodies", "lsim_sensor_capture", "lsim_sensor_mount_jitter",
                                             "lsim_sensor_instrument", "lsim_sensor_capture_inst"))


def neutral_rows(num_envs, latency):
    rows = np.zeros((num_envs, 8), np.float32)
    rows[:, 0], rows[:, 1], rows[:, 4] = latency, 1.0, 1.0
    return rows


class DrawRig:
    """`inst` [N, 8] starts as NaN with GUARD guard floats behind it, episode_length as 1; `ranges`: the struct's seven range fields (NEUTRAL's,
    overridden).  `device`: None -- numpy arrays and the shim -- or a torch device and `entry` = the library's lsim_sensor_instrument."""

    def __init__(self, num_envs, env_stride=1, seed=1, rank=0, stream_id=0, device=None, entry=None, **ranges):
        N = self.N = int(num_envs)
        self.device = device
        a = {"inst": emu_binding.aligned((N * 8 + GUARD,), np.float32), "episode_length": emu_binding.aligned((N,), np.int64)}
        a["inst"][:N * 8] = np.nan
        a["inst"][N * 8:] = GUARD_VALUE
        a["episode_length"][:] = 1
        if device is not None:
            import torch
            a = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in a.items()}
        self.a = a
        si = abi.LsimSensorInstrument()
        si.inst, si.episode_length = self._ptr("inst"), self._ptr("episode_length")
        si.seed, si.rank, si.stream_id, si.num_envs, si.env_stride = int(seed), int(rank), int(stream_id), N, int(env_stride)
        self.si = si
        self.set_ranges(**dict(NEUTRAL, **ranges))
        self._entry = entry if device is not None else lib().emu_sensor_instrument

    def _ptr(self, k):
        return self.a[k].data_ptr() if self.device is not None else self.a[k].ctypes.data

    def set_ranges(self, **ranges):
        """the struct's ranges, in place; `self.ranges` holds them as the struct does (fp32)"""
        for k, v in ranges.items():
            assert k in RANGES, k
            setattr(self.si, k, v)
        self.ranges = {k: getattr(self.si, k) for k in RANGES}

    def put(self, name, value):
        if self.device is not None:
            import torch
            cur = self.a[name]
            v = np.broadcast_to(np.asarray(value, dtype=self.get(name).dtype), tuple(cur.shape)).copy()
            cur.copy_(torch.from_numpy(v).to(self.device))
        else:
            self.a[name][:] = value

    def get(self, name):
        if self.device is not None:
            import torch
            torch.cuda.synchronize()
            return self.a[name].cpu().numpy().copy()
        return self.a[name].copy()

    def fill_rows(self, value=np.nan):
        m = self.get("inst")
        m[:self.N * 8] = value
        self.put("inst", m)

    def launch(self, tick, flags=0, edit=None, stream=None):
        """one launch; `edit(si)` changes a copy of the struct first; returns the entry point's value"""
        si = abi.LsimSensorInstrument.from_buffer_copy(self.si)
        si.tick, si.flags = tick, flags
        if edit:
            edit(si)
        if self.device is not None and stream is None:
            import torch
            stream = torch.cuda.current_stream().cuda_stream
        return self._entry(ctypes.byref(si), None if stream is None else ctypes.c_void_p(stream))

    def read(self):
        """(inst [N, 8], guard [GUARD]) copies"""
        m = self.get("inst")
        return m[:self.N * 8].reshape(self.N, 8), m[self.N * 8:]


class CaptureRig(SB.Rig):
    """SB.Rig plus `inst` [N, 8] (the neutral rows of the model's latency to begin with; put("inst", rows) changes them).  launch() is
    lsim_sensor_capture_inst, plain() lsim_sensor_capture on the same struct and arrays.  `device`: as SB.Rig's, with `entry` = the library
    (its two entry points are taken by name)."""

    def __init__(self, *a, device=None, entry=None, **kw):
        L = entry
        super().__init__(*a, device=device, entry=None if L is None else L.lsim_sensor_capture, **kw)
        inst = emu_binding.aligned((self.N, 8), np.float32)
        inst[:] = neutral_rows(self.N, self.p["latency"])
        if device is not None:
            import torch
            inst = torch.from_numpy(np.ascontiguousarray(inst)).to(device)
        self.a["inst"] = inst
        self._plain = self._entry
        self._inst_entry = L.lsim_sensor_capture_inst if device is not None else lib().emu_sensor_capture_inst

    def launch(self, tick, flags=0, edit=None, inst="own"):
        """one lsim_sensor_capture_inst; `edit(sm)` changes a copy of the struct first, `inst` replaces the pointer (an address or None)"""
        sm = abi.LsimSensorModel.from_buffer_copy(self.sm)
        sm.tick, sm.flags = tick, flags
        if edit:
            edit(sm)
        stream = None
        if self.device is not None:
            import torch
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        ptr = self._ptr("inst") if isinstance(inst, str) else inst
        return self._inst_entry(ctypes.byref(sm), None if ptr is None else ctypes.c_void_p(ptr), stream)

    def plain(self, tick, flags=0, edit=None):
        """one lsim_sensor_capture on the same struct"""
        return SB.Rig.launch(self, tick, flags, edit)
