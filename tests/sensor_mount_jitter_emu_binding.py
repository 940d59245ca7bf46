"""TEST INFRASTRUCTURE -- builds and binds tests/emu/emu_sensor_mount_jitter.cpp (the CPU shim of the mount-jitter launch,
isaacgymloco_amd/csrc/ls_sensor_mount_jitter.h compiled by g++ under LS_EMU), and Rig: one lsim_sensor_mount_jitter with the arrays it points
to, in host memory for the shim or in device memory for the HIP library, driven launch by launch."""
import ctypes

import numpy as np

import emu_binding
import sensor_model_emu_binding as SB
from helpers import abi

HEADERS = SB.HEADERS + ["ls_sensor_mount_jitter.h"]
GUARD = 16              # floats behind the last row of `mount`, pre-filled and checked
GUARD_VALUE = np.float32(-123.5)


def lib():
    return emu_binding.load_shim("sensor_mount_jitter", HEADERS)


def EmuApi():
    """the sensor, encoder and memory shims plus this one, for envs.sensors.RaySensor(api=...); counts the sensor launches"""
    import depth_memory_emu_binding as GB
    return GB.EmuApi(lib(), count=("lsim_raycast", "lsim_raycast_bodies", "lsim_sensor_capture", "lsim_sensor_mount_jitter"))


class Rig:
    """`nominal` [N, 7]; `mount` starts as NaN with GUARD guard floats behind it, episode_length as 1.  `device`: None -- numpy arrays and
    the shim -- or a torch device and `entry` = the library's lsim_sensor_mount_jitter."""

    def __init__(self, nominal, pos_range=(0.0, 0.0, 0.0), rot_range=(0.0, 0.0, 0.0), env_stride=1, seed=1, rank=0, stream_id=0, device=None, entry=None):
        nominal = np.ascontiguousarray(nominal, np.float32)
        N = self.N = nominal.shape[0]
        self.device = device
        a = {"nominal": emu_binding.aligned((N, 7), np.float32), "mount": emu_binding.aligned((N * 7 + GUARD,), np.float32),
             "episode_length": emu_binding.aligned((N,), np.int64)}
        a["nominal"][:] = nominal
        a["mount"][:N * 7] = np.nan
        a["mount"][N * 7:] = GUARD_VALUE
        a["episode_length"][:] = 1
        if device is not None:
            import torch
            a = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in a.items()}
        self.a = a
        mj = abi.LsimSensorMountJitter()
        mj.nominal, mj.mount, mj.episode_length = self._ptr("nominal"), self._ptr("mount"), self._ptr("episode_length")
        mj.seed, mj.rank, mj.stream_id, mj.num_envs, mj.env_stride = int(seed), int(rank), int(stream_id), N, int(env_stride)
        self.mj = mj
        self.set_ranges(pos_range, rot_range)
        self._entry = entry if device is not None else lib().emu_sensor_mount_jitter

    def _ptr(self, k):
        return self.a[k].data_ptr() if self.device is not None else self.a[k].ctypes.data

    def set_ranges(self, pos_range, rot_range):
        """the struct's ranges, in place"""
        for k in range(3):
            self.mj.pos_range[k], self.mj.rot_range[k] = float(pos_range[k]), float(rot_range[k])
        self.pos_range = np.array([self.mj.pos_range[k] for k in range(3)], np.float32)
        self.rot_range = np.array([self.mj.rot_range[k] for k in range(3)], np.float32)

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

    def fill_mount(self, value=np.nan):
        m = self.get("mount")
        m[:self.N * 7] = value
        self.put("mount", m)

    def launch(self, tick, flags=0, edit=None, stream=None):
        """one launch; `edit(mj)` changes a copy of the struct first; returns the entry point's value"""
        mj = abi.LsimSensorMountJitter.from_buffer_copy(self.mj)
        mj.tick, mj.flags = tick, flags
        if edit:
            edit(mj)
        if self.device is not None and stream is None:
            import torch
            stream = torch.cuda.current_stream().cuda_stream
        return self._entry(ctypes.byref(mj), None if stream is None else ctypes.c_void_p(stream))

    def read(self):
        """(mount [N, 7], guard [GUARD]) copies"""
        m = self.get("mount")
        return m[:self.N * 7].reshape(self.N, 7), m[self.N * 7:]
