"""TEST INFRASTRUCTURE -- builds and binds tests/emu/emu_odometry.cpp and tests/emu/emu_map_rows.cpp (the CPU shims of the two launches of
isaacgymloco_amd/csrc/ls_odometry.h compiled by g++ under LS_EMU), and their rigs: one struct with the arrays it points to, in host memory
for the shim or in device memory for the HIP library, driven launch by launch.  Every array a launch writes has GUARD elements behind it,
pre-filled and checked."""
import ctypes

import numpy as np

import emu_binding
import sensor_model_emu_binding as SB
from helpers import abi

HEADERS = SB.HEADERS + ["ls_odometry.h"]
GUARD = 16
GUARD_VALUE = np.float32(-123.5)
EST_INITIAL = np.float32(777.0)
LsimOdometry = abi.STRUCTS["lsim_odometry_t"]
LsimMapRows = abi.STRUCTS["lsim_map_rows_t"]


def lib():
    return emu_binding.load_shim("odometry", HEADERS)


def rows_lib():
    return emu_binding.load_shim("map_rows", HEADERS)


def EmuApi():
    """the sensor, encoder, memory and map shims plus these two, for envs.sensors.RaySensor(api=...); counts the sensor launches"""
    import depth_memory_emu_binding as GB
    import elevation_map_emu_binding as EB
    import sensor_instrument_emu_binding as IB
    import sensor_mount_jitter_emu_binding as MB
    return GB.EmuApi(MB.lib(), IB.lib(), EB.lib(), lib(), rows_lib(),
                     count=("lsim_raycast", "lsim_raycast_bodies", "lsim_sensor_capture", "lsim_sensor_capture_inst", "lsim_sensor_mount_jitter",
                            "lsim_sensor_instrument", "lsim_elevation_map", "lsim_odometry_step", "lsim_map_rows"))


class _Arrays:
    def _ptr(self, k):
        return self.a[k].data_ptr() if self.device is not None else self.a[k].ctypes.data

    def _to_device(self):
        if self.device is not None:
            import torch
            self.a = {k: torch.from_numpy(np.ascontiguousarray(v)).to(self.device) for k, v in self.a.items()}

    def put(self, name, value):
        cur = self.get(name)
        cur[...] = np.asarray(value, dtype=cur.dtype)
        if self.device is not None:
            import torch
            self.a[name].copy_(torch.from_numpy(cur).to(self.device))
        else:
            self.a[name][...] = cur

    def get(self, name):
        if self.device is not None:
            import torch
            torch.cuda.synchronize()
            return self.a[name].cpu().numpy().copy()
        return self.a[name].copy()

    def _stream(self, stream):
        if self.device is not None and stream is None:
            import torch
            stream = torch.cuda.current_stream().cuda_stream
        return None if stream is None else ctypes.c_void_p(stream)


class Rig(_Arrays):
    """N envs: `root_states` start as the identity pose at the origin, episode_length as 1, `odo` as zeros and `est` as EST_INITIAL, each
    with GUARD guard floats behind it.  `device`: None -- numpy arrays and the shim -- or a torch device and `entry` = the library's
    lsim_odometry_step."""

    def __init__(self, N, ranges=(0.0,) * 6, env_stride=1, seed=1, rank=0, stream_id=0, device=None, entry=None):
        self.N, self.device = int(N), device
        al = emu_binding.aligned
        a = {"root_states": al((N, 13), np.float32), "est": al((N * 13 + GUARD,), np.float32), "odo": al((N * 12 + GUARD,), np.float32),
             "episode_length": al((N,), np.int64)}
        a["root_states"][:, 6] = 1.0
        a["est"][:N * 13] = EST_INITIAL
        a["est"][N * 13:] = GUARD_VALUE
        a["odo"][N * 12:] = GUARD_VALUE
        a["episode_length"][:] = 1
        self.a = a
        self._to_device()
        od = LsimOdometry()
        od.root_states, od.est, od.odo, od.episode_length = (self._ptr(k) for k in ("root_states", "est", "odo", "episode_length"))
        od.seed, od.rank, od.stream_id, od.num_envs, od.env_stride = int(seed), int(rank), int(stream_id), self.N, int(env_stride)
        self.od = od
        self.set_ranges(ranges)
        self._entry = entry if device is not None else lib().emu_odometry_step

    def set_ranges(self, ranges):
        """the struct's six ranges (scale, yaw, z, then the three noises), in place"""
        for name, v in zip(("scale_range", "yaw_range", "z_range", "pos_noise", "yaw_noise", "z_noise"), ranges):
            setattr(self.od, name, float(v))
        self.ranges = tuple(np.float32(v) for v in ranges)

    def launch(self, tick, flags=0, edit=None, stream=None):
        """one launch; `edit(od)` changes a copy of the struct first; returns the entry point's value"""
        od = LsimOdometry.from_buffer_copy(self.od)
        od.tick, od.flags = tick, flags
        if edit:
            edit(od)
        return self._entry(ctypes.byref(od), self._stream(stream))

    def read(self):
        """copies (odo [N, 12], est [N, 13]); asserts both guards intact"""
        odo, est = self.get("odo"), self.get("est")
        assert (odo[self.N * 12:] == GUARD_VALUE).all() and (est[self.N * 13:] == GUARD_VALUE).all(), "a guard was overwritten"
        return odo[:self.N * 12].reshape(self.N, 12), est[:self.N * 13].reshape(self.N, 13)

    def fill(self, name, value):
        v = self.get(name)
        v[:self.N * (12 if name == "odo" else 13)] = value
        self.put(name, v)


class RowsRig(_Arrays):
    """N envs, P points, `channels`: scan [N, P + scan_pad], known [N, P + known_pad], pose [N, 13], rows [N, ld] with GUARD floats behind
    it; the padding of scan is NaN, of known 0x7E, and rows start as ROWS_INITIAL."""
    ROWS_INITIAL = np.float32(555.0)

    def __init__(self, N, P, channels, scan_pad=3, known_pad=5, ld_pad=2, env_stride=1, z_offset=0.5, scale=5.0, device=None, entry=None):
        self.N, self.P, self.channels, self.device = int(N), int(P), int(channels), device
        self.scan_stride, self.known_stride, self.ld = P + scan_pad, P + known_pad, channels * P + ld_pad
        al = emu_binding.aligned
        a = {"scan": al((N, self.scan_stride), np.float32), "known": al((N, self.known_stride), np.uint8), "pose": al((N, 13), np.float32),
             "rows": al((N * self.ld + GUARD,), np.float32)}
        a["scan"][:, P:] = np.nan
        a["known"][:, P:] = 0x7E
        a["pose"][:, 6] = 1.0
        a["rows"][:N * self.ld] = self.ROWS_INITIAL
        a["rows"][N * self.ld:] = GUARD_VALUE
        self.a = a
        self._to_device()
        mr = LsimMapRows()
        mr.scan, mr.known, mr.pose, mr.rows = (self._ptr(k) for k in ("scan", "known", "pose", "rows"))
        mr.num_points, mr.channels, mr.scan_stride, mr.known_stride, mr.ld = self.P, self.channels, self.scan_stride, self.known_stride, self.ld
        mr.num_envs, mr.env_stride, mr.z_offset, mr.scale = self.N, int(env_stride), float(z_offset), float(scale)
        self.mr = mr
        self._entry = entry if device is not None else rows_lib().emu_map_rows

    def launch(self, edit=None, stream=None):
        mr = LsimMapRows.from_buffer_copy(self.mr)
        if edit:
            edit(mr)
        return self._entry(ctypes.byref(mr), self._stream(stream))

    def read(self):
        """copy of rows [N, ld]; asserts the guard intact"""
        r = self.get("rows")
        assert (r[self.N * self.ld:] == GUARD_VALUE).all(), "the guard of rows was overwritten"
        return r[:self.N * self.ld].reshape(self.N, self.ld)
