"""TEST INFRASTRUCTURE -- builds and binds tests/emu/emu_odometry.cpp and tests/emu/emu_map_rows.cpp (the CPU shims of the two launches of
isaacgymloco_amd/csrc/ls_odometry.h compiled by g++ under LS_EMU), and their rigs: one struct with the arrays it points to, in host memory
for the shim or in device memory for the HIP library, driven launch by launch.  Every array a launch writes has guard elements behind it,
pre-filled with GUARD_VALUE and checked."""
import numpy as np

import emu_binding
from helpers import abi
from launch_rig import EditRig, LaunchRig

GUARD_VALUE = np.float32(-123.5)
EST_INITIAL = np.float32(777.0)
LsimOdometry = abi.STRUCTS["lsim_odometry_t"]
LsimMapRows = abi.STRUCTS["lsim_map_rows_t"]


def lib():
    return emu_binding.shim("odometry")


def rows_lib():
    return emu_binding.shim("map_rows")


def EmuApi():
    """the sensor, encoder, memory and map shims plus these two, for envs.sensors.RaySensor(api=...); counts the sensor launches"""
    return emu_binding.api("raycast", "raycast_bodies", "sensor_model", "depth_encoder", "depth_memory", "sensor_mount_jitter", "sensor_instrument",
                           "elevation_map", "odometry", "map_rows",
                           count=("lsim_raycast", "lsim_raycast_bodies", "lsim_sensor_capture", "lsim_sensor_capture_inst", "lsim_sensor_mount_jitter",
                                  "lsim_sensor_instrument", "lsim_elevation_map", "lsim_odometry_step", "lsim_map_rows"))


class Rig(LaunchRig):
    """N envs: `root_states` start as the identity pose at the origin, episode_length as 1, `odo` as zeros and `est` as EST_INITIAL, each
    with guard floats behind it.  `device`: None -- numpy arrays and the shim -- or a torch device and `entry` = the library's
    lsim_odometry_step."""

    def __init__(self, N, ranges=(0.0,) * 6, env_stride=1, seed=1, rank=0, stream_id=0, device=None, entry=None):
        super().__init__(device)
        self.N = int(N)
        pose = np.zeros((N, 13), np.float32)
        pose[:, 6] = 1.0
        self.add("root_states", pose)
        self.add("est", np.full((N, 13), EST_INITIAL, np.float32), guard=GUARD_VALUE)
        self.add("odo", np.zeros((N, 12), np.float32), guard=GUARD_VALUE)
        self.add("episode_length", np.ones(N, np.int64))
        od = LsimOdometry()
        self.point(od, ("root_states", "est", "odo", "episode_length"))
        od.seed, od.rank, od.stream_id, od.num_envs, od.env_stride = int(seed), int(rank), int(stream_id), self.N, int(env_stride)
        self.od = self.bind(od, entry if device is not None else lib().emu_odometry_step)
        self.set_ranges(ranges)

    def set_ranges(self, ranges):
        """the struct's six ranges (scale, yaw, z, then the three noises), in place"""
        for name, v in zip(("scale_range", "yaw_range", "z_range", "pos_noise", "yaw_noise", "z_noise"), ranges):
            setattr(self.od, name, float(v))
        self.ranges = tuple(np.float32(v) for v in ranges)

    def read(self):
        """copies (odo [N, 12], est [N, 13]); asserts both guards intact"""
        self.assert_guards()
        return self.get("odo"), self.get("est")

    def fill(self, name, value):
        self.put(name, value)


class RowsRig(EditRig):
    """N envs, P points, `channels`: scan [N, P + scan_pad], known [N, P + known_pad], pose [N, 13], rows [N, ld] with guard floats behind
    it; the padding of scan is NaN, of known 0x7E, and rows start as ROWS_INITIAL."""
    ROWS_INITIAL = np.float32(555.0)

    def __init__(self, N, P, channels, scan_pad=3, known_pad=5, ld_pad=2, env_stride=1, z_offset=0.5, scale=5.0, device=None, entry=None):
        super().__init__(device)
        self.N, self.P, self.channels = int(N), int(P), int(channels)
        self.scan_stride, self.known_stride, self.ld = P + scan_pad, P + known_pad, channels * P + ld_pad
        scan, known, pose = np.zeros((N, self.scan_stride), np.float32), np.zeros((N, self.known_stride), np.uint8), np.zeros((N, 13), np.float32)
        scan[:, P:], known[:, P:], pose[:, 6] = np.nan, 0x7E, 1.0
        self.add("scan", scan)
        self.add("known", known)
        self.add("pose", pose)
        self.add("rows", np.full((N, self.ld), self.ROWS_INITIAL, np.float32), guard=GUARD_VALUE)
        mr = LsimMapRows()
        self.point(mr, ("scan", "known", "pose", "rows"))
        mr.num_points, mr.channels, mr.scan_stride, mr.known_stride, mr.ld = self.P, self.channels, self.scan_stride, self.known_stride, self.ld
        mr.num_envs, mr.env_stride, mr.z_offset, mr.scale = self.N, int(env_stride), float(z_offset), float(scale)
        self.mr = self.bind(mr, entry if device is not None else rows_lib().emu_map_rows)

    def read(self):
        """copy of rows [N, ld]; asserts the guard intact"""
        self.assert_guards()
        return self.get("rows")
