"""TEST INFRASTRUCTURE -- builds and binds tests/emu/emu_sensor_mount_jitter.cpp (the CPU shim of the mount-jitter launch,
isaacgymloco_amd/csrc/ls_sensor_mount_jitter.h compiled by g++ under LS_EMU), and Rig: one lsim_sensor_mount_jitter with the arrays it points
to, in host memory for the shim or in device memory for the HIP library, driven launch by launch."""
import numpy as np

import emu_binding
from helpers import abi
from launch_rig import LaunchRig

GUARD_VALUE = np.float32(-123.5)     # behind the last row of `mount`, pre-filled and checked


def lib():
    return emu_binding.shim("sensor_mount_jitter")


def EmuApi():
    """the sensor, encoder and memory shims plus this one, for envs.sensors.RaySensor(api=...); counts the sensor launches"""
    return emu_binding.api("raycast", "raycast_bodies", "sensor_model", "depth_encoder", "depth_memory", "sensor_mount_jitter",
                           count=("lsim_raycast", "lsim_raycast_bodies", "lsim_sensor_capture", "lsim_sensor_mount_jitter"))


class Rig(LaunchRig):
    """`nominal` [N, 7]; `mount` starts as NaN with guard floats behind it, episode_length as 1.  `device`: None -- numpy arrays and
    the shim -- or a torch device and `entry` = the library's lsim_sensor_mount_jitter."""

    def __init__(self, nominal, pos_range=(0.0, 0.0, 0.0), rot_range=(0.0, 0.0, 0.0), env_stride=1, seed=1, rank=0, stream_id=0, device=None, entry=None):
        nominal = np.ascontiguousarray(nominal, np.float32)
        N = self.N = nominal.shape[0]
        super().__init__(device)
        self.add("nominal", nominal)
        self.add("mount", np.full((N, 7), np.nan, np.float32), guard=GUARD_VALUE)
        self.add("episode_length", np.ones(N, np.int64))
        mj = abi.LsimSensorMountJitter()
        self.point(mj, ("nominal", "mount", "episode_length"))
        mj.seed, mj.rank, mj.stream_id, mj.num_envs, mj.env_stride = int(seed), int(rank), int(stream_id), N, int(env_stride)
        self.mj = self.bind(mj, entry if device is not None else lib().emu_sensor_mount_jitter)
        self.set_ranges(pos_range, rot_range)

    def set_ranges(self, pos_range, rot_range):
        """the struct's ranges, in place"""
        for k in range(3):
            self.mj.pos_range[k], self.mj.rot_range[k] = float(pos_range[k]), float(rot_range[k])
        self.pos_range = np.array([self.mj.pos_range[k] for k in range(3)], np.float32)
        self.rot_range = np.array([self.mj.rot_range[k] for k in range(3)], np.float32)

    def fill_mount(self, value=np.nan):
        self.put("mount", value)

    def read(self):
        """(mount [N, 7], guard) copies; asserts the guard intact"""
        self.assert_guards()
        return self.get("mount"), self.raw("mount")[self.N * 7:]
