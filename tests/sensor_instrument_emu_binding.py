"""TEST INFRASTRUCTURE -- builds and binds tests/emu/emu_sensor_instrument.cpp (the CPU shim of the two instrument launches,
isaacgymloco_amd/csrc/ls_sensor_instrument.h compiled by g++ under LS_EMU), and two rigs, in host memory for the shim or in device memory for
the HIP library, driven launch by launch: DrawRig, one lsim_sensor_instrument with the arrays it points to, and CaptureRig, the Rig of
tests/sensor_model_emu_binding.py with an `inst` array, whose launch() is lsim_sensor_capture_inst and whose plain() is lsim_sensor_capture."""
import ctypes

import numpy as np

import emu_binding
import sensor_model_emu_binding as SB
from helpers import abi
from launch_rig import LaunchRig

GUARD_VALUE = np.float32(-123.5)     # behind the last row of `inst`, pre-filled and checked
RANGES = ("lat_lo", "lat_hi", "gain_lo", "gain_hi", "scale_range", "quad_range", "fov_range")
NEUTRAL = dict(lat_lo=0, lat_hi=0, gain_lo=1.0, gain_hi=1.0, scale_range=0.0, quad_range=0.0, fov_range=0.0)


def lib():
    return emu_binding.shim("sensor_instrument")


def EmuApi():
    """the sensor, encoder, memory and mount-jitter shims plus this one, for envs.sensors.RaySensor(api=...); counts the sensor launches"""
    return emu_binding.api("raycast", "raycast_bodies", "sensor_model", "depth_encoder", "depth_memory", "sensor_mount_jitter", "sensor_instrument",
                           count=("lsim_raycast", "lsim_raycast_bodies", "lsim_sensor_capture", "lsim_sensor_mount_jitter",
                                  "lsim_sensor_instrument", "lsim_sensor_capture_inst"))


def neutral_rows(num_envs, latency):
    rows = np.zeros((num_envs, 8), np.float32)
    rows[:, 0], rows[:, 1], rows[:, 4] = latency, 1.0, 1.0
    return rows


class DrawRig(LaunchRig):
    """`inst` [N, 8] starts as NaN with guard floats behind it, episode_length as 1; `ranges`: the struct's seven range fields (NEUTRAL's,
    overridden).  `device`: None -- numpy arrays and the shim -- or a torch device and `entry` = the library's lsim_sensor_instrument."""

    def __init__(self, num_envs, env_stride=1, seed=1, rank=0, stream_id=0, device=None, entry=None, **ranges):
        N = self.N = int(num_envs)
        super().__init__(device)
        self.add("inst", np.full((N, 8), np.nan, np.float32), guard=GUARD_VALUE)
        self.add("episode_length", np.ones(N, np.int64))
        si = abi.LsimSensorInstrument()
        self.point(si, ("inst", "episode_length"))
        si.seed, si.rank, si.stream_id, si.num_envs, si.env_stride = int(seed), int(rank), int(stream_id), N, int(env_stride)
        self.si = self.bind(si, entry if device is not None else lib().emu_sensor_instrument)
        self.set_ranges(**dict(NEUTRAL, **ranges))

    def set_ranges(self, **ranges):
        """the struct's ranges, in place; `self.ranges` holds them as the struct does (fp32)"""
        for k, v in ranges.items():
            assert k in RANGES, k
            setattr(self.si, k, v)
        self.ranges = {k: getattr(self.si, k) for k in RANGES}

    def fill_rows(self, value=np.nan):
        self.put("inst", value)

    def read(self):
        """(inst [N, 8], guard) copies; asserts the guard intact"""
        self.assert_guards()
        return self.get("inst"), self.raw("inst")[self.N * 8:]


class CaptureRig(SB.Rig):
    """SB.Rig plus `inst` [N, 8] (the neutral rows of the model's latency to begin with; put("inst", rows) changes them).  launch() is
    lsim_sensor_capture_inst, plain() lsim_sensor_capture on the same struct and arrays.  `device`: as SB.Rig's, with `entry` = the library
    (its two entry points are taken by name)."""

    def __init__(self, *a, device=None, entry=None, **kw):
        L = entry
        super().__init__(*a, device=device, entry=None if L is None else L.lsim_sensor_capture, **kw)
        self.add("inst", neutral_rows(self.N, self.p["latency"]))
        self._inst_entry = L.lsim_sensor_capture_inst if device is not None else lib().emu_sensor_capture_inst

    def launch(self, tick, flags=0, edit=None, inst="own"):
        """one lsim_sensor_capture_inst; `edit(sm)` changes a copy of the struct first, `inst` replaces the pointer (an address or None)"""
        ptr = self.ptr("inst") if isinstance(inst, str) else inst
        return super().launch(tick, flags, edit, entry=lambda sm, stream: self._inst_entry(sm, None if ptr is None else ctypes.c_void_p(ptr), stream))

    def plain(self, tick, flags=0, edit=None):
        """one lsim_sensor_capture on the same struct"""
        return super().launch(tick, flags, edit)
