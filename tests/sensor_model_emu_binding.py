"""TEST INFRASTRUCTURE -- builds and binds tests/emu/emu_sensor_model.cpp (the CPU shim of the sensor-model launch,
isaacgymloco_amd/csrc/ls_sensor_model.h compiled by g++ under LS_EMU), and Rig: one lsim_sensor_model with the arrays it points to, in host
memory for the shim or in device memory for the HIP library, driven launch by launch."""
import numpy as np

import emu_binding
import raycast_bodies_emu_binding as BE
import raycast_emu_binding as EMU
from helpers import abi
from launch_rig import LaunchRig

IDENTITY = dict(period=1, stagger=0, latency=0, frames=1, sigma0=0.0, sigma2=0.0, p_drop=0.0, drop_value=0.0, offset=0.0, gain=1.0,
                seed=1, rank=0, stream_id=0)
WRITTEN = ("out", "labels", "hist", "state")


def lib():
    return emu_binding.shim("sensor_model")


def EmuApi():
    """every range-sensor entry point of the three shims, for envs.sensors.RaySensor(api=...); counts the launches"""
    return emu_binding.api("raycast", "raycast_bodies", "sensor_model", count=("lsim_raycast", "lsim_raycast_bodies", "lsim_sensor_capture"))


class Rig(LaunchRig):
    """`bodies` = None (the terrain-only form) or dict(tables, env_robot, dof_pos, body_mask, flags); `model`: the scalar fields of the struct
    (IDENTITY's, overridden; clip_lo / clip_hi default to (0, far)).  `device`: None -- numpy arrays and the shim -- or a torch device and
    `entry` = the library's lsim_sensor_capture.  `out` starts as NaN, `labels` as 255, `hist` as -7; those and `state` are guarded."""

    def __init__(self, scene, root_states, mount, dirs, near, far, scale=None, env_stride=1, bodies=None, hist_stride=None, device=None, entry=None, **model):
        super().__init__(device)
        N, R = root_states.shape[0], dirs.shape[0]
        self.N, self.R, self.near, self.far = N, R, near, far
        self.p = dict(IDENTITY, clip_lo=0.0, clip_hi=far)
        self.p.update(model)
        sm = abi.LsimSensorModel()
        if bodies is None:
            rc, a = EMU.fill(scene, root_states, mount, dirs, near, far, scale, env_stride)
            a["labels"] = np.full((N, R + 5), 255, np.uint8)
            sm.rb.rc, sm.rb.label_stride = rc, R + 5
        else:
            rb, a = BE.fill(scene, bodies["tables"], bodies.get("env_robot"), root_states, bodies["dof_pos"], mount, dirs, near, far, scale=scale,
                            env_stride=env_stride, body_mask=bodies.get("body_mask", 0x1FFFF), flags=bodies.get("flags", 0))
            sm.rb = rb
            self._robots = a.pop("robots")                   # robots_host keeps pointing at this table
            a["robots"] = np.frombuffer(self._robots, dtype=np.uint8)
        self.K = self.p["latency"] + self.p["frames"]
        self.hist_stride = hist_stride or (R + 3) // 4 * 4
        a["episode_length"] = np.ones(N, np.int64)
        a["hist"] = np.full((N, max(self.K, 1), self.hist_stride), -7.0, np.float32)
        for k, v in a.items():                               # re-homed: the same shapes and strides, a guard behind what the launch may write
            self.add(k, v, guard=True if k in WRITTEN else None)
        self.point(sm.rb.rc, ("root_states", "mount", "dirs", "out", "state", "scale", "mesh"))
        self.point(sm.rb, ("dof_state", "env_robot", "labels", "robots"))
        self.point(sm, ("episode_length", "hist"))
        sm.hist_stride = self.hist_stride
        for k, v in self.p.items():
            setattr(sm, k, int(v) if k in ("period", "stagger", "latency", "frames", "seed", "rank", "stream_id") else v)
        self.sm = self.bind(sm, entry if device is not None else lib().emu_sensor_capture)

    def read(self):
        """(out [N, R], labels [N, R], hist [N, K, R], state [4]) copies; asserts every guard intact"""
        self.assert_guards()
        return self.get("out")[:, :self.R], self.get("labels")[:, :self.R], self.get("hist")[:, :, :self.R], self.get("state")
