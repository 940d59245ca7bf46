"""TEST INFRASTRUCTURE -- builds and binds tests/emu/emu_sensor_model.cpp (the CPU shim of the sensor-model launch,
isaacgymloco_amd/csrc/ls_sensor_model.h compiled by g++ under LS_EMU), and Rig: one lsim_sensor_model with the arrays it points to, in host
memory for the shim or in device memory for the HIP library, driven launch by launch."""
import ctypes

import numpy as np

import emu_binding
import raycast_bodies_emu_binding as BE
import raycast_emu_binding as EMU
from helpers import abi

HEADERS = ["ls_raycast.h", "ls_raycast_bodies.h", "ls_sensor_model.h", "ls_math.h"]
IDENTITY = dict(period=1, stagger=0, latency=0, frames=1, sigma0=0.0, sigma2=0.0, p_drop=0.0, drop_value=0.0, offset=0.0, gain=1.0,
                seed=1, rank=0, stream_id=0)


def lib():
    return emu_binding.load_shim("sensor_model", HEADERS)


def EmuApi():
    """every range-sensor entry point of the three shims, for envs.sensors.RaySensor(api=...); counts the launches"""
    return emu_binding.EmuApi(EMU.lib(), BE.lib(), lib(), count=("lsim_raycast", "lsim_raycast_bodies", "lsim_sensor_capture"))


class Rig:
    """`bodies` = None (the terrain-only form) or dict(tables, env_robot, dof_pos, body_mask, flags); `model`: the scalar fields of the struct
    (IDENTITY's, overridden; clip_lo / clip_hi default to (0, far)).  `device`: None -- numpy arrays and the shim -- or a torch device and
    `entry` = the library's lsim_sensor_capture.  `out` starts as NaN, `labels` as 255, `hist` as -7."""

    def __init__(self, scene, root_states, mount, dirs, near, far, scale=None, env_stride=1, bodies=None, hist_stride=None, device=None, entry=None, **model):
        N, R = root_states.shape[0], dirs.shape[0]
        self.N, self.R, self.near, self.far, self.device = N, R, near, far, device
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
        self.K = self.p["latency"] + self.p["frames"]
        self.hist_stride = hist_stride or (R + 3) // 4 * 4
        a["episode_length"] = EMU.aligned((N,), np.int64)
        a["episode_length"][:] = 1
        a["hist"] = EMU.aligned((N, max(self.K, 1), self.hist_stride), np.float32)
        a["hist"][:] = -7.0
        self._robots = a.pop("robots", None)
        if device is not None:
            import torch
            a = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in a.items()}
            if self._robots is not None:
                a["robots"] = torch.from_numpy(np.frombuffer(self._robots, dtype=np.uint8).copy()).to(device)
                sm.rb.robots = a["robots"].data_ptr()
        self.a = a
        for k in ("root_states", "mount", "dirs", "out", "state", "scale", "mesh"):
            if k in a:
                setattr(sm.rb.rc, k, self._ptr(k))
        for k in ("dof_state", "env_robot", "labels"):
            if k in a:
                setattr(sm.rb, k, self._ptr(k))
        sm.episode_length, sm.hist, sm.hist_stride = self._ptr("episode_length"), self._ptr("hist"), self.hist_stride
        for k, v in self.p.items():
            setattr(sm, k, int(v) if k in ("period", "stagger", "latency", "frames", "seed", "rank", "stream_id") else v)
        self.sm = sm
        self._entry = entry if device is not None else lib().emu_sensor_capture

    def _ptr(self, k):
        return self.a[k].data_ptr() if self.device is not None else self.a[k].ctypes.data

    def put(self, name, value):
        """overwrite an array (root_states, episode_length, out, labels, hist, dof_state ...) with a value that broadcasts to it"""
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

    def launch(self, tick, flags=0, edit=None):
        """one launch; `edit(sm)` changes a copy of the struct first; returns the entry point's value"""
        sm = abi.LsimSensorModel.from_buffer_copy(self.sm)
        sm.tick, sm.flags = tick, flags
        if edit:
            edit(sm)
        stream = None
        if self.device is not None:
            import torch
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        return self._entry(ctypes.byref(sm), stream)

    def read(self):
        """(out [N, R], labels [N, R], hist [N, K, R], state [4]) copies"""
        return self.get("out")[:, :self.R], self.get("labels")[:, :self.R], self.get("hist")[:, :, :self.R], self.get("state")
