"""TEST INFRASTRUCTURE -- builds and binds tests/emu/emu_elevation_map.cpp (the CPU shim of the elevation-map launch,
isaacgymloco_amd/csrc/ls_elevation_map.h compiled by g++ under LS_EMU), and Rig: one lsim_elevation_map with the arrays it points to, in
host memory for the shim or in device memory for the HIP library, driven launch by launch.  Every array the launch writes has GUARD
elements behind it, pre-filled and checked."""
import ctypes

import numpy as np

import emu_binding
import sensor_model_emu_binding as SB
from helpers import abi

HEADERS = SB.HEADERS + ["ls_elevation_map.h"]
GUARD = 16
WRITTEN = {"height": np.float32, "stamp": np.int32, "cell": np.uint32, "scan": np.float32, "known": np.uint8}
GUARD_VALUE = {"height": -123.5, "stamp": 0x5A5A5A5A, "cell": 0xA5A5A5A5, "scan": -321.25, "known": 0x7E}
INITIAL = {"height": 777.0, "stamp": -1, "cell": 0, "scan": 555.0, "known": 9}


def lib():
    return emu_binding.load_shim("elevation_map", HEADERS)


def EmuApi():
    """the sensor, encoder and memory shims plus this one, for envs.sensors.RaySensor(api=...); counts the sensor launches"""
    import depth_memory_emu_binding as GB
    import sensor_instrument_emu_binding as IB
    import sensor_mount_jitter_emu_binding as MB
    return GB.EmuApi(MB.lib(), IB.lib(), lib(), count=("lsim_raycast", "lsim_raycast_bodies", "lsim_sensor_capture", "lsim_sensor_capture_inst",
                                                       "lsim_sensor_mount_jitter", "lsim_sensor_instrument", "lsim_elevation_map"))


class Rig:
    """N envs, a G x G map, `dirs` [R, 3], `pts` [P, 2].  root_states start as the identity pose at the origin, the mount as the identity,
    depth as 1e9 (every ray a miss), labels (when `labels`) as 1, episode_length as 1; the map as never written (stamp -1, height and cell
    INITIAL), scan / known as INITIAL.  `device`: None -- numpy arrays and the shim -- or a torch device and `entry` = the library's
    lsim_elevation_map."""

    def __init__(self, N, G, dirs, pts, res=2.0 ** -4, inv_scale=None, labels=False, env_stride=1, period=1, stagger=0, a=1.0, b=0.0, t_lo=0.0,
                 t_hi=100.0, unknown_drop=0.5, depth_pad=4, device=None, entry=None):
        dirs, pts = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3), np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        self.N, self.G, self.R, self.P, self.device = int(N), int(G), dirs.shape[0], pts.shape[0], device
        N, G, R, P = self.N, self.G, self.R, self.P
        self.depth_stride, self.label_stride, self.scan_stride, self.known_stride = R + depth_pad, R + 3, P + 1, P + 2
        al = emu_binding.aligned
        a_ = {"root_states": al((N, 13), np.float32), "mount": al((N, 7), np.float32), "dirs": al((R, 3), np.float32), "pts": al((P, 2), np.float32),
              "depth": al((N, self.depth_stride), np.float32), "episode_length": al((N,), np.int64), "state": al((1,), np.int64)}
        a_["root_states"][:, 6] = 1.0
        a_["mount"][:, 6] = 1.0
        a_["dirs"][:], a_["pts"][:] = dirs, pts
        a_["depth"][:] = 1e9
        a_["episode_length"][:] = 1
        if inv_scale is not None:
            a_["inv_scale"] = al((R,), np.float32)
            a_["inv_scale"][:] = inv_scale
        if labels:
            a_["labels"] = al((N, self.label_stride), np.uint8)
            a_["labels"][:] = 1
        self.sizes = {"height": N * G * G, "stamp": N * G * G, "cell": N * G * G, "scan": N * self.scan_stride, "known": N * self.known_stride}
        for k, dt in WRITTEN.items():
            a_[k] = al((self.sizes[k] + GUARD,), dt)
            a_[k][:self.sizes[k]] = INITIAL[k]
            a_[k][self.sizes[k]:] = np.array(GUARD_VALUE[k]).astype(dt)
        if device is not None:
            import torch
            a_ = {k: torch.from_numpy(np.ascontiguousarray(v).view(np.int32) if v.dtype == np.uint32 else np.ascontiguousarray(v)).to(device) for k, v in a_.items()}
        self.a = a_
        em = abi.LsimElevationMap()
        em.root_states, em.assumed_mount, em.dirs, em.pts = self._ptr("root_states"), self._ptr("mount"), self._ptr("dirs"), self._ptr("pts")
        em.depth, em.episode_length, em.state = self._ptr("depth"), self._ptr("episode_length"), self._ptr("state")
        em.inv_scale = self._ptr("inv_scale") if inv_scale is not None else None
        em.labels = self._ptr("labels") if labels else None
        em.height, em.stamp, em.cell, em.scan, em.known = (self._ptr(k) for k in ("height", "stamp", "cell", "scan", "known"))
        em.depth_stride, em.label_stride, em.scan_stride, em.known_stride = self.depth_stride, self.label_stride, self.scan_stride, self.known_stride
        em.num_envs, em.num_rays, em.env_stride, em.num_points, em.size = N, R, int(env_stride), P, G
        em.period, em.stagger = int(period), int(stagger)
        em.res, em.a, em.b, em.t_lo, em.t_hi, em.unknown_drop = res, a, b, t_lo, t_hi, unknown_drop
        self.em = em
        self._entry = entry if device is not None else lib().emu_elevation_map

    def _ptr(self, k):
        return self.a[k].data_ptr() if self.device is not None else self.a[k].ctypes.data

    def put(self, name, value):
        """array `name` = value (broadcast); depth and labels take [N, R] rows, a written array its elements ahead of the guard"""
        cur = self.get(name, guard=True)
        value = np.asarray(value, dtype=cur.dtype)
        if name in ("depth", "labels"):
            cur[:, :self.R] = value
        elif name in self.sizes:
            cur[:self.sizes[name]] = value.reshape(-1) if value.ndim else value
        else:
            cur[...] = value
        if self.device is not None:
            import torch
            self.a[name].copy_(torch.from_numpy(cur.view(np.int32) if cur.dtype == np.uint32 else cur).to(self.device))
        else:
            self.a[name][...] = cur

    def get(self, name, guard=False):
        if self.device is not None:
            import torch
            torch.cuda.synchronize()
            v = self.a[name].cpu().numpy().copy()
            if name == "cell":
                v = v.view(np.uint32)
        else:
            v = self.a[name].copy()
        return v if guard or name not in self.sizes else v[:self.sizes[name]]

    def launch(self, tick, flags=0, edit=None, stream=None):
        """one launch; `edit(em)` changes a copy of the struct first; returns the entry point's value"""
        em = abi.LsimElevationMap.from_buffer_copy(self.em)
        em.tick, em.flags = tick, flags
        if edit:
            edit(em)
        if self.device is not None and stream is None:
            import torch
            stream = torch.cuda.current_stream().cuda_stream
        return self._entry(ctypes.byref(em), None if stream is None else ctypes.c_void_p(stream))

    def read(self):
        """copies: height, stamp, cell [N, G, G]; scan, known [N, P]; state (int); asserts every guard intact"""
        N, G = self.N, self.G
        out = {}
        for k in WRITTEN:
            v = self.get(k, guard=True)
            assert (v[self.sizes[k]:] == np.array(GUARD_VALUE[k]).astype(WRITTEN[k])).all(), f"guard of {k} overwritten"
            out[k] = v[:self.sizes[k]]
        for k in ("height", "stamp", "cell"):
            out[k] = out[k].reshape(N, G, G)
        out["scan_pad"], out["known_pad"] = out["scan"].reshape(N, self.scan_stride)[:, self.P:], out["known"].reshape(N, self.known_stride)[:, self.P:]
        out["scan"], out["known"] = out["scan"].reshape(N, self.scan_stride)[:, :self.P], out["known"].reshape(N, self.known_stride)[:, :self.P]
        out["state"] = int(self.get("state")[0])
        return out

    def inputs(self):
        """what the reference reads: copies of the input arrays"""
        d = {k: self.get(k) for k in ("root_states", "mount", "depth", "episode_length")}
        d["depth"] = d["depth"][:, :self.R]
        d["labels"] = self.get("labels")[:, :self.R] if "labels" in self.a else None
        return d
