"""TEST INFRASTRUCTURE -- builds and binds tests/emu/emu_elevation_map.cpp (the CPU shim of the elevation-map launch,
isaacgymloco_amd/csrc/ls_elevation_map.h compiled by g++ under LS_EMU), and Rig: one lsim_elevation_map with the arrays it points to, in
host memory for the shim or in device memory for the HIP library, driven launch by launch.  Every array the launch writes has guard
elements behind it, pre-filled with GUARD_VALUE and checked."""
import numpy as np

import emu_binding
from helpers import abi
from launch_rig import LaunchRig

WRITTEN = {"height": np.float32, "stamp": np.int32, "cell": np.uint32, "scan": np.float32, "known": np.uint8}
GUARD_VALUE = {"height": -123.5, "stamp": 0x5A5A5A5A, "cell": 0xA5A5A5A5, "scan": -321.25, "known": 0x7E}
INITIAL = {"height": 777.0, "stamp": -1, "cell": 0, "scan": 555.0, "known": 9}


def lib():
    return emu_binding.shim("elevation_map")


def EmuApi():
    """the sensor, encoder and memory shims plus this one, for envs.sensors.RaySensor(api=...); counts the sensor launches"""
    return emu_binding.api("raycast", "raycast_bodies", "sensor_model", "depth_encoder", "depth_memory", "sensor_mount_jitter", "sensor_instrument",
                           "elevation_map", count=("lsim_raycast", "lsim_raycast_bodies", "lsim_sensor_capture", "lsim_sensor_capture_inst",
                                                   "lsim_sensor_mount_jitter", "lsim_sensor_instrument", "lsim_elevation_map"))


class Rig(LaunchRig):
    """N envs, a G x G map, `dirs` [R, 3], `pts` [P, 2].  root_states start as the identity pose at the origin, the mount as the identity,
    depth as 1e9 (every ray a miss), labels (when `labels`) as 1, episode_length as 1; the map as never written (stamp -1, height and cell
    INITIAL), scan / known as INITIAL.  `device`: None -- numpy arrays and the shim -- or a torch device and `entry` = the library's
    lsim_elevation_map."""

    def __init__(self, N, G, dirs, pts, res=2.0 ** -4, inv_scale=None, labels=False, env_stride=1, period=1, stagger=0, a=1.0, b=0.0, t_lo=0.0,
                 t_hi=100.0, unknown_drop=0.5, depth_pad=4, device=None, entry=None):
        dirs, pts = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3), np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        super().__init__(device)
        self.N, self.G, self.R, self.P = int(N), int(G), dirs.shape[0], pts.shape[0]
        N, G, R, P = self.N, self.G, self.R, self.P
        self.depth_stride, self.label_stride, self.scan_stride, self.known_stride = R + depth_pad, R + 3, P + 1, P + 2
        pose = np.zeros((N, 13), np.float32)
        pose[:, 6] = 1.0
        self.add("root_states", pose)
        self.add("mount", pose[:, :7])
        self.add("dirs", dirs)
        self.add("pts", pts)
        self.add("depth", np.full((N, self.depth_stride), 1e9, np.float32))
        self.add("episode_length", np.ones(N, np.int64))
        self.add("state", np.zeros(1, np.int64), guard=True)
        if inv_scale is not None:
            self.add("inv_scale", np.broadcast_to(np.asarray(inv_scale, np.float32), (R,)))
        if labels:
            self.add("labels", np.ones((N, self.label_stride), np.uint8))
        shapes = {"height": (N, G, G), "stamp": (N, G, G), "cell": (N, G, G), "scan": (N, self.scan_stride), "known": (N, self.known_stride)}
        for k, dt in WRITTEN.items():
            self.add(k, np.full(shapes[k], INITIAL[k], dt), guard=GUARD_VALUE[k])
        em = abi.LsimElevationMap()
        self.point(em, ("root_states", "dirs", "pts", "depth", "episode_length", "state", "inv_scale", "labels", "height", "stamp", "cell", "scan", "known"))
        em.assumed_mount = self.ptr("mount")
        em.depth_stride, em.label_stride, em.scan_stride, em.known_stride = self.depth_stride, self.label_stride, self.scan_stride, self.known_stride
        em.num_envs, em.num_rays, em.env_stride, em.num_points, em.size = N, R, int(env_stride), P, G
        em.period, em.stagger = int(period), int(stagger)
        em.res, em.a, em.b, em.t_lo, em.t_hi, em.unknown_drop = res, a, b, t_lo, t_hi, unknown_drop
        self.em = self.bind(em, entry if device is not None else lib().emu_elevation_map)

    def put(self, name, value):
        """array `name` = value (broadcast); depth and labels take [N, R] rows"""
        if name in ("depth", "labels"):
            rows = self.get(name)
            rows[:, :self.R] = value
            value = rows
        super().put(name, value)

    def read(self):
        """copies: height, stamp, cell [N, G, G]; scan, known [N, P]; state (int); asserts every guard intact"""
        self.assert_guards()
        out = {k: self.get(k) for k in WRITTEN}
        out["scan_pad"], out["known_pad"] = out["scan"][:, self.P:], out["known"][:, self.P:]
        out["scan"], out["known"] = out["scan"][:, :self.P], out["known"][:, :self.P]
        out["state"] = int(self.get("state")[0])
        return out

    def inputs(self):
        """what the reference reads: copies of the input arrays"""
        d = {k: self.get(k) for k in ("root_states", "mount", "depth", "episode_length")}
        d["depth"] = d["depth"][:, :self.R]
        d["labels"] = self.get("labels")[:, :self.R] if "labels" in self.a else None
        return d
