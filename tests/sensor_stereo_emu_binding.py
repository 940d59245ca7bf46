"""TEST INFRASTRUCTURE -- builds and binds tests/emu/emu_sensor_stereo.cpp (the CPU shim of the stereo-artefact launch,
isaacgymloco_amd/csrc/ls_sensor_stereo.h compiled by g++ under LS_EMU), and Rig: one lsim_sensor_stereo with the arrays it points to, in
host memory for the shim or in device memory for the HIP library, driven launch by launch.  Every array the launch writes (hist, state)
has guard elements behind it, pre-filled with GUARD_VALUE and checked on every read."""
import numpy as np

import emu_binding
from helpers import abi
from launch_rig import LaunchRig

GUARD_VALUE = {"hist": np.float32(-123.5), "state": np.int64(0x5A5A5A5A5A5A)}
SCALARS = ("width", "height", "num_envs", "env_stride", "period", "stagger", "latency", "frames", "seed", "rank", "stream_id", "fb", "max_disparity",
           "window", "t_lo", "t_hi", "edge_radius", "edge_rel", "p_edge_hole", "p_edge_cum", "drop_value", "clip_lo", "clip_hi", "offset", "gain")
_INT = ("width", "height", "num_envs", "env_stride", "period", "stagger", "latency", "frames", "seed", "rank", "stream_id", "window", "edge_radius")
DEFAULTS = dict(env_stride=1, period=1, stagger=0, latency=0, frames=1, seed=3, rank=0, stream_id=2, fb=8.0, max_disparity=64.0, window=8, t_lo=0.0625,
                t_hi=16.0, edge_radius=1, edge_rel=0.0625, p_edge_hole=0.0, p_edge_cum=0.0, drop_value=0.0, clip_lo=0.0, clip_hi=32.0, offset=0.0, gain=1.0)


def lib():
    return emu_binding.shim("sensor_stereo")


def EmuApi():
    """the sensor, encoder, memory and map shims plus this one, for envs.sensors.RaySensor(api=...); counts the sensor launches"""
    return emu_binding.api("raycast", "raycast_bodies", "sensor_model", "depth_encoder", "depth_memory", "sensor_mount_jitter", "sensor_instrument",
                           "elevation_map", "frames_log", "sensor_stereo", count=("lsim_sensor_capture", "lsim_sensor_capture_inst",
                                                                                  "lsim_sensor_instrument", "lsim_sensor_stereo", "lsim_elevation_map"))


class Rig(LaunchRig):
    """N envs of a width x height image.  `depth` [N, R] (rows padded to depth_stride), `labels` [N, R] or None, `inv_scale` [R] or None,
    `inst` [N, 8] or None; `hist` starts as `hist` [N, K, R] (default: distinct values per env, slot and pixel) inside rows padded to
    hist_stride, episode_length as 1, state as 0.  `device`: None -- numpy arrays and the shim -- or a torch device and `entry` = the
    library's lsim_sensor_stereo.  **params: the struct's by-value fields over DEFAULTS."""

    def __init__(self, width, height, depth, labels=None, inv_scale=None, inst=None, hist=None, device=None, entry=None, **params):
        depth = np.asarray(depth, np.float32)
        N, R = depth.shape[0], width * height
        assert depth.shape == (N, R)
        self.p = dict(DEFAULTS, width=int(width), height=int(height), num_envs=N)
        self.p.update(params)
        super().__init__(device)
        self.N, self.R, self.K = N, R, self.p["latency"] + self.p["frames"]
        self.depth_stride, self.label_stride, self.hist_stride = R + 5, R + 3, (R + 3) // 4 * 4 + 4
        d = np.full((N, self.depth_stride), np.nan, np.float32)
        d[:, :R] = depth
        self.add("depth", d)
        self.add("episode_length", np.ones(N, np.int64))
        if labels is not None:
            lab = np.zeros((N, self.label_stride), np.uint8)
            lab[:, :R] = labels
            self.add("labels", lab)
        if inv_scale is not None:
            self.add("inv_scale", np.broadcast_to(np.asarray(inv_scale, np.float32), (R,)))
        if inst is not None:
            self.add("inst", np.broadcast_to(np.asarray(inst, np.float32), (N, 8)))
        h = np.full((N, self.K, self.hist_stride), -9.25, np.float32)
        h[:, :, :R] = initial_hist(N, self.K, R) if hist is None else hist
        self.add("hist", h, guard=GUARD_VALUE["hist"])
        self.add("state", np.zeros(2, np.int64), guard=GUARD_VALUE["state"])
        st = abi.LsimSensorStereo()
        self.point(st, ("depth", "labels", "inv_scale", "episode_length", "inst", "hist", "state"))
        st.depth_stride, st.label_stride, st.hist_stride = self.depth_stride, self.label_stride, self.hist_stride
        for k in SCALARS:
            setattr(st, k, int(self.p[k]) if k in _INT else self.p[k])
        self.st = self.bind(st, entry if device is not None else lib().emu_sensor_stereo)

    def read(self):
        """copies: hist [N, K, R], hist_pad (the padding of every slot), state [2]; asserts every guard intact"""
        self.assert_guards()
        h = self.get("hist")
        return {"hist": h[:, :, :self.R].copy(), "hist_pad": h[:, :, self.R:].copy(), "state": self.get("state")}

    def inputs(self):
        """what the reference reads: copies of depth [N, R], labels, inv_scale, episode_length, inst (None where absent)"""
        d = {k: (self.get(k) if k in self.a else None) for k in ("depth", "labels", "inv_scale", "episode_length", "inst")}
        d["depth"] = d["depth"][:, :self.R]
        if d["labels"] is not None:
            d["labels"] = d["labels"][:, :self.R]
        return d


def initial_hist(N, K, R):
    """[N, K, R] float32, every element its own exactly representable value: what a capture might have left"""
    return (np.arange(N * K * R, dtype=np.float32).reshape(N, K, R) * np.float32(2.0 ** -8) + np.float32(100.0)).astype(np.float32)
