"""TEST INFRASTRUCTURE -- builds and binds tests/emu/emu_sensor_stereo.cpp (the CPU shim of the stereo-artefact launch,
isaacgymloco_amd/csrc/ls_sensor_stereo.h compiled by g++ under LS_EMU), and Rig: one lsim_sensor_stereo with the arrays it points to, in
host memory for the shim or in device memory for the HIP library, driven launch by launch.  Every array the launch writes (hist, state)
has GUARD elements behind it, pre-filled and checked on every read."""
import ctypes

import numpy as np

import emu_binding
import sensor_model_emu_binding as SB
from helpers import abi

HEADERS = SB.HEADERS + ["ls_sensor_stereo.h"]
GUARD = 16
GUARD_VALUE = {"hist": np.float32(-123.5), "state": np.int64(0x5A5A5A5A5A5A)}
SCALARS = ("width", "height", "num_envs", "env_stride", "period", "stagger", "latency", "frames", "seed", "rank", "stream_id", "fb", "max_disparity",
           "window", "t_lo", "t_hi", "edge_radius", "edge_rel", "p_edge_hole", "p_edge_cum", "drop_value", "clip_lo", "clip_hi", "offset", "gain")
_INT = ("width", "height", "num_envs", "env_stride", "period", "stagger", "latency", "frames", "seed", "rank", "stream_id", "window", "edge_radius")
DEFAULTS = dict(env_stride=1, period=1, stagger=0, latency=0, frames=1, seed=3, rank=0, stream_id=2, fb=8.0, max_disparity=64.0, window=8, t_lo=0.0625,
                t_hi=16.0, edge_radius=1, edge_rel=0.0625, p_edge_hole=0.0, p_edge_cum=0.0, drop_value=0.0, clip_lo=0.0, clip_hi=32.0, offset=0.0, gain=1.0)


def lib():
    return emu_binding.load_shim("sensor_stereo", HEADERS)


def EmuApi():
    """the sensor, encoder, memory and map shims plus this one, for envs.sensors.RaySensor(api=...); counts the sensor launches"""
    import depth_memory_emu_binding as GB
    import elevation_map_emu_binding as EB
    import frames_log_emu_binding as FB
    import sensor_instrument_emu_binding as IB
    import sensor_mount_jitter_emu_binding as MB
    return GB.EmuApi(MB.lib(), IB.lib(), EB.lib(), FB.lib(), lib(), count=("lsim_sensor_capture", "lsim_sensor_capture_inst", "lsim_sensor_instrument",
                                                                "lsim_sensor_stereo", "lsim_elevation_map"))


class Rig:
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
        self.N, self.R, self.K, self.device = N, R, self.p["latency"] + self.p["frames"], device
        self.depth_stride, self.label_stride, self.hist_stride = R + 5, R + 3, (R + 3) // 4 * 4 + 4
        al = emu_binding.aligned
        a = {"depth": al((N, self.depth_stride), np.float32), "episode_length": al((N,), np.int64)}
        a["depth"][:] = np.nan
        a["depth"][:, :R] = depth
        a["episode_length"][:] = 1
        if labels is not None:
            a["labels"] = al((N, self.label_stride), np.uint8)
            a["labels"][:, :R] = labels
        if inv_scale is not None:
            a["inv_scale"] = al((R,), np.float32)
            a["inv_scale"][:] = inv_scale
        if inst is not None:
            a["inst"] = al((N, 8), np.float32)
            a["inst"][:] = inst
        self.sizes = {"hist": N * self.K * self.hist_stride, "state": 2}
        a["hist"], a["state"] = al((self.sizes["hist"] + GUARD,), np.float32), al((2 + GUARD,), np.int64)
        if hist is None:
            hist = initial_hist(N, self.K, R)
        h = np.full((N, self.K, self.hist_stride), -9.25, np.float32)
        h[:, :, :R] = hist
        a["hist"][:self.sizes["hist"]], a["hist"][self.sizes["hist"]:] = h.reshape(-1), GUARD_VALUE["hist"]
        a["state"][2:] = GUARD_VALUE["state"]
        if device is not None:
            import torch
            a = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in a.items()}
        self.a = a
        st = abi.LsimSensorStereo()
        for k in ("depth", "labels", "inv_scale", "episode_length", "inst", "hist", "state"):
            setattr(st, k, self._ptr(k) if k in a else None)
        st.depth_stride, st.label_stride, st.hist_stride = self.depth_stride, self.label_stride, self.hist_stride
        for k in SCALARS:
            setattr(st, k, int(self.p[k]) if k in _INT else self.p[k])
        self.st = st
        self._entry = entry if device is not None else lib().emu_sensor_stereo

    def _ptr(self, k):
        return self.a[k].data_ptr() if self.device is not None else self.a[k].ctypes.data

    def put(self, name, value):
        """array `name` (episode_length, inst, ...) = value, broadcast"""
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

    def launch(self, tick, flags=0, edit=None, stream=None):
        """one launch; `edit(st)` changes a copy of the struct first; returns the entry point's value"""
        st = abi.LsimSensorStereo.from_buffer_copy(self.st)
        st.tick, st.flags = tick, flags
        if edit:
            edit(st)
        if self.device is not None and stream is None:
            import torch
            stream = torch.cuda.current_stream().cuda_stream
        return self._entry(ctypes.byref(st), None if stream is None else ctypes.c_void_p(stream))

    def read(self):
        """copies: hist [N, K, R], hist_pad (the padding of every slot), state [2]; asserts every guard intact"""
        out = {}
        for k in ("hist", "state"):
            v = self.get(k)
            assert (v[self.sizes[k]:] == GUARD_VALUE[k]).all(), f"guard of {k} overwritten"
            out[k] = v[:self.sizes[k]]
        h = out["hist"].reshape(self.N, self.K, self.hist_stride)
        out["hist"], out["hist_pad"] = h[:, :, :self.R].copy(), h[:, :, self.R:].copy()
        return out

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
