"""TEST INFRASTRUCTURE -- builds and binds tests/emu/emu_foot_scan.cpp (the CPU shim of the foot-scan launch,
isaacgymloco_amd/csrc/ls_foot_scan.h compiled by g++ under LS_EMU) and its rig: the struct with the arrays it points to, in host memory for
the shim or in device memory for the HIP library.  Every array the launch writes has guard elements behind it, pre-filled and checked."""
import ctypes

import numpy as np

import emu_binding
from helpers import abi
from launch_rig import EditRig

_SENSOR = ["ls_raycast.h", "ls_raycast_bodies.h", "ls_sensor_model.h", "ls_math.h"]
HEADERS = _SENSOR + ["ls_elevation_map.h", "ls_foot_scan.h"]
LsimFootScan = abi.STRUCTS["lsim_foot_scan_t"]
TERRAIN, MAP = abi.DEFINES["LSIM_FOOT_SCAN_TERRAIN"], abi.DEFINES["LSIM_FOOT_SCAN_MAP"]
MAX_POINTS = abi.DEFINES["LSIM_FOOT_SCAN_MAX_POINTS"]
ROWS_INITIAL, HEIGHTS_INITIAL, KNOWN_INITIAL = np.float32(555.0), np.float32(333.0), np.uint8(0x5A)
GUARD_VALUE = np.float32(-123.5)


def lib():
    L = emu_binding.load_shim("foot_scan", HEADERS)
    L.emu_foot_scan_centres.argtypes = [ctypes.POINTER(LsimFootScan), ctypes.c_int, ctypes.c_void_p]      # test-only: the FK foot centres
    L.emu_foot_scan_centres.restype = ctypes.c_int
    return L


def EmuApi():
    """the sensor, map, odometry and row shims plus this one, for envs.sensors.RaySensor(api=...) and TerrainFootScan(api=...); counts the launches"""
    return emu_binding.api("raycast", "raycast_bodies", "sensor_model", "depth_encoder", "depth_memory", "sensor_mount_jitter", "sensor_instrument",
                           "elevation_map", "odometry", "map_rows", lib(),
                           count=("lsim_raycast", "lsim_raycast_bodies", "lsim_sensor_capture", "lsim_sensor_capture_inst", "lsim_sensor_mount_jitter",
                                  "lsim_sensor_instrument", "lsim_elevation_map", "lsim_odometry_step", "lsim_map_rows", "lsim_foot_scan"))


def table_bytes(tables):
    """the lsim_raycast_robot tables as one ctypes array (kept by the caller) and its bytes"""
    arr = (abi.LsimRaycastRobot * len(tables))(*tables)
    return arr, np.frombuffer(arr, dtype=np.uint8).copy()


class Rig(EditRig):
    """one scene (a dict of tests/foot_scan_scenes.py) as a launch: rows [N, ld], heights [N, 4K + pad] and known [N, 4K + pad] start as
    *_INITIAL with guards behind them; state is one int64 with a guard.  `device`: None -- numpy arrays and the shim -- or a torch device and
    `entry` = the library's lsim_foot_scan.  robots_host always points at host memory."""

    def __init__(self, sc, ld_pad=3, heights_pad=2, known_pad=5, outputs=True, device=None, entry=None):
        super().__init__(device)
        self.sc = sc
        pose = np.asarray(sc["pose"], np.float32)
        self.N, self.K = N, K = pose.shape[0], np.asarray(sc["pattern"]).shape[0]
        K4, C = 4 * K, int(sc["channels"])
        self.ld, self.heights_stride, self.known_stride = C * K4 + ld_pad, K4 + heights_pad, K4 + known_pad
        dof = np.zeros((N, 12, 2), np.float32)
        dof[:, :, 0], dof[:, :, 1] = sc["dof_pos"], 7.0                   # velocities: not read
        self._tables, tb = table_bytes(sc["tables"])
        self.add("pose", pose)
        self.add("dof_state", dof)
        self.add("robots", tb)
        self.add("pattern", np.asarray(sc["pattern"], np.float32))
        if sc.get("env_robot") is not None:
            self.add("env_robot", np.asarray(sc["env_robot"], np.uint8))
        if sc["source"] == TERRAIN:
            if sc["mesh_type"] != 0:
                self.add("height_grid", np.asarray(sc["height_grid"], np.int16))
        else:
            self.add("height", np.asarray(sc["height"], np.float32))
            self.add("stamp", np.asarray(sc["stamp"], np.int32))
            self.add("cell", np.asarray(sc["cell"], np.uint32))
        self.add("rows", np.full((N, self.ld), ROWS_INITIAL, np.float32), guard=GUARD_VALUE)
        if outputs:
            self.add("heights", np.full((N, self.heights_stride), HEIGHTS_INITIAL, np.float32), guard=GUARD_VALUE)
            self.add("known", np.full((N, self.known_stride), KNOWN_INITIAL, np.uint8), guard=np.uint8(0x7E))
        self.add("state", np.zeros(1, np.int64), guard=np.int64(-77))
        fs = LsimFootScan()
        self.point(fs, ("pose", "dof_state", "env_robot", "robots", "pattern", "height_grid", "height", "stamp", "cell", "rows", "heights", "known", "state"))
        fs.robots_host = ctypes.addressof(self._tables)
        fs.source, fs.num_envs, fs.env_stride, fs.num_robots = int(sc["source"]), N, int(sc["env_stride"]), len(sc["tables"])
        fs.num_points, fs.channels, fs.ld, fs.heights_stride, fs.known_stride = K, C, self.ld, self.heights_stride, self.known_stride
        fs.z_offset, fs.scale = float(sc["z_offset"]), float(sc["scale"])
        if sc["source"] == TERRAIN:
            fs.mesh_type = int(sc["mesh_type"])
            if sc["mesh_type"] != 0:
                g = np.asarray(sc["height_grid"])
                fs.grid_rows, fs.grid_cols = g.shape
                fs.horizontal_scale, fs.vertical_scale, fs.border_size = float(sc["hs"]), float(sc["vs"]), float(sc["border"])
        else:
            fs.size, fs.res, fs.unknown_drop = int(sc["G"]), float(sc["res"]), float(sc["unknown_drop"])
        self.fs = self.bind(fs, entry if device is not None else lib().emu_foot_scan)

    def read(self):
        """dict of copies: rows, heights, known (where the rig has them) and state; asserts the guards intact"""
        self.assert_guards()
        out = {k: self.get(k) for k in ("rows", "heights", "known") if k in self.a}
        out["state"] = int(self.get("state")[0])
        return out

    def run(self, stream=None):
        """one launch that must succeed: what read() gives after it, with the arrays before it under `before`"""
        before = self.read()
        assert self.launch(stream=stream) == 0
        got = self.read()
        got["before"] = before
        return got
