"""TEST INFRASTRUCTURE -- builds and binds tests/emu/emu_raycast_bodies.cpp (the CPU shim of the body-aware range-sensor launch,
isaacgymloco_amd/csrc/ls_raycast_bodies.h compiled by g++ under LS_EMU) and fills an lsim_raycast_bodies from numpy arrays."""
import ctypes
import os
import subprocess

import numpy as np

import raycast_emu_binding as EMU
from helpers import ROOT, abi

SRC = os.path.join(ROOT, "tests", "emu", "emu_raycast_bodies.cpp")
_libs = {}


def build(counters=False):
    out = os.path.join(ROOT, "tests", "_build", "libraycast_bodies_emu_counters.so" if counters else "libraycast_bodies_emu.so")
    deps = [SRC, os.path.join(ROOT, "include", "lsim.h")] + [os.path.join(ROOT, "isaacgymloco_amd", "csrc", f) for f in ("ls_raycast.h", "ls_raycast_bodies.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas"] +
                              (["-DLS_RAYCAST_COUNTERS"] if counters else []) + ["-o", out, SRC])
    return out


def lib(counters=False):
    if counters not in _libs:
        L = ctypes.CDLL(build(counters))
        sz = ctypes.POINTER(ctypes.c_size_t)
        L.emu_raycast_bodies_sizes.argtypes = [sz, sz]
        L.emu_raycast_bodies.argtypes = [ctypes.POINTER(abi.LsimRaycastBodies), ctypes.c_void_p]
        _libs[counters] = L
    return _libs[counters]


class EmuApi(EMU.EmuApi):
    """the four range-sensor entry points with the library's signatures (stream ignored), for envs.sensors.RaySensor(api=...); counts the calls"""

    def __init__(self):
        self.calls = {"lsim_raycast": 0, "lsim_raycast_bodies": 0}

    def lsim_raycast(self, rc, stream):
        self.calls["lsim_raycast"] += 1
        return super().lsim_raycast(rc, stream)

    def lsim_raycast_bodies_sizes(self, sb, rb):
        return lib().emu_raycast_bodies_sizes(sb, rb)

    def lsim_raycast_bodies(self, rb, stream):
        self.calls["lsim_raycast_bodies"] += 1
        return lib().emu_raycast_bodies(rb, None)


def fill(scene, tables, env_robot, root_states, dof_pos, mount, dirs, near, far, scale=None, env_stride=1, body_mask=0x1FFFF, flags=0, labels=True,
         out_fill=np.nan):
    """(lsim_raycast_bodies, dict of the arrays it points to): `tables` a list of lsim_raycast_robot, `env_robot` [N] or None, dof_pos [N, 12]"""
    rc, a = EMU.fill(scene, root_states, mount, dirs, near, far, scale, env_stride, out_fill)
    N, R = root_states.shape[0], dirs.shape[0]
    a["dof_state"] = EMU.aligned((N, 12, 2), np.float32)
    a["dof_state"][:, :, 0] = dof_pos
    a["robots"] = (abi.LsimRaycastRobot * len(tables))(*tables)
    rb = abi.LsimRaycastBodies()
    rb.rc = rc
    rb.dof_state = a["dof_state"].ctypes.data
    rb.robots = rb.robots_host = ctypes.addressof(a["robots"])
    rb.num_robots = len(tables)
    if env_robot is not None:
        a["env_robot"] = np.ascontiguousarray(env_robot, np.uint8)
        rb.env_robot = a["env_robot"].ctypes.data
    if labels:
        a["labels"] = np.full((N, R + 5), 255, np.uint8)
        rb.labels, rb.label_stride = a["labels"].ctypes.data, R + 5
    rb.body_mask, rb.flags = body_mask, flags
    return rb, a


def cast(scene, tables, env_robot, root_states, dof_pos, mount, dirs, near, far, counters=False, **kw):
    """run the emulated launch: (out [N, R], labels [N, R], state [4], body poses [N, 17, 8])"""
    rb, a = fill(scene, tables, env_robot, root_states, dof_pos, mount, dirs, near, far, **kw)
    bodies = np.full((root_states.shape[0], 17, 8), np.nan, np.float32)
    rv = lib(counters).emu_raycast_bodies(ctypes.byref(rb), bodies.ctypes.data)
    assert rv == 0, rv
    R = dirs.shape[0]
    return a["out"][:, :R].copy(), a["labels"][:, :R].copy(), a["state"].copy(), bodies
