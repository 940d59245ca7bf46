"""TEST INFRASTRUCTURE -- builds and binds tests/emu/emu_raycast_bodies.cpp (the CPU shim of the body-aware range-sensor launch,
isaacgymloco_amd/csrc/ls_raycast_bodies.h compiled by g++ under LS_EMU) and fills an lsim_raycast_bodies from numpy arrays."""
import ctypes

import numpy as np

import emu_binding
import raycast_emu_binding as EMU
from helpers import abi


def lib(counters=False):
    L = emu_binding.shim("raycast_bodies", counters)
    L.emu_raycast_bodies_poses.argtypes = [ctypes.POINTER(abi.LsimRaycastBodies), ctypes.c_void_p]       # test-only: the body pose output
    return L


def EmuApi():
    """the four range-sensor entry points of the two shims, for envs.sensors.RaySensor(api=...); counts the launches"""
    return emu_binding.api("raycast", "raycast_bodies", count=("lsim_raycast", "lsim_raycast_bodies"))


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
    rv = lib(counters).emu_raycast_bodies_poses(ctypes.byref(rb), bodies.ctypes.data)
    assert rv == 0, rv
    R = dirs.shape[0]
    return a["out"][:, :R].copy(), a["labels"][:, :R].copy(), a["state"].copy(), bodies
