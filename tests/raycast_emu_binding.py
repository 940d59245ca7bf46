"""TEST INFRASTRUCTURE -- builds and binds tests/emu/emu_raycast.cpp (the CPU shim of the range-sensor launch, isaacgymloco_amd/csrc/ls_raycast.h
compiled by g++ under LS_EMU) and fills an lsim_raycast from numpy arrays."""
import ctypes

import numpy as np

import emu_binding
from emu_binding import aligned
from helpers import abi


def lib(counters=False):
    return emu_binding.shim("raycast", counters)


def EmuApi():
    """lsim_raycast_sizes / lsim_raycast of the shim, for envs.sensors.RaySensor(api=...)"""
    return emu_binding.api("raycast")


def fill(scene, root_states, mount, dirs, near, far, scale=None, env_stride=1, out_fill=np.nan):
    """(lsim_raycast, dict of the arrays it points to) for a scene of tests/raycast_reference.py: dict(mesh_type, words or None, hs, vs, border)"""
    N, R = root_states.shape[0], dirs.shape[0]
    stride = (R + 3) // 4 * 4
    a = {"root_states": aligned((N, 13), np.float32), "mount": aligned((N, 7), np.float32), "dirs": aligned((R, 3), np.float32),
         "out": aligned((N, stride), np.float32), "state": aligned((abi.DEFINES["LSIM_RAYCAST_STATE_WORDS"],), np.int64)}
    a["root_states"][:], a["mount"][:], a["dirs"][:] = root_states, mount, dirs
    a["out"][:] = out_fill
    rc = abi.LsimRaycast()
    for k in ("root_states", "mount", "dirs", "out", "state"):
        setattr(rc, k, a[k].ctypes.data)
    if scale is not None:
        a["scale"] = aligned((R,), np.float32)
        a["scale"][:] = scale
        rc.scale = a["scale"].ctypes.data
    words = scene.get("words")
    if words is not None:
        a["mesh"] = aligned(words.shape, np.int32)
        a["mesh"][:] = words
        rc.mesh = a["mesh"].ctypes.data
        rc.grid_rows, rc.grid_cols = words.shape
    rc.mesh_type = scene["mesh_type"]
    rc.horizontal_scale, rc.vertical_scale, rc.border_size = scene.get("hs", 0.0), scene.get("vs", 0.0), scene.get("border", 0.0)
    rc.num_envs, rc.num_rays, rc.env_stride, rc.out_stride = N, R, env_stride, stride
    rc.near, rc.far = near, far
    return rc, a


def cast(scene, root_states, mount, dirs, near, far, scale=None, env_stride=1, counters=False):
    """run the emulated launch: (out [N,R], state [4])"""
    rc, a = fill(scene, root_states, mount, dirs, near, far, scale, env_stride)
    rv = lib(counters).emu_raycast(ctypes.byref(rc), None)
    assert rv == 0, rv
    return a["out"][:, :dirs.shape[0]].copy(), a["state"].copy()
