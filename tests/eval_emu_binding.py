"""TEST INFRASTRUCTURE -- builds and binds tests/emu/emu_eval.cpp (the CPU shim of the evaluator launch, isaacgymloco_amd/csrc/ls_eval.h compiled
by g++ under LS_EMU) and helps to fill an lsim_eval from numpy arrays."""
import ctypes

import numpy as np

import emu_binding
from emu_binding import aligned
from helpers import abi

# lsim_eval field -> (dtype, per-env shape) of the simulator buffers and per-env constants
FIELDS = {"rew": (np.float32, ()), "reset_buf": (np.uint8, ()), "time_out_buf": (np.uint8, ()), "commands": (np.float32, (4,)),
          "base_lin_vel": (np.float32, (3,)), "base_ang_vel": (np.float32, (3,)), "root_states": (np.float32, (13,)), "dof_state": (np.float32, (12, 2)),
          "torques": (np.float32, (12,)), "actions": (np.float32, (12,)), "last_actions": (np.float32, (12,)), "contact_filt": (np.uint8, (4,)),
          "contact_forces": (np.float32, (17, 3)), "terrain_types": (np.int64, ()), "terrain_levels": (np.int64, ()),
          "robot_ids": (np.uint8, ()), "torque_limits": (np.float32, (12,)), "default_dof_pos": (np.float32, (12,)), "action_scale": (np.float32, (12,))}


def lib():
    L = emu_binding.shim("eval")
    L.emu_eval_accumulate_ordered.argtypes = [ctypes.POINTER(abi.LsimEval), ctypes.c_void_p]       # test-only: the env order permutation
    return L


def EmuApi():
    """lsim_eval_sizes / _clear / _accumulate of the shim, for learn.evaluate.Evaluator(api=...)"""
    return emu_binding.api("eval")


class EmuEval:
    """the evaluator over numpy arrays: `.bufs[name]` are the input arrays to fill before each `.accumulate()`"""

    def __init__(self, N, num_robots, num_types, num_levels, group_by, trace_envs=(), trace_capacity=1, feet_bodies=(4, 8, 12, 16), with_robot_ids=True):
        L = lib()
        self.N = N
        self.bufs = {k: aligned((N,) + shp, dt) for k, (dt, shp) in FIELDS.items()}
        groups = (num_robots if group_by & 1 else 1) * (num_types if group_by & 2 else 1) * (num_levels if group_by & 4 else 1)
        sb, tb, rb = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        assert L.emu_eval_sizes(N, groups, len(trace_envs), trace_capacity, ctypes.byref(sb), ctypes.byref(tb), ctypes.byref(rb)) == 0
        assert tb.value == groups * abi.NUM_EVAL_WORDS * 8 and rb.value == trace_capacity * len(trace_envs) * abi.DEFINES["LSIM_EVAL_TRACE_DIM"] * 4
        self.state = aligned((sb.value,), np.uint8)
        self.table = aligned((groups, abi.NUM_EVAL_WORDS), np.int64)
        self.trace = aligned((trace_capacity, len(trace_envs), abi.DEFINES["LSIM_EVAL_TRACE_DIM"]), np.float32)
        e = abi.LsimEval()
        for k, arr in self.bufs.items():
            if k == "robot_ids" and not with_robot_ids:
                continue
            setattr(e, k, arr.ctypes.data)
        e.state, e.table = self.state.ctypes.data, self.table.ctypes.data
        e.trace = self.trace.ctypes.data if len(trace_envs) else None
        e.num_envs, e.num_robots, e.num_types, e.num_levels, e.group_by, e.num_groups = N, num_robots, num_types, num_levels, group_by, groups
        e.num_trace_envs, e.trace_capacity = len(trace_envs), trace_capacity
        for k, b in enumerate(feet_bodies):
            e.feet_bodies[k] = b
        for k, i in enumerate(trace_envs):
            e.trace_envs[k] = i
        self.e = e
        assert L.emu_eval_clear(ctypes.byref(e), None) == 0

    def accumulate(self, order=None):
        o = None if order is None else np.ascontiguousarray(order, np.int32)
        rc = lib().emu_eval_accumulate_ordered(ctypes.byref(self.e), None if o is None else o.ctypes.data)
        assert rc == 0, rc


def emu_mixed_env(cfg, seed=3):
    """the product's LeggedRobot surface over the lane emulator of kernels A / B (tests/emu_env.py)"""
    from emu_env import EmuLeggedRobot
    return EmuLeggedRobot(cfg, seed=seed)
