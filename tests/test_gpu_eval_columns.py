"""GPU: lsim_eval_columns_accumulate on a real device against the CPU build of the same kernel source (tests/emu/emu_eval_columns.cpp), which
tests/test_eval_columns.py pins to the semantics of include/lsim.h: the int64 tables equal, bit for bit, and equal again on a second run."""
import ctypes

import numpy as np
import pytest

import eval_columns_emu_binding as CB
import eval_emu_binding as EE
from helpers import abi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W = abi.EVAL_WORDS


class DeviceRig:
    """CB.Rig's twin in device memory, launched through the HIP library: the evaluator's struct and the columns' struct over torch tensors"""

    def __init__(self, N, num_cols, ld, big):
        import torch
        from isaacgymloco_amd import lib
        self.L, self.N = lib.load(), N
        self.bufs = {k: torch.zeros((N,) + shp, dtype=getattr(torch, np.dtype(dt).name), device=DEV) for k, (dt, shp) in EE.FIELDS.items()}
        self.bufs["torque_limits"] += 1.0
        by = 7 if big else 0
        groups = CB.R_BIG * CB.T_BIG * CB.L_BIG if big else 1
        sb, tb, rb = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        assert self.L.lsim_eval_sizes(N, groups, 0, 1, ctypes.byref(sb), ctypes.byref(tb), ctypes.byref(rb)) == 0
        self.state = torch.zeros(sb.value // 8, dtype=torch.int64, device=DEV)
        self.main = torch.zeros(groups, abi.NUM_EVAL_WORDS, dtype=torch.int64, device=DEV)
        e = abi.LsimEval()
        for k, t in self.bufs.items():
            setattr(e, k, t.data_ptr())
        e.state, e.table, e.trace = self.state.data_ptr(), self.main.data_ptr(), None
        e.num_envs, e.num_robots, e.num_types, e.num_levels, e.group_by, e.num_groups = N, CB.R_BIG, CB.T_BIG, CB.L_BIG, by, groups
        e.num_trace_envs, e.trace_capacity = 0, 1
        for k, b in enumerate((4, 8, 12, 16)):
            e.feet_bodies[k] = b
        self.e = e
        self.values = torch.zeros(N, ld, dtype=torch.float32, device=DEV)
        # a guard row behind the table: a write past the last group would show
        self.flat = torch.zeros((groups + 1) * (1 + CB.COL_WORDS * num_cols), dtype=torch.int64, device=DEV)
        self.table = self.flat[:groups * (1 + CB.COL_WORDS * num_cols)].view(groups, -1)
        c = abi.LsimEvalColumns()
        c.state, c.reset_buf, c.values, c.table = self.state.data_ptr(), self.bufs["reset_buf"].data_ptr(), self.values.data_ptr(), self.table.data_ptr()
        c.num_envs, c.num_groups, c.num_cols, c.ld = N, groups, num_cols, ld
        self.c = c
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert self.L.lsim_eval_clear(ctypes.byref(e), self.stream) == 0
        self.flat[-(1 + CB.COL_WORDS * num_cols):] = 777
        self.table[...] = 555                                                     # clear() zeroes the table and only the table
        assert self.L.lsim_eval_columns_clear(ctypes.byref(c), self.stream) == 0

    def step(self, s):
        import torch
        for k in ("reset_buf", "terrain_levels", "terrain_types", "robot_ids"):
            self.bufs[k].copy_(torch.from_numpy(s[k]))
        self.values.copy_(torch.from_numpy(s["values"]))
        assert self.L.lsim_eval_accumulate(ctypes.byref(self.e), self.stream) == 0
        assert self.L.lsim_eval_columns_accumulate(ctypes.byref(self.c), self.stream) == 0


def device_run(N, num_cols, ld, big):
    import torch
    steps, _ = CB.script(N, num_cols, ld, big)
    rig = DeviceRig(N, num_cols, ld, big)
    for s in steps:
        rig.step(s)
    torch.cuda.synchronize()
    assert (rig.flat[rig.table.numel():] == 777).all()
    return rig.table.cpu().numpy().copy(), rig.main.cpu().numpy().copy()


def shim_run(N, num_cols, ld, big):
    steps, _ = CB.script(N, num_cols, ld, big)
    rig = CB.Rig(N, num_cols, ld, big)
    for s in steps:
        rig.feed(s)
        rig.ev.accumulate()
        rig.accumulate_columns()
    return rig.table.copy(), rig.ev.table.copy()


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("num_cols,ld", [(1, 1), (6, 9)])
@pytest.mark.parametrize("N", [1, 257, 700])
def test_device_table_equals_the_cpu_build_of_the_kernel_source(N, num_cols, ld, big):
    want, want_main = shim_run(N, num_cols, ld, big)
    got, main = device_run(N, num_cols, ld, big)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got[:, 0], main[:, W["samples"]])
    np.testing.assert_array_equal(main[:, W["samples"]], want_main[:, W["samples"]])
    if N > 1:
        assert got[:, 3::3].sum() > 0 and got[:, 1::3].any()                       # non-finite values and sums both present
    again, _ = device_run(N, num_cols, ld, big)
    np.testing.assert_array_equal(again, got)


def test_launch_before_the_first_evaluator_launch_adds_nothing():
    import torch
    steps, _ = CB.script(257, 6, 6, True)
    rig = DeviceRig(257, 6, 6, True)
    rig.values.copy_(torch.from_numpy(steps[0]["values"]))
    assert rig.L.lsim_eval_columns_accumulate(ctypes.byref(rig.c), rig.stream) == 0
    torch.cuda.synchronize()
    assert not rig.table.any()
