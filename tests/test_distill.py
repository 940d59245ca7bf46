"""CPU: lsim_distill_loss (isaacgymloco_amd/csrc/ls_distill.h) through its shim tests/emu/emu_distill.cpp -- the header's own validation,
chunking and per-item functions compiled by g++ -- against the numpy statement of tests/distill_reference.py.
tests/test_gpu_distill.py runs the same checks on the HIP library."""
import ctypes

import pytest

import distill_emu_binding as DB
import distill_reference as R
from helpers import abi


def test_the_prototype_and_the_struct_are_the_headers():
    assert abi.PROTOTYPES["lsim_distill_loss"] == (ctypes.c_int, [ctypes.POINTER(abi.LsimDistillLoss), ctypes.c_void_p])
    names = [f[0] for f in abi.LsimDistillLoss._fields_]
    assert names == ["mu", "target", "index", "g", "partial", "batch", "actions", "target_rows", "mu_stride", "target_stride", "g_stride", "scale"]
    assert abi.ABI_VERSION == 7


def test_the_cases_reach_both_paths():
    paths = {(actions, pad): R.make_case("one", actions, pad)[4] for _, actions, pad in R.cases()}
    assert paths == {(12, 0): True, (12, 4): True, (12, 3): False, (13, 0): False, (13, 3): False, (1, 0): False, (1, 3): False}


@pytest.mark.parametrize("kind,actions,pad", R.cases())
def test_the_gradient_is_the_fp32_statement_and_the_sums_are_within_the_bound(kind, actions, pad):
    DB.check_case(DB.Rig, kind, actions, pad)


def test_bad_arguments_are_refused_untouched():
    DB.check_refusals(DB.Rig, lambda: DB.lib().emu_distill_loss(None, None))
