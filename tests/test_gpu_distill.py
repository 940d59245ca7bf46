"""GPU: lsim_distill_loss (isaacgymloco_amd/csrc/ls_distill.h) on a real device: the checks of tests/test_distill.py -- the numpy fp32
statement bit for bit, the sums within the header's bound, refusals that write nothing -- on the HIP library."""
import pytest

import distill_emu_binding as DB
import distill_reference as R
from isaacgymloco_amd import lib

pytestmark = pytest.mark.gpu


def hip_rig(*a, **kw):
    return DB.Rig(*a, device="cuda:0", entry=lib.load().lsim_distill_loss, **kw)


@pytest.mark.parametrize("kind,actions,pad", R.cases())
def test_the_gradient_is_the_fp32_statement_and_the_sums_are_within_the_bound(kind, actions, pad):
    DB.check_case(hip_rig, kind, actions, pad)


def test_bad_arguments_are_refused_untouched():
    DB.check_refusals(hip_rig, lambda: lib.load().lsim_distill_loss(None, None))
