"""GPU: lsim_sensor_frames_log and lsim_latent_rows_grad (isaacgymloco_amd/csrc/ls_frames_log.h) on a real device: the checks of
tests/test_frames_log.py -- the numpy state machine and the sequential fp32 sum, exact equality -- on the HIP library."""
import pytest

import frames_log_emu_binding as FB
import frames_log_reference as R
from isaacgymloco_amd import lib

pytestmark = pytest.mark.gpu


def hip_rig(*a, **kw):
    return FB.Rig(*a, device="cuda:0", entry=lib.load().lsim_sensor_frames_log, **kw)


def hip_grad_rig(*a, **kw):
    return FB.GradRig(*a, device="cuda:0", entry=lib.load().lsim_latent_rows_grad, **kw)


@pytest.mark.parametrize("N", R.SIZES)
def test_the_frame_log_is_the_state_machine(N):
    FB.check_scenario(hip_rig, N)


def test_a_row_whose_pixels_are_no_multiple_of_four():
    FB.check_scenario(hip_rig, 70, pixels=10)


def test_the_frame_log_refuses_bad_arguments_untouched():
    FB.check_refusals(hip_rig, lambda: lib.load().lsim_sensor_frames_log(None, None))


@pytest.mark.parametrize("latent_dim", [1, 64, 80])
@pytest.mark.parametrize("N", [8, 70])
def test_gradient_rows_are_the_sequential_sum(N, latent_dim):
    FB.check_grad(hip_grad_rig, N, latent_dim, null_call=(lambda: lib.load().lsim_latent_rows_grad(None, None)) if N == 8 else None)
