"""CPU: the two launches of isaacgymloco_amd/csrc/ls_frames_log.h through their shim (tests/emu/emu_frames_log.cpp: the same validation and
per-env / per-row / per-column functions the HIP kernels call) against the numpy references of tests/frames_log_reference.py.
tests/test_gpu_frames_log.py runs the same checks on the device."""
import numpy as np
import pytest

import frames_log_emu_binding as FB
import frames_log_reference as R


@pytest.mark.parametrize("N", R.SIZES)
def test_the_frame_log_is_the_state_machine(N):
    FB.check_scenario(FB.Rig, N)


def test_a_row_whose_pixels_are_no_multiple_of_four():
    rig, ref = FB.check_scenario(FB.Rig, 70, pixels=10)
    log = rig.read()[0][:int(ref.state[R.COUNT])]
    assert (log[:, :, 10:] == 0.0).all() and (log[:, :, :10] != 0.0).all()


def test_envs_that_are_not_visited_get_no_row():
    N, cap = 10, 40
    rig = FB.Rig(N, cap, env_stride=3)
    ref = R.FramesLog(N, R.STEPS, cap, R.FRAMES, R.PIXELS, R.ROW_STRIDE, R.PERIOD, 1, env_stride=3, log_fill=FB.LOG_FILL, int_fill=FB.INT_FILL)
    for call in R.launches(N):
        ref.launch(*call)
        assert rig.launch(*call) == 0
    log, row_of, row_src, state = rig.read()
    assert np.array_equal(row_of, ref.row_of) and np.array_equal(row_src, ref.row_src) and np.array_equal(state, ref.state)
    assert np.array_equal(log.view(np.uint32), ref.log.view(np.uint32))
    assert (row_of[:, np.arange(N) % 3 != 0] == -1).all() and (row_of[:, ::3] >= 0).all()


def test_the_frame_log_refuses_bad_arguments_untouched():
    FB.check_refusals(FB.Rig, lambda: FB.lib().emu_sensor_frames_log(None, None))


@pytest.mark.parametrize("latent_dim", [1, 64, 80])
@pytest.mark.parametrize("N", [8, 70])
def test_gradient_rows_are_the_sequential_sum(N, latent_dim):
    FB.check_grad(FB.GradRig, N, latent_dim, null_call=(lambda: FB.lib().emu_latent_rows_grad(None, None)) if N == 8 else None)
