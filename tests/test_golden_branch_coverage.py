"""The config-branch fixtures (tests/golden/step_aliengo_{ctrl_v,ctrl_t,dr_off,curricula_off,plane_allterms_inside}.npz, captured from the
reference's own LeggedRobot.step() by tools/gen_golden.py) really take the branch they are there to pin.  Reads the fixtures only: every
condition is a property of the reference's outputs, so a regenerated fixture that no longer exercises its branch fails here, not silently."""
import numpy as np
import pytest

import golden_replay as GR
from helpers import abi


def _counters(fx):
    return fx["in_counter_before"] + 1          # common_step_counter as the step's own code sees it (LR:194)


def _resets(fx):
    return fx["out_term_mask"].astype(bool)     # [T, N]: the envs reset_idx ran for


@pytest.mark.parametrize("name", ["aliengo_ctrl_v", "aliengo_ctrl_t"])
def test_control_law_fixtures_are_not_saturated(name):
    fx = GR.load(name)
    tau, lim = fx["out_substep_torques"], fx["torque_limits"]
    on = np.abs(tau) == lim
    inside = np.abs(tau) < lim
    assert np.all(on | inside)
    print(name, f"inside {inside.mean():.3f}, on a limit {on.mean():.3f}")
    assert inside.mean() >= 0.5, "a saturated fixture pins the clip, not the law"
    assert on.mean() >= 0.05, "the clip of LR:688 is exercised"
    if name == "aliengo_ctrl_v":    # the kd term is live: the joint speeds the law reads differ from the ones the previous step left in last_dof_vel
        differs = fx["out_last_dof_vel"][:-1] != fx["in_dof"][1:, :, :, 1]
        print(name, f"last_dof_vel != dof_vel in {differs.mean():.3f} of the entries")
        assert differs.mean() >= 0.9


def test_dr_off_fixture_takes_the_off_branches():
    fx = GR.load("aliengo_dr_off")
    cnt, rst = _counters(fx), _resets(fx)
    assert (cnt % 8 == 0).any() and (cnt % 500 == 0).any() and (cnt % 800 == 0).any()
    assert (fx["out_time_out"].astype(bool) & rst).any(), "a time-out reset"
    later = np.arange(len(cnt)) >= 1            # step 0 follows the start-up reset_idx(all)
    assert rst[later].any()
    for k in ("kp_factors", "kd_factors", "friction"):      # LR:336-339, LR:534: not redrawn
        assert np.all(fx["out_" + k] == fx["out_" + k][0]), k
    res = fx["out_restitution"]
    changed = res[1:] != res[:-1]
    assert changed[rst[1:]].all() and not changed[~rst[1:]].any(), "restitution is redrawn on reset (LR:536), and only there"
    assert not fx["out_delay_steps"].any() and not fx["out_delay_on"].any()
    np.testing.assert_array_equal(fx["out_delayed_actions"], np.repeat(np.clip(fx["in_actions"], -100, 100)[:, :, None, :], 4, axis=2))   # LR:133
    assert not fx["out_extras_time_outs"].any(), "extras['time_outs'] is never written (LR:358)"
    # no push (LR:627), no disturbance (LR:631): the injected base velocity comes back untouched unless the env was reset, and the
    # disturbance columns of the privileged observation (LR:397: 48:51 of the newest frame) stay zero
    keep = ~rst
    np.testing.assert_array_equal(fx["out_root_states"][keep][:, 7:9], fx["in_root"][keep][:, 7:9])
    assert not fx["out_priv_obs"][:, :, 48:51].any()
    # add_noise off (LR:393): the newest frame's first 45 entries are the clean values; 9:21 is dof_pos - default scaled by 1 -> check through dof_vel (21:33, x 0.05)
    np.testing.assert_allclose(fx["out_obs"][:, :, 21:33], fx["out_dof_state"][:, :, :, 1] * 0.05, rtol=1e-6, atol=1e-7)


def test_curricula_off_fixture_takes_the_off_branches():
    fx = GR.load("aliengo_curricula_off")
    cnt, rst = _counters(fx), _resets(fx)
    t = int(np.flatnonzero(cnt % 1000 == 0)[0])
    assert rst[t].any()
    cfg = GR.scenario_cfg("aliengo_curricula_off")
    # LR:875: mean(episode_sums) / max_episode_length > 0.8 * scale * dt, on every env (the override sets them all)
    assert fx["in_track_override"][t] / 1000.0 > 0.8 * cfg.rewards.scales.tracking_lin_vel * 0.02
    np.testing.assert_array_equal(fx["out_command_ranges"][t], fx["out_command_ranges"][0])
    assert np.all(fx["out_command_ranges"] == fx["out_command_ranges"][0])
    lv = fx["out_terrain_levels"]
    assert np.all(lv == lv[0]) and rst[1:].any(), "terrain_levels unchanged by every reset (LR:302)"
    assert not fx["out_commands"][:, :, 3].any(), "commands[:, 3] is never drawn with heading_command off (LR:643-646)"
    yaw = fx["out_commands"][:, :, 2]
    assert (yaw[1:] != yaw[:-1])[rst[1:]].all() and np.abs(yaw).max() <= 1.0, "the yaw-rate command is drawn instead (LR:646)"


def test_plane_fixture_takes_the_plane_branches():
    fx = GR.load("aliengo_plane_allterms_inside")
    assert "height_grid" not in fx.files
    assert not fx["out_measured_heights"].any()             # LR:1331-1332
    es = fx["out_episode_sums"]
    for nm in ("base_height", "foot_clearance_terrain", "foot_clearance_terrain_up"):    # LR:1370, LR:1719, LR:1746
        assert np.abs(es[:, :, abi.REWARD_IDS[nm]]).max() > 0, nm
    org = fx["init_env_origins"]                            # LR:1243-1250: ceil(16 / 4) x 4 grid, env.env_spacing apart
    np.testing.assert_array_equal(fx["out_env_origins"], np.broadcast_to(org, fx["out_env_origins"].shape))
    assert len({tuple(r) for r in org[:, :2]}) == len(org) and not org[:, 2].any()
    assert _resets(fx)[1:].any()
