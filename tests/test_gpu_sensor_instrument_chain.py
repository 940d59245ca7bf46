"""GPU: the instrument error through envs/sensors.py on a full LeggedRobot -- 64 Aliengo envs on stairs with a 64 x 48 camera at period 4
staggered, an InstrumentError together with a MountJitter, time-outs and one by-hand reset on the way -- and through a vision policy's
training step, checkpoint and evaluation."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, FAR = 64, 5.0
INSTRUMENT = dict(latency=(0, 2), noise_gain=(0.5, 2.0), depth_scale=0.02, depth_quad=0.005, fov=0.02)
COUNTED = ("lsim_sensor_mount_jitter", "lsim_sensor_instrument", "lsim_sensor_capture_inst", "lsim_sensor_capture")


def bits(t):
    return np.ascontiguousarray(t.cpu().numpy() if isinstance(t, torch.Tensor) else t, np.float32).view(np.int32)


def _env(seed, episode_length_s=None):
    from isaacgymloco_amd.envs import config as C
    from isaacgymloco_amd.envs.legged_robot import LeggedRobot
    from isaacgymloco_amd.learn.evaluate import play_cfg
    cfg = play_cfg(C.aliengo_cfg())
    cfg.env.num_envs = N
    if episode_length_s is not None:
        cfg.env.episode_length_s = episode_length_s
    cfg.terrain.num_rows, cfg.terrain.num_cols = 2, 2
    cfg.terrain.terrain_proportions = [0.0, 0.0, 0.0, 0.0, 0.5, 0.5]       # stairs up and down
    env = LeggedRobot(cfg, sim_device=DEV, seed=seed)
    env.reset()
    return env


def _instrument():
    from isaacgymloco_amd.envs import sensors
    return sensors.InstrumentError(**INSTRUMENT)


def _jitter():
    from isaacgymloco_amd.envs import sensors
    return sensors.MountJitter(pos=0.01, rot_deg=(1.0, 5.0, 1.0))


def _camera(env, api=None, **kw):
    from isaacgymloco_amd.envs import sensors
    kw.setdefault("model", sensors.SensorModel(period=4, stagger=True, latency=2, frames=2, noise=(0.01, 0.002), dropout=0.02, normalise=True))
    return sensors.depth_camera(env, 64, 48, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, near=0.05, far=FAR, api=api, **kw)


class Counting:
    """the loaded library with its sensor launches counted"""

    def __init__(self, L):
        self._L, self.calls = L, dict.fromkeys(COUNTED, 0)
        for name in COUNTED:
            setattr(self, name, self._counted(name))

    def _counted(self, name):
        def call(*a):
            self.calls[name] += 1
            return getattr(self._L, name)(*a)
        return call

    def __getattr__(self, name):
        return getattr(self._L, name)


def test_reset_envs_draw_a_new_row_and_their_history_is_rendered_under_it():
    from isaacgymloco_amd import abi
    env = _env(5)
    api = Counting(env._L)
    cam = env.add_sensor("depth", _camera(env, api, see_robot=True, instrument=_instrument(), mount_jitter=_jitter()))
    twin = _camera(env, see_robot=True)
    torch.cuda.synchronize()
    assert api.calls == {"lsim_sensor_mount_jitter": 1, "lsim_sensor_instrument": 1, "lsim_sensor_capture_inst": 1, "lsim_sensor_capture": 0}
    rows = cam.instrument_rows().cpu().numpy()
    assert set(np.unique(rows[:, 0])) == {0.0, 1.0, 2.0} and (rows[:, 1] >= 0.5).all() and (rows[:, 1] <= 2.0).all() and (rows[:, 5:] == 0).all()
    assert (np.abs(rows[:, 2]) <= 0.02).all() and (np.abs(rows[:, 3]) <= 0.005).all() and (np.abs(rows[:, 4] - 1.0) <= 0.02 + 1e-6).all()
    assert len({r.tobytes() for r in rows}) == N

    def fresh_equal_the_twin(envs, what):
        """lsim_sensor_capture_inst, FILL_ALL, on the camera's present mounts and rows, tick and stream: the whole history of a fresh env"""
        twin.mount.copy_(cam.mount)
        twin.stage("capture").struct.tick, twin.stage("capture").struct.flags, twin.stage("capture").struct.stream_id = cam.tick, abi.DEFINES["LSIM_SENSOR_FILL_ALL"], cam.stream_id
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert env._L.lsim_sensor_capture_inst(ctypes.byref(twin.stage("capture").struct), cam.instrument_rows().data_ptr(), stream) == 0
        torch.cuda.synchronize()
        np.testing.assert_array_equal(bits(cam.history())[envs], bits(twin.history())[envs], err_msg=what)

    fresh_equal_the_twin(np.arange(N), "add_sensor")
    k = torch.arange(N, device=DEV) % 16
    near_end = torch.where((k >= 3) & (k <= 6), int(env.max_episode_length) - 2 - k, torch.full_like(k, 5))
    env.episode_length_buf = near_end.to(env.episode_length_buf.dtype)
    g = torch.Generator().manual_seed(2)
    resets = 0
    for step in range(12):
        if step == 6:                           # a reset by hand between two steps
            before = cam.instrument_rows().clone()
            env.reset_idx([2, 9])
            torch.cuda.synchronize()
            fresh = (env.episode_length_buf == 0).cpu().numpy()
            assert fresh[[2, 9]].all()
            np.testing.assert_array_equal((bits(cam.instrument_rows()) != bits(before)).any(axis=1), fresh)
            fresh_equal_the_twin(np.nonzero(fresh)[0], "reset_idx by hand")
        before, hist_b, tick = cam.instrument_rows().clone(), cam.history().clone(), env.common_step_counter
        env.step_device((torch.randn(N, 12, generator=g) * 0.5).to(DEV))
        torch.cuda.synchronize()
        reset = env.reset_buf.cpu().numpy().astype(bool)
        changed = (bits(cam.instrument_rows()) != bits(before)).any(axis=1)
        np.testing.assert_array_equal(changed, reset, err_msg=f"step {step}")
        fresh_equal_the_twin(np.nonzero(reset)[0], f"step {step}")
        due = reset | ((tick + np.arange(N)) % 4 == 0)
        np.testing.assert_array_equal(bits(cam.history())[~due], bits(hist_b)[~due])
        assert (bits(cam.history())[due] != bits(hist_b)[due]).any(axis=(1, 2)).all()
        resets += int(reset.sum())
    assert resets >= 16, "the time-outs happened"
    assert api.calls == {"lsim_sensor_mount_jitter": 14, "lsim_sensor_instrument": 14, "lsim_sensor_capture_inst": 14, "lsim_sensor_capture": 0}
    assert int(cam.nonfinite_rays) == 0 and int(twin.nonfinite_rays) == 0 and int(env.nonfinite_envs) == 0
    assert bool(torch.isfinite(cam.history()).all())


def _runner(env):
    from isaacgymloco_amd.learn.bench_train import train_cfg_dict
    from isaacgymloco_amd.learn.depth_encoder import DepthEncoder
    from isaacgymloco_amd.learn.vision import VisionOnPolicyRunner
    tc = train_cfg_dict("aliengo")
    tc["runner"]["num_steps_per_env"] = 6
    torch.manual_seed(5)
    return VisionOnPolicyRunner(env, tc, sensor="depth", encoder=DepthEncoder(48, 64, 2), device=DEV)


def test_train_save_and_evaluate_with_the_recorded_instrument(tmp_path):
    from isaacgymloco_amd.envs import sensors
    from isaacgymloco_amd.learn.evaluate import evaluate
    env = _env(5, episode_length_s=0.3)
    api = Counting(env._L)
    cam = env.add_sensor("depth", _camera(env, api, instrument=_instrument()))
    run = _runner(env)
    run.learn(1)
    torch.cuda.synchronize()
    assert api.calls["lsim_sensor_instrument"] == api.calls["lsim_sensor_capture_inst"] >= 1 + 6 and api.calls["lsim_sensor_capture"] == 0
    path = str(tmp_path / "model.pt")
    run.save(path)
    record = torch.load(path, map_location="cpu", weights_only=False)["vision"]["sensor"]
    assert record["instrument"] == _instrument().record() and record == cam.spec()
    wide = sensors.InstrumentError(latency=(0, 2), noise_gain=(1.0, 4.0), depth_scale=0.05, depth_quad=0.01, fov=0.05)
    blank = {"latency": None, "noise_gain": None, "depth_scale": None, "depth_quad": None, "fov": None}
    results = {}
    for choice in ("trained", None, wide):
        env2 = _env(9, episode_length_s=0.3)
        cam2 = env2.add_sensor("depth", sensors.from_spec(env2, record))          # as the command line builds it
        assert cam2.instrument == _instrument()
        res = evaluate(env2, path, 20, commands=(0.8, 0.0, 0.0), camera_instrument=choice).result()
        torch.cuda.synchronize()
        tot = res["total"]
        assert res["steps"] == 20 and tot["episodes"] > 0 and tot["samples"] > 0
        for v in [tot[m] for m in ("fall_rate", "lin_vel_error_rms", "episode_return_mean")] + [c["mean"] for c in tot["columns"].values()]:
            assert np.isfinite(v)
        assert all(c["nonfinite"] == 0 for c in tot["columns"].values()) and res["nonfinite"] == {"addends": 0, "simulator_env_steps": 0}
        assert int(cam2.nonfinite_rays) == 0 and bool(torch.isfinite(cam2.latent()).all())
        entry = res["conventions"]["camera_instrument"]
        if choice == "trained":
            assert entry == dict(_instrument().record(), choice="trained") and cam2.instrument == _instrument()
        elif choice is None:
            assert entry == dict(blank, choice="off") and cam2.instrument is None and cam2.stage("instrument") is None
        else:
            assert entry == dict(wide.record(), choice="override") and cam2.instrument == wide
            assert float(cam2.instrument_rows()[:, 2].abs().max()) > 0.02
        results[entry["choice"]] = res
    assert results["trained"]["total"]["columns"] != results["off"]["total"]["columns"], "the instrument error reaches the policy's inputs"


def test_a_runner_whose_camera_has_no_instrument_launches_neither_kernel():
    env = _env(5, episode_length_s=0.3)
    api = Counting(env._L)
    cam = env.add_sensor("depth", _camera(env, api))
    run = _runner(env)
    run.learn(1)
    torch.cuda.synchronize()
    assert api.calls["lsim_sensor_instrument"] == api.calls["lsim_sensor_capture_inst"] == 0 and api.calls["lsim_sensor_capture"] >= 1 + 6
    assert cam.instrument is None and cam.stage("instrument") is None and "instrument" not in cam.spec()
