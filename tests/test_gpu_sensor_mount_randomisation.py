"""GPU: the mount jitter through envs/sensors.py on a full LeggedRobot -- 64 Aliengo envs on stairs with a 64 x 48 camera, time-outs on the
way -- and through a vision policy's training step, checkpoint and evaluation."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, FAR = 64, 5.0


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


def _jitter():
    from isaacgymloco_amd.envs import sensors
    return sensors.MountJitter(pos=0.01, rot_deg=(1.0, 5.0, 1.0))


def _camera(env, api=None, **kw):
    from isaacgymloco_amd.envs import sensors
    kw.setdefault("model", sensors.SensorModel(period=4, stagger=True, latency=1, frames=2, clip=(0.0, FAR)))     # the identity on a clean depth
    return sensors.depth_camera(env, 64, 48, 87.0, mount_pos=kw.pop("mount_pos", (0.3, 0.0, 0.05)), pitch_deg=30.0, near=0.05, far=FAR, api=api, **kw)


class Counting:
    """the loaded library with its jitter launches counted"""

    def __init__(self, L):
        self._L, self.jitter_launches = L, 0

    def __getattr__(self, name):
        return getattr(self._L, name)

    def lsim_sensor_mount_jitter(self, *a):
        self.jitter_launches += 1
        return self._L.lsim_sensor_mount_jitter(*a)


def test_reset_envs_get_a_new_mount_and_their_history_is_rendered_from_it():
    env = _env(5)
    api = Counting(env._L)
    cam = env.add_sensor("depth", _camera(env, api, see_robot=True, mount_jitter=_jitter()))
    twin = _camera(env, see_robot=True, model=None, mount_pos=cam.mount[:, :3])
    torch.cuda.synchronize()
    assert api.jitter_launches == 1 and (bits(cam.mount) != bits(cam.mount_nominal)).any(axis=1).all()
    assert float((cam.mount[:, :3] - cam.mount_nominal[:, :3]).abs().max()) <= 0.01 + 1e-7

    def twin_equals(envs, what):
        twin.mount.copy_(cam.mount)
        want = twin.update().cpu().numpy()
        hist = cam.history().cpu().numpy()[:, :, :cam.num_rays]
        for k in range(hist.shape[1]):
            np.testing.assert_array_equal(bits(hist[envs, k]), bits(want[envs]), err_msg=f"{what}: slot {k}")
        return want

    twin_equals(np.arange(N), "add_sensor")
    k = torch.arange(N, device=DEV) % 16
    near_end = torch.where((k >= 3) & (k <= 6), int(env.max_episode_length) - 2 - k, torch.full_like(k, 5))
    env.episode_length_buf = near_end.to(env.episode_length_buf.dtype)
    g = torch.Generator().manual_seed(2)
    resets = 0
    for step in range(12):
        before, hist_b, tick = cam.mount.clone(), cam.history().clone(), env.common_step_counter
        env.step_device((torch.randn(N, 12, generator=g) * 0.5).to(DEV))
        torch.cuda.synchronize()
        reset = env.reset_buf.cpu().numpy().astype(bool)
        changed = (bits(cam.mount) != bits(before)).any(axis=1)
        np.testing.assert_array_equal(changed, reset, err_msg=f"step {step}")
        np.testing.assert_array_equal(bits(cam.mount)[~reset], bits(before)[~reset])
        clean = twin_equals(np.nonzero(reset)[0], f"step {step}")
        due = reset | ((tick + np.arange(N)) % 4 == 0)
        hist = cam.history().cpu().numpy()
        np.testing.assert_array_equal(bits(hist[due, -1, :cam.num_rays]), bits(clean[due]))
        np.testing.assert_array_equal(bits(hist[~due]), bits(hist_b)[~due])
        resets += int(reset.sum())
    assert resets >= 16, "the time-outs happened"
    assert api.jitter_launches == 13
    assert int(cam.nonfinite_rays) == 0 and int(twin.nonfinite_rays) == 0 and int(env.nonfinite_envs) == 0


def _runner(env):
    from isaacgymloco_amd.learn.bench_train import train_cfg_dict
    from isaacgymloco_amd.learn.depth_encoder import DepthEncoder
    from isaacgymloco_amd.learn.vision import VisionOnPolicyRunner
    tc = train_cfg_dict("aliengo")
    tc["runner"]["num_steps_per_env"] = 6
    torch.manual_seed(5)
    return VisionOnPolicyRunner(env, tc, sensor="depth", encoder=DepthEncoder(48, 64, 2), device=DEV)


def test_train_save_and_evaluate_with_the_recorded_jitter(tmp_path):
    from isaacgymloco_amd.envs import sensors
    from isaacgymloco_amd.learn.evaluate import evaluate
    env = _env(5, episode_length_s=0.3)
    api = Counting(env._L)
    cam = env.add_sensor("depth", _camera(env, api, mount_jitter=_jitter(), model=sensors.SensorModel(period=4, stagger=True, latency=1, frames=2, normalise=True)))
    run = _runner(env)
    run.learn(1)
    torch.cuda.synchronize()
    assert api.jitter_launches >= 1 + 6 and (bits(cam.mount) != bits(cam.mount_nominal)).any(axis=1).all()
    path = str(tmp_path / "model.pt")
    run.save(path)
    record = torch.load(path, map_location="cpu", weights_only=False)["vision"]["sensor"]
    assert record["mount_jitter"] == {"pos": [0.01] * 3, "rot_deg": [1.0, 5.0, 1.0]} and record == cam.spec()
    results = {}
    for choice in ("trained", None):
        env2 = _env(9, episode_length_s=0.3)
        cam2 = env2.add_sensor("depth", sensors.from_spec(env2, record))          # as the command line builds it
        assert cam2.mount_jitter == _jitter() and torch.equal(cam2.mount_nominal, cam.mount_nominal)
        res = evaluate(env2, path, 20, commands=(0.8, 0.0, 0.0), camera_jitter=choice).result()
        torch.cuda.synchronize()
        tot = res["total"]
        assert res["steps"] == 20 and tot["episodes"] > 0 and tot["samples"] > 0
        for v in [tot[m] for m in ("fall_rate", "lin_vel_error_rms", "episode_return_mean")] + [c["mean"] for c in tot["columns"].values()]:
            assert np.isfinite(v)
        assert all(c["nonfinite"] == 0 for c in tot["columns"].values()) and res["nonfinite"] == {"addends": 0, "simulator_env_steps": 0}
        assert int(cam2.nonfinite_rays) == 0 and bool(torch.isfinite(cam2.latent()).all())
        results[choice] = res
        if choice == "trained":
            assert res["conventions"]["camera_jitter"] == {"choice": "trained", "pos": [0.01] * 3, "rot_deg": [1.0, 5.0, 1.0]}
            assert cam2.mount_jitter == _jitter() and (bits(cam2.mount) != bits(cam2.mount_nominal)).any(axis=1).all()
        else:
            assert res["conventions"]["camera_jitter"] == {"choice": "off", "pos": None, "rot_deg": None}
            assert cam2.mount_jitter is None and cam2.mount is cam2.mount_nominal
    assert results["trained"]["total"]["columns"] != results[None]["total"]["columns"], "the mount error reaches the policy's inputs"


def test_a_runner_whose_camera_has_no_jitter_launches_no_jitter_kernel():
    env = _env(5, episode_length_s=0.3)
    api = Counting(env._L)
    cam = env.add_sensor("depth", _camera(env, api))
    run = _runner(env)
    run.learn(1)
    torch.cuda.synchronize()
    assert api.jitter_launches == 0 and cam.mount is cam.mount_nominal and "mount_jitter" not in cam.spec()
