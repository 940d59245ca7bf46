"""CPU: the mount jitter through the Python surface (envs/sensors.py MountJitter, RaySensor(mount_jitter=...), spec() / from_spec(), the
vision checkpoint's record and evaluate(camera_jitter=...)) on the emulated LeggedRobot, every launch through the CPU builds of the kernel
sources.  The launch itself is held to its reference in tests/test_sensor_mount_jitter.py."""
import math

import numpy as np
import pytest
import torch

import eval_columns_emu_binding as CB
import sensor_mount_jitter_emu_binding as MB
import sensor_mount_jitter_reference as MR
from helpers import C
from isaacgymloco_amd.envs import sensors
from isaacgymloco_amd.learn.depth_encoder import DepthEncoder

FAR = 5.0
JITTER = dict(pos=0.01, rot_deg=(1.0, 5.0, 1.0))
MODEL = dict(period=3, stagger=True, latency=1, frames=2, clip=(0.0, FAR))       # clean depth lies in [0, far]: the model is the identity, exactly
ENC = dict(c1=4, k1=3, s1=2, c2=8, k2=3, s2=1, latent_dim=10)
COUNTS0 = {"lsim_raycast": 0, "lsim_raycast_bodies": 0, "lsim_sensor_capture": 0, "lsim_sensor_mount_jitter": 0}


def bits(t):
    return np.ascontiguousarray(t.numpy() if isinstance(t, torch.Tensor) else t, np.float32).view(np.int32)


def _env(N=8, seed=3, mixed=False):
    from emu_env import EmuLeggedRobot
    from isaacgymloco_amd.learn.evaluate import play_cfg
    cfg = play_cfg(C.mixed_cfg("aliengo", {"aliengo": 0.5, "go2": 0.5})[0] if mixed else C.aliengo_cfg())
    cfg.env.num_envs = N
    cfg.terrain.num_rows, cfg.terrain.num_cols = 2, 2
    cfg.terrain.terrain_proportions = [0.0, 0.0, 0.0, 0.0, 0.5, 0.5]
    env = EmuLeggedRobot(cfg, seed=seed)
    env.reset()
    return env


def _camera(env, api, w=8, h=6, **kw):
    kw.setdefault("model", sensors.SensorModel(**MODEL))
    return sensors.depth_camera(env, w, h, 87.0, mount_pos=kw.pop("mount_pos", (0.3, 0.0, 0.05)), pitch_deg=30.0, near=0.05, far=FAR, api=api, **kw)


def test_mount_jitter_values():
    j = sensors.MountJitter(pos=0.01, rot_deg=(1, 5, 1))
    assert j.pos == (0.01, 0.01, 0.01) and j.rot_deg == (1.0, 5.0, 1.0) and j.record() == {"pos": [0.01] * 3, "rot_deg": [1.0, 5.0, 1.0]}
    assert sensors.MountJitter(**j.record()) == j and sensors.MountJitter() != j and sensors.MountJitter().pos == (0.0, 0.0, 0.0)
    for bad in (dict(pos=-0.01), dict(rot_deg=(1, -1, 1)), dict(pos=math.nan), dict(rot_deg=math.inf), dict(pos=(1, 2))):
        with pytest.raises(ValueError):
            sensors.MountJitter(**bad)


def test_without_a_jitter_nothing_is_launched_and_the_spec_is_the_one_of_before():
    env, api = _env(), MB.EmuApi()
    cam = env.add_sensor("depth", _camera(env, api))
    g = torch.Generator().manual_seed(0)
    for _ in range(3):
        env.step_device(torch.randn(8, 12, generator=g) * 0.3)
    env.reset_idx([1])
    assert api.calls["lsim_sensor_mount_jitter"] == 0 and api.calls["lsim_sensor_capture"] == 5
    assert cam.mount is cam.mount_nominal and cam.mount_jitter is None and cam.stage("mount_jitter") is None and cam.stage("capture").struct.rb.rc.mount == cam.mount.data_ptr()
    assert list(cam.spec()) == ["kind", "width", "height", "dirs", "scale", "near", "far", "env_stride", "see_robot", "labels", "frame", "ignore_bodies",
                                "model", "mount"]
    plain = _camera(env, api, model=None)
    assert "mount_jitter" not in plain.spec() and plain.mount is plain.mount_nominal


def test_a_jitter_needs_a_model_and_the_entry_point():
    env, api = _env(), MB.EmuApi()
    with pytest.raises(ValueError, match="model"):
        _camera(env, api, model=None, mount_jitter=sensors.MountJitter(**JITTER))
    with pytest.raises(ValueError, match="model"):
        sensors.lidar(env, 2, 20.0, 8, api=api, mount_jitter=sensors.MountJitter(**JITTER))
    with pytest.raises(TypeError):
        _camera(env, api, mount_jitter=JITTER)
    import sensor_model_emu_binding as SB
    from isaacgymloco_amd import lib
    with pytest.raises(lib.LsimError, match="lsim_sensor_mount_jitter"):
        _camera(env, SB.EmuApi(), mount_jitter=sensors.MountJitter(**JITTER))       # a library from before the entry point
    assert api.calls == COUNTS0


def _twin_equals(cam, twin, envs, what):
    """the plain ray cast from cam's present mount rows: what every slot of a just-filled history must hold (identity model), bit for bit"""
    twin.mount.copy_(cam.mount)
    want = twin.update().numpy()
    hist = cam.history().numpy()[:, :, :cam.num_rays]
    for e in envs:
        for k in range(hist.shape[1]):
            np.testing.assert_array_equal(bits(hist[e, k]), bits(want[e]), err_msg=f"{what}: env {e} slot {k}")
    return want


def test_reset_envs_get_a_new_mount_and_their_history_is_rendered_from_it():
    N = 8
    env, api = _env(N), MB.EmuApi()
    jit = sensors.MountJitter(**JITTER)
    cam = _camera(env, api, see_robot=True, mount_jitter=jit)
    assert cam.mount is not cam.mount_nominal and torch.equal(cam.mount, cam.mount_nominal) and api.calls == COUNTS0
    assert cam.stage("capture").struct.rb.rc.mount == cam.bodies_struct.rc.mount == cam.ray_struct.mount == cam.mount.data_ptr() != cam.mount_nominal.data_ptr()
    env.add_sensor("first", _camera(env, api, model=None))                  # so that the camera's stream_id is 1
    env.add_sensor("depth", cam)
    assert api.calls["lsim_sensor_mount_jitter"] == 1 and cam.stream_id == cam.stage("mount_jitter").struct.stream_id == 1
    twin = _camera(env, api, see_robot=True, model=None, mount_pos=cam.mount[:, :3])
    # add_sensor drew every env: the header's formulas on the camera's own seed, rank, stream and tick, degrees turned into radians
    nominal = cam.mount_nominal.numpy()
    rot = [math.radians(d) for d in jit.rot_deg]
    want, tol = MR.expected(nominal, nominal, np.ones(N, bool), env.lcfg.seed, env.lcfg.rank, env.common_step_counter, 1, jit.pos, rot)
    got = cam.mount.numpy()
    assert (np.abs(got - want) <= tol).all() and (bits(got) != bits(nominal)).any(axis=1).all()
    assert (np.abs(got[:, :3] - nominal[:, :3]) <= 0.01 + 1e-7).all()
    _twin_equals(cam, twin, range(N), "add_sensor")
    # time-outs on the way: env k of (1, 4, 6) ends its episode at step 1 + k // 2
    el = torch.full((N,), 5, dtype=env.episode_length_buf.dtype)
    for k in (1, 4, 6):
        el[k] = int(env.max_episode_length) - 1 - k // 2
    env.episode_length_buf = el
    g = torch.Generator().manual_seed(1)
    seen = set()
    for step in range(9):
        if step == 5:                           # a reset by hand between two steps: RESETS_ONLY, the tick of the step that follows
            before = cam.mount.clone()
            env.reset_idx([2, 5])
            changed = (bits(cam.mount) != bits(before)).any(axis=1)
            fresh = env.episode_length_buf.numpy() == 0          # 2 and 5, and whoever the step before reset: the rule is episode_length == 0,
            assert fresh[[2, 5]].all() and fresh.sum() < N       # for the capture (which refills their history again) as for the mount
            np.testing.assert_array_equal(changed, fresh)
            _twin_equals(cam, twin, np.nonzero(fresh)[0], "reset_idx by hand")
            by_hand = cam.mount.clone()
        before, hist_b, tick = cam.mount.clone(), cam.history().clone(), env.common_step_counter
        env.step_device(torch.randn(N, 12, generator=g) * 0.3)
        reset = env.reset_buf.numpy().astype(bool)
        np.testing.assert_array_equal(reset, env.episode_length_buf.numpy() == 0)
        changed = (bits(cam.mount) != bits(before)).any(axis=1)
        np.testing.assert_array_equal(changed, reset, err_msg=f"step {step}")
        np.testing.assert_array_equal(bits(cam.mount[~torch.from_numpy(reset)]), bits(before[~torch.from_numpy(reset)]))
        clean = _twin_equals(cam, twin, np.nonzero(reset)[0], f"step {step}")
        due = reset | ((tick + np.arange(N)) % 3 == 0)
        hist = cam.history().numpy()[:, :, :cam.num_rays]
        np.testing.assert_array_equal(bits(hist[due, -1]), bits(clean[due]))                       # every capture is from the present rows
        np.testing.assert_array_equal(bits(cam.history()[~torch.from_numpy(due)]), bits(hist_b[~torch.from_numpy(due)]))
        if step == 5:                           # the step that shares the by-hand reset's tick leaves those rows as they are
            np.testing.assert_array_equal(bits(cam.mount[[2, 5]]), bits(by_hand[[2, 5]]))
        seen |= set(np.nonzero(reset)[0].tolist())
    assert {1, 4, 6} <= seen, "the time-outs happened"
    assert int(cam.nonfinite_rays) == 0
    assert api.calls["lsim_sensor_mount_jitter"] == api.calls["lsim_sensor_capture"] == 1 + 9 + 1
    # back to the nominal mount, and on again
    cam.set_mount_jitter(None)
    assert cam.mount is cam.mount_nominal and cam.stage("capture").struct.rb.rc.mount == cam.mount_nominal.data_ptr() and "mount_jitter" not in cam.spec()
    calls = api.calls["lsim_sensor_mount_jitter"]
    env.step_device(torch.zeros(N, 12))
    assert api.calls["lsim_sensor_mount_jitter"] == calls


def test_spec_round_trips_the_nominal_mount_and_the_jitter():
    api = MB.EmuApi()
    jit = sensors.MountJitter(pos=(0.01, 0.02, 0.005), rot_deg=(1.0, 5.0, 2.0))
    env = _env()
    cam = env.add_sensor("depth", _camera(env, api, mount_jitter=jit))
    spec = cam.spec()
    import json
    assert json.loads(json.dumps(spec)) == spec
    assert spec["mount_jitter"] == {"pos": [0.01, 0.02, 0.005], "rot_deg": [1.0, 5.0, 2.0]}
    assert spec["mount"] == _camera(env, api).spec()["mount"] and not torch.equal(cam.mount, cam.mount_nominal)      # the nominal pose, not the drawn ones
    back = sensors.from_spec(env, spec, api=api)
    assert back.mount_jitter == jit and torch.equal(back.mount_nominal, cam.mount_nominal) and back.spec() == spec
    assert [back.stage("mount_jitter").struct.pos_range[k] for k in range(3)] == [cam.stage("mount_jitter").struct.pos_range[k] for k in range(3)]
    assert [back.stage("mount_jitter").struct.rot_range[k] for k in range(3)] == [cam.stage("mount_jitter").struct.rot_range[k] for k in range(3)] == [np.float32(math.radians(d)) for d in jit.rot_deg]
    plain = sensors.from_spec(env, spec, api=api, mount_jitter=None)
    assert plain.mount_jitter is None and plain.mount is plain.mount_nominal and "mount_jitter" not in plain.spec()
    assert plain.spec() == {k: v for k, v in spec.items() if k != "mount_jitter"}
    other = sensors.from_spec(env, spec, api=api, mount_jitter=sensors.MountJitter(pos=0.05))
    assert other.spec()["mount_jitter"] == {"pos": [0.05] * 3, "rot_deg": [0.0] * 3}
    assert sensors.from_spec(env, plain.spec(), api=api).mount_jitter is None
    with pytest.raises(ValueError):
        sensors.from_spec(env, spec, api=api, mount_jitter="trained")
    # a mount per robot on the mixed instance
    menv = _env(mixed=True)
    mounts = {"aliengo": (0.3, 0.0, 0.05), "go2": (0.25, 0.0, 0.03)}
    mcam = menv.add_sensor("depth", _camera(menv, api, mount_pos=mounts, see_robot=True, mount_jitter=jit))
    mspec = mcam.spec()
    assert set(mspec["mount"]) == {"aliengo", "go2"} and mspec["mount_jitter"] == spec["mount_jitter"]
    mback = sensors.from_spec(menv, mspec, api=api)
    assert torch.equal(mback.mount_nominal, mcam.mount_nominal) and mback.mount_jitter == jit and mback.spec() == mspec
    # a nominal mount per env: recorded as None, as before, and rebuilt with the override
    per_env = torch.zeros(8, 3)
    per_env[:, 0] = torch.arange(8) * 0.01
    odd = _camera(env, api, mount_pos=per_env, mount_jitter=jit)
    assert odd.spec()["mount"] is None and odd.spec()["mount_jitter"] == spec["mount_jitter"]
    again = sensors.from_spec(env, odd.spec(), mount_pos=per_env, mount_quat=odd.mount_nominal[0, 3:], api=api)
    assert torch.equal(again.mount_nominal, odd.mount_nominal) and again.mount_jitter == jit


def _runner(env, cam):
    from isaacgymloco_amd.learn import vision as V
    from isaacgymloco_amd.learn.bench_train import train_cfg_dict
    tc = train_cfg_dict("aliengo")
    tc["runner"]["num_steps_per_env"] = 4
    torch.manual_seed(7)
    return V.VisionOnPolicyRunner(env, tc, sensor=cam, encoder=DepthEncoder(12, 16, 2, **ENC), device="cpu")


def _evaluate(env, policy, steps=4, **kw):
    from isaacgymloco_amd.learn.evaluate import Evaluator, evaluate
    return evaluate(env, policy, steps, commands=(0.5, 0.0, 0.0), evaluator=Evaluator(env, api=CB.EmuApi()), **kw)


def test_a_vision_checkpoint_records_the_jitter_and_evaluate_honours_the_choice(tmp_path):
    api = MB.EmuApi()
    jit = sensors.MountJitter(**JITTER)
    env = _env()
    cam = env.add_sensor("depth", _camera(env, api, 16, 12, mount_jitter=jit))
    run = _runner(env, cam)
    path = str(tmp_path / "vision.pt")
    run.save(path)
    record = torch.load(path, weights_only=False)["vision"]["sensor"]
    assert record == cam.spec() and record["mount_jitter"] == jit.record()
    entry = {"pos": [0.01] * 3, "rot_deg": [1.0, 5.0, 1.0]}

    def fresh(**kw):
        e = _env()
        return e, e.add_sensor("depth", sensors.from_spec(e, record, api=api, **kw))

    # "trained", the default: the record's jitter -- kept on a camera that has it, put on one that does not
    env2, cam2 = fresh()
    assert cam2.mount_jitter == jit
    calls = api.calls["lsim_sensor_mount_jitter"]
    res = _evaluate(env2, path).result()
    assert res["conventions"]["camera_jitter"] == dict(entry, choice="trained") and cam2.mount_jitter == jit
    assert api.calls["lsim_sensor_mount_jitter"] == calls + 4 and not torch.equal(cam2.mount, cam2.mount_nominal)
    assert res["steps"] == 4 and res["total"]["columns"]["depth_influence"]["nonfinite"] == 0
    env3, cam3 = fresh(mount_jitter=None)
    res = _evaluate(env3, path, camera_jitter="trained").result()
    assert res["conventions"]["camera_jitter"] == dict(entry, choice="trained") and cam3.mount_jitter == jit
    assert (bits(cam3.mount) != bits(cam3.mount_nominal)).any(axis=1).all(), "every env's mount was drawn before the first step"
    # None: the nominal mount, and no jitter launch
    env4, cam4 = fresh()
    calls = api.calls["lsim_sensor_mount_jitter"]
    res = _evaluate(env4, path, camera_jitter=None).result()
    assert res["conventions"]["camera_jitter"] == {"choice": "off", "pos": None, "rot_deg": None}
    assert cam4.mount_jitter is None and cam4.mount is cam4.mount_nominal and api.calls["lsim_sensor_mount_jitter"] == calls
    # an override beyond the trained range
    env5, cam5 = fresh()
    wide = sensors.MountJitter(pos=0.03, rot_deg=10.0)
    res = _evaluate(env5, path, camera_jitter=wide).result()
    assert res["conventions"]["camera_jitter"] == {"choice": "override", "pos": [0.03] * 3, "rot_deg": [10.0] * 3} and cam5.mount_jitter == wide
    assert float((cam5.mount[:, :3] - cam5.mount_nominal[:, :3]).abs().max()) > 0.01
    # a runner brings no record: its camera stays as it is
    res = _evaluate(env, run, steps=2).result()
    assert res["conventions"]["camera_jitter"] == dict(entry, choice="trained") and cam.mount_jitter == jit
    for bad in ("off", 3):
        with pytest.raises((ValueError, TypeError)):
            _evaluate(env, run, steps=1, camera_jitter=bad)
    # a policy without a camera has no such entry
    from isaacgymloco_amd.learn.modules import HIMActorCritic
    torch.manual_seed(0)
    env6 = _env()
    assert "camera_jitter" not in _evaluate(env6, HIMActorCritic(270, 238, 45, 12), steps=1).result()["conventions"]


def test_the_command_line_reads_the_choice():
    from isaacgymloco_amd.learn.evaluate import parse_args, parse_camera_jitter
    base = ["--task", "aliengo", "--checkpoint", "x.pt", "--out", "y.json"]
    assert parse_args(base).camera_jitter == "trained" and parse_args(base + ["--camera-jitter", "off"]).camera_jitter is None
    assert parse_args(base + ["--camera-jitter", "pos=0.02,rot_deg=1/5/1"]).camera_jitter == sensors.MountJitter(pos=0.02, rot_deg=(1, 5, 1))
    assert parse_camera_jitter("rot_deg=3") == sensors.MountJitter(rot_deg=3.0)
    for bad in ("on", "pos=1/2", "pos=-1", "yaw=3", "pos=0.1,pos=0.2"):
        with pytest.raises(SystemExit):
            parse_args(base + ["--camera-jitter", bad])
