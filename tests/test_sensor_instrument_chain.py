"""CPU: the instrument error through the Python surface (envs/sensors.py InstrumentError, RaySensor(instrument=...), spec() / from_spec(), the
vision checkpoint's record and evaluate(camera_instrument=...)) on the emulated LeggedRobot, every launch through the CPU builds of the kernel
sources.  The two launches themselves are held to their reference in tests/test_sensor_instrument.py."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

import eval_columns_emu_binding as CB
import sensor_instrument_emu_binding as IB
import sensor_instrument_reference as IR
from helpers import C, abi
from isaacgymloco_amd.envs import sensors
from isaacgymloco_amd.learn.depth_encoder import DepthEncoder

FAR = 5.0
INSTRUMENT = dict(latency=(0, 2), noise_gain=(0.5, 2.0), depth_scale=0.02, depth_quad=0.005, fov=0.02)
JITTER = dict(pos=0.01, rot_deg=(1.0, 5.0, 1.0))
MODEL = dict(period=3, stagger=True, latency=2, frames=2, noise=(0.01, 0.002), dropout=0.02, normalise=True)
ENC = dict(c1=4, k1=3, s1=2, c2=8, k2=3, s2=1, latent_dim=10)
LAUNCHES = ("lsim_raycast", "lsim_raycast_bodies", "lsim_sensor_capture", "lsim_sensor_mount_jitter", "lsim_sensor_instrument", "lsim_sensor_capture_inst")
FILL_ALL = abi.DEFINES["LSIM_SENSOR_FILL_ALL"]


def bits(t):
    return np.ascontiguousarray(t.numpy() if isinstance(t, torch.Tensor) else t, np.float32).view(np.int32)


def _env(N=8, seed=3):
    from emu_env import EmuLeggedRobot
    from isaacgymloco_amd.learn.evaluate import play_cfg
    cfg = play_cfg(C.aliengo_cfg())
    cfg.env.num_envs = N
    cfg.terrain.num_rows, cfg.terrain.num_cols = 2, 2
    cfg.terrain.terrain_proportions = [0.0, 0.0, 0.0, 0.0, 0.5, 0.5]
    env = EmuLeggedRobot(cfg, seed=seed)
    env.reset()
    return env


def _camera(env, api, w=8, h=6, **kw):
    kw.setdefault("model", sensors.SensorModel(**MODEL))
    return sensors.depth_camera(env, w, h, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, near=0.05, far=FAR, api=api, **kw)


def test_instrument_error_values():
    i = sensors.InstrumentError(**INSTRUMENT)
    assert i.latency == (0, 2) and i.noise_gain == (0.5, 2.0) and (i.depth_scale, i.depth_quad, i.fov) == (0.02, 0.005, 0.02)
    assert i.record() == {"latency": [0, 2], "noise_gain": [0.5, 2.0], "depth_scale": 0.02, "depth_quad": 0.005, "fov": 0.02}
    assert sensors.InstrumentError(**i.record()) == i and sensors.InstrumentError() != i and json.loads(json.dumps(i.record())) == i.record()
    d = sensors.InstrumentError()
    assert d.latency is None and d.noise_gain == (1.0, 1.0) and (d.depth_scale, d.depth_quad, d.fov) == (0.0, 0.0, 0.0)
    assert "latency=(0, 2)" in repr(i) and eval("sensors." + repr(i)) == i
    for bad in (dict(latency=(2, 1)), dict(latency=(-1, 1)), dict(latency=(0, 8)), dict(latency=(0.5, 1)), dict(noise_gain=(2.0, 1.0)),
                dict(noise_gain=(-0.1, 1.0)), dict(depth_scale=-0.01), dict(depth_quad=math.nan), dict(fov=1.0), dict(fov=math.inf), dict(fov=-0.1)):
        with pytest.raises(ValueError):
            sensors.InstrumentError(**bad)


def test_without_an_instrument_nothing_is_launched_and_the_spec_is_the_one_of_before():
    env, api = _env(), IB.EmuApi()
    cam = env.add_sensor("depth", _camera(env, api))
    g = torch.Generator().manual_seed(0)
    for _ in range(3):
        env.step_device(torch.randn(8, 12, generator=g) * 0.3)
    env.reset_idx([1])
    assert api.calls == dict.fromkeys(LAUNCHES, 0) | {"lsim_sensor_capture": 5}
    assert cam.instrument is None and cam.stage("instrument") is None
    with pytest.raises(ValueError):
        cam.instrument_rows()
    assert list(cam.spec()) == ["kind", "width", "height", "dirs", "scale", "near", "far", "env_stride", "see_robot", "labels", "frame", "ignore_bodies",
                                "model", "mount"]


def test_an_instrument_needs_a_model_a_latency_the_history_holds_forward_rays_and_the_entry_points():
    env, api = _env(), IB.EmuApi()
    inst = sensors.InstrumentError(**INSTRUMENT)
    with pytest.raises(ValueError, match="model"):
        _camera(env, api, model=None, instrument=inst)
    with pytest.raises(ValueError, match="latency"):
        _camera(env, api, model=sensors.SensorModel(**dict(MODEL, latency=1)), instrument=inst)
    _camera(env, api, model=sensors.SensorModel(**dict(MODEL, latency=1)), instrument=sensors.InstrumentError(latency=(0, 1)))
    with pytest.raises(ValueError, match="fov"):
        sensors.lidar(env, 2, 20.0, 8, api=api, model=sensors.SensorModel(**MODEL), instrument=inst)
    lid = sensors.lidar(env, 2, 20.0, 8, api=api, model=sensors.SensorModel(**MODEL), instrument=sensors.InstrumentError(**dict(INSTRUMENT, fov=0.0)))
    assert lid.instrument_rows().shape == (8, 8)
    with pytest.raises(TypeError):
        _camera(env, api, instrument=INSTRUMENT)
    import sensor_mount_jitter_emu_binding as MB
    from isaacgymloco_amd import lib
    with pytest.raises(lib.LsimError, match="lsim_sensor_instrument"):
        _camera(env, MB.EmuApi(), instrument=inst)          # a library from before the entry points
    assert api.calls == dict.fromkeys(LAUNCHES, 0)


def _twin_history(cam, twin, api):
    """lsim_sensor_capture_inst, FILL_ALL, on the camera's present mounts and rows, tick and stream: what the whole history of a just-reset
    env must hold, bit for bit"""
    twin.mount.copy_(cam.mount)
    twin.stage("capture").struct.tick, twin.stage("capture").struct.flags, twin.stage("capture").struct.stream_id = cam.tick, FILL_ALL, cam.stream_id
    assert api.lsim_sensor_capture_inst(ctypes.byref(twin.stage("capture").struct), cam.instrument_rows().data_ptr(), None) == 0
    return twin.history().numpy().copy()


def test_reset_envs_draw_a_new_row_and_their_history_is_rendered_under_it():
    N = 8
    env, api = _env(N), IB.EmuApi()
    inst = sensors.InstrumentError(**INSTRUMENT)
    cam = _camera(env, api, see_robot=True, instrument=inst, mount_jitter=sensors.MountJitter(**JITTER))
    np.testing.assert_array_equal(cam.instrument_rows().numpy(), IB.neutral_rows(N, 2))
    assert api.calls == dict.fromkeys(LAUNCHES, 0)
    env.add_sensor("first", _camera(env, api, model=None))                  # so that the camera's stream_id is 1
    env.add_sensor("depth", cam)
    assert api.calls["lsim_sensor_instrument"] == api.calls["lsim_sensor_capture_inst"] == api.calls["lsim_sensor_mount_jitter"] == 1
    assert api.calls["lsim_sensor_capture"] == 0 and cam.stream_id == cam.stage("instrument").struct.stream_id == 1
    twin = _camera(env, api, see_robot=True)
    calls_twin = 0
    # add_sensor drew every env: the header's formulas on the camera's own seed, rank, stream and tick
    rows = cam.instrument_rows().numpy().copy()
    r = {k: getattr(cam.stage("instrument").struct, k) for k in IB.RANGES}
    assert (r["lat_lo"], r["lat_hi"]) == (0, 2) and r["gain_lo"] == 0.5 and r["fov_range"] == np.float32(0.02)
    want, tol = IR.expected(rows, np.ones(N, bool), env.lcfg.seed, env.lcfg.rank, env.common_step_counter, 1, r)
    assert (np.abs(rows - want) <= tol).all() and (rows[:, 1:5] != IB.neutral_rows(N, 2)[:, 1:5]).all()

    def fresh_equal_the_twin(envs, what):
        nonlocal calls_twin
        calls_twin += 1
        want = _twin_history(cam, twin, api)
        np.testing.assert_array_equal(bits(cam.history().numpy()[envs]), bits(want[envs]), err_msg=what)

    fresh_equal_the_twin(np.arange(N), "add_sensor")
    el = torch.full((N,), 5, dtype=env.episode_length_buf.dtype)
    for k in (1, 4, 6):
        el[k] = int(env.max_episode_length) - 1 - k // 2
    env.episode_length_buf = el
    g = torch.Generator().manual_seed(1)
    seen = set()
    for step in range(12):
        if step == 5:                           # a reset by hand between two steps: RESETS_ONLY, the tick of the step that follows
            before = cam.instrument_rows().clone()
            env.reset_idx([2, 5])
            fresh = env.episode_length_buf.numpy() == 0
            np.testing.assert_array_equal((bits(cam.instrument_rows()) != bits(before)).any(axis=1), fresh)
            fresh_equal_the_twin(np.nonzero(fresh)[0], "reset_idx by hand")
            by_hand = cam.instrument_rows().clone()
        before, hist_b, tick = cam.instrument_rows().clone(), cam.history().clone(), env.common_step_counter
        env.step_device(torch.randn(N, 12, generator=g) * 0.3)
        reset = env.reset_buf.numpy().astype(bool)
        np.testing.assert_array_equal(reset, env.episode_length_buf.numpy() == 0)
        changed = (bits(cam.instrument_rows()) != bits(before)).any(axis=1)
        np.testing.assert_array_equal(changed, reset, err_msg=f"step {step}")
        fresh_equal_the_twin(np.nonzero(reset)[0], f"step {step}")
        due = reset | ((tick + np.arange(N)) % 3 == 0)
        np.testing.assert_array_equal(bits(cam.history()[~torch.from_numpy(due)]), bits(hist_b[~torch.from_numpy(due)]))
        if step == 5:                           # the step that shares the by-hand reset's tick leaves those rows as they are
            np.testing.assert_array_equal(bits(cam.instrument_rows()[[2, 5]]), bits(by_hand[[2, 5]]))
        seen |= set(np.nonzero(reset)[0].tolist())
    assert {1, 4, 6} <= seen, "the time-outs happened"
    rows = cam.instrument_rows().numpy()
    assert set(np.unique(rows[:, 0])) <= {0.0, 1.0, 2.0} and (rows[:, 5:] == 0).all()
    assert int(cam.nonfinite_rays) == 0
    n = 1 + 12 + 1
    assert api.calls["lsim_sensor_instrument"] == api.calls["lsim_sensor_mount_jitter"] == n and api.calls["lsim_sensor_capture_inst"] == n + calls_twin
    assert api.calls["lsim_sensor_capture"] == 0
    # back to the shared constants, and on again
    cam.set_instrument(None)
    assert cam.instrument is None and cam.stage("instrument") is None and "instrument" not in cam.spec()
    env.step_device(torch.zeros(N, 12))
    assert api.calls["lsim_sensor_instrument"] == n and api.calls["lsim_sensor_capture"] == 1
    cam.set_instrument(inst)
    np.testing.assert_array_equal(cam.instrument_rows().numpy(), IB.neutral_rows(N, 2))
    cam.refresh()
    assert (cam.instrument_rows().numpy()[:, 1:5] != IB.neutral_rows(N, 2)[:, 1:5]).all() and cam.stream_id == cam.stage("instrument").struct.stream_id == 1


def test_the_draw_comes_before_the_capture():
    """with the two launches swapped a reset env's history is rendered under its previous row: the twin's check must tell"""
    N = 8
    env, api = _env(N), IB.EmuApi()
    cam = env.add_sensor("depth", _camera(env, api, instrument=sensors.InstrumentError(**INSTRUMENT)))
    twin = _camera(env, api)
    env.step_device(torch.zeros(N, 12))         # another tick than add_sensor's: other draws
    draw, capture = api.lsim_sensor_instrument, api.lsim_sensor_capture_inst
    held = []
    api.lsim_sensor_instrument = lambda *a: held.append(a) or 0
    api.lsim_sensor_capture_inst = lambda *a: (capture(*a), draw(*held.pop()))[0]
    before = cam.instrument_rows().clone()
    env.reset_idx(list(range(N)))               # everyone starts an episode
    assert (bits(cam.instrument_rows()) != bits(before)).any(axis=1).all() and not held
    api.lsim_sensor_instrument, api.lsim_sensor_capture_inst = draw, capture
    want = _twin_history(cam, twin, api)
    assert (bits(cam.history().numpy()) != bits(want)).any(axis=(1, 2)).all()


def test_spec_round_trips_the_instrument():
    api = IB.EmuApi()
    inst = sensors.InstrumentError(**INSTRUMENT)
    env = _env()
    cam = env.add_sensor("depth", _camera(env, api, instrument=inst, mount_jitter=sensors.MountJitter(**JITTER)))
    spec = cam.spec()
    assert json.loads(json.dumps(spec)) == spec and spec["instrument"] == inst.record() and list(spec)[-2:] == ["mount_jitter", "instrument"]
    back = sensors.from_spec(env, spec, api=api)
    assert back.instrument == inst and back.mount_jitter == cam.mount_jitter and back.spec() == spec
    assert all(getattr(back.stage("instrument").struct, k) == getattr(cam.stage("instrument").struct, k) for k in IB.RANGES)
    plain = sensors.from_spec(env, spec, api=api, instrument=None)
    assert plain.instrument is None and plain.stage("instrument") is None and plain.spec() == {k: v for k, v in spec.items() if k != "instrument"}
    other = sensors.from_spec(env, spec, api=api, instrument=sensors.InstrumentError(depth_scale=0.05))
    assert other.spec()["instrument"] == {"latency": None, "noise_gain": [1.0, 1.0], "depth_scale": 0.05, "depth_quad": 0.0, "fov": 0.0}
    assert (other.stage("instrument").struct.lat_lo, other.stage("instrument").struct.lat_hi) == (2, 2)                # None: the model's latency for every env
    assert sensors.from_spec(env, plain.spec(), api=api).instrument is None
    with pytest.raises(ValueError):
        sensors.from_spec(env, spec, api=api, instrument="trained")


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


def test_a_vision_checkpoint_records_the_instrument_and_evaluate_honours_the_choice(tmp_path):
    api = IB.EmuApi()
    inst = sensors.InstrumentError(**INSTRUMENT)
    env = _env()
    cam = env.add_sensor("depth", _camera(env, api, 16, 12, instrument=inst))
    run = _runner(env, cam)
    run.learn(1)
    assert api.calls["lsim_sensor_instrument"] == api.calls["lsim_sensor_capture_inst"] >= 1 + 4 and api.calls["lsim_sensor_capture"] == 0
    path = str(tmp_path / "vision.pt")
    run.save(path)
    record = torch.load(path, weights_only=False)["vision"]["sensor"]
    assert record == cam.spec() and record["instrument"] == inst.record()
    entry = inst.record()
    neutral = IB.neutral_rows(8, 2)

    def fresh(**kw):
        e = _env()
        return e, e.add_sensor("depth", sensors.from_spec(e, record, api=api, **kw))

    # "trained", the default: the record's instrument -- kept on a camera that has it, put on one that does not
    env2, cam2 = fresh()
    calls = api.calls["lsim_sensor_instrument"]
    res = _evaluate(env2, path, 20).result()
    assert res["conventions"]["camera_instrument"] == dict(entry, choice="trained") and cam2.instrument == inst
    assert res["conventions"]["camera_jitter"] == {"choice": "trained", "pos": None, "rot_deg": None}
    assert api.calls["lsim_sensor_instrument"] == calls + 20 and res["steps"] == 20
    assert res["total"]["columns"]["depth_influence"]["nonfinite"] == 0 and int(cam2.nonfinite_rays) == 0
    env3, cam3 = fresh(instrument=None)
    res = _evaluate(env3, path, camera_instrument="trained").result()
    assert res["conventions"]["camera_instrument"] == dict(entry, choice="trained") and cam3.instrument == inst
    assert (cam3.instrument_rows().numpy()[:, 1:5] != neutral[:, 1:5]).all(), "every env's row was drawn before the first step"
    # None: the model's constants, lsim_sensor_capture, and no draw
    env4, cam4 = fresh()
    calls = dict(api.calls)
    res = _evaluate(env4, path, camera_instrument=None).result()
    assert res["conventions"]["camera_instrument"] == {"choice": "off", "latency": None, "noise_gain": None, "depth_scale": None, "depth_quad": None, "fov": None}
    assert cam4.instrument is None and cam4.stage("instrument") is None
    assert api.calls["lsim_sensor_instrument"] == calls["lsim_sensor_instrument"] and api.calls["lsim_sensor_capture"] > calls["lsim_sensor_capture"]
    # an override beyond the trained range
    env5, cam5 = fresh()
    wide = sensors.InstrumentError(latency=(0, 2), noise_gain=(1.0, 4.0), depth_scale=0.05, fov=0.05)
    res = _evaluate(env5, path, camera_instrument=wide).result()
    assert res["conventions"]["camera_instrument"] == dict(wide.record(), choice="override") and cam5.instrument == wide
    assert float(np.abs(cam5.instrument_rows().numpy()[:, 2]).max()) > 0.02
    # a runner brings no record: its camera stays as it is
    res = _evaluate(env, run, steps=2).result()
    assert res["conventions"]["camera_instrument"] == dict(entry, choice="trained") and cam.instrument == inst
    for bad in ("off", 3):
        with pytest.raises((ValueError, TypeError)):
            _evaluate(env, run, steps=1, camera_instrument=bad)
    # a policy without a camera has no such entry
    from isaacgymloco_amd.learn.modules import HIMActorCritic
    torch.manual_seed(0)
    assert "camera_instrument" not in _evaluate(_env(), HIMActorCritic(270, 238, 45, 12), steps=1).result()["conventions"]


def test_the_command_line_reads_the_choice():
    from isaacgymloco_amd.learn.evaluate import parse_args, parse_camera_instrument
    base = ["--task", "aliengo", "--checkpoint", "x.pt", "--out", "y.json"]
    assert parse_args(base).camera_instrument == "trained" and parse_args(base + ["--camera-instrument", "off"]).camera_instrument is None
    text = "latency=0:2,noise_gain=0.5:2,depth_scale=0.02,depth_quad=0.005,fov=0.02"
    assert parse_args(base + ["--camera-instrument", text]).camera_instrument == sensors.InstrumentError(**INSTRUMENT)
    assert parse_camera_instrument("fov=0.03") == sensors.InstrumentError(fov=0.03)
    for bad in ("on", "latency=1", "latency=2:1", "fov=1", "gain=3", "fov=0.1,fov=0.2", "noise_gain=1"):
        with pytest.raises(SystemExit):
            parse_args(base + ["--camera-instrument", bad])
