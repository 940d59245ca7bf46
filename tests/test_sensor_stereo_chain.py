"""CPU: the stereo artefacts through the Python surface (envs/sensors.py StereoArtifacts, depth_camera(stereo=...), set_stereo(), spec() /
from_spec(), the vision checkpoint's record and evaluate(camera_stereo=...)) on the emulated LeggedRobot, every launch through the CPU
builds of the kernel sources.  The launch itself is held to its reference in tests/test_sensor_stereo.py."""
import gc
import json
import math
import weakref

import numpy as np
import pytest
import torch

import eval_columns_emu_binding as CB
import sensor_stereo_emu_binding as B
import sensor_stereo_reference as REF
from helpers import C, abi
from isaacgymloco_amd.envs import sensors
from isaacgymloco_amd.learn.depth_encoder import DepthEncoder

N, W, H, FAR = 8, 16, 12, 5.0
MODEL = dict(period=3, stagger=True, latency=1, frames=2, noise=(0.01, 0.002), dropout=0.0, normalise=True)
STEREO = dict(baseline=0.05, max_disparity=20.0, edge_radius=1, edge_rel=0.05, edge_hole=0.3, edge_fatten=0.3)
ENC = dict(c1=4, k1=3, s1=2, c2=8, k2=3, s2=1, latent_dim=10)
FILL_ALL, RESETS_ONLY = REF.FILL_ALL, REF.RESETS_ONLY


def bits(t):
    return np.ascontiguousarray(t.numpy() if isinstance(t, torch.Tensor) else t, np.float32).view(np.int32)


def _env(seed=3):
    from emu_env import EmuLeggedRobot
    from isaacgymloco_amd.learn.evaluate import play_cfg
    cfg = play_cfg(C.aliengo_cfg())
    cfg.env.num_envs = N
    cfg.terrain.num_rows, cfg.terrain.num_cols = 2, 2
    cfg.terrain.terrain_proportions = [0.0, 0.0, 0.0, 0.0, 0.5, 0.5]
    env = EmuLeggedRobot(cfg, seed=seed)
    env.reset()
    return env


def _camera(env, api, **kw):
    kw.setdefault("model", sensors.SensorModel(**MODEL))
    kw.setdefault("see_robot", True)
    kw.setdefault("labels", kw["see_robot"])
    return sensors.depth_camera(env, W, H, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, near=0.05, far=FAR, api=api, **kw)


def params_of(st):
    return {k: getattr(st, k) for k in B.SCALARS}


def expected(cam, pre_hist, tick, flags, state):
    """the reference on the sensor's own out and label rows and the history `pre_hist` the capture left"""
    st = cam.stage("stereo").struct
    inst = cam.instrument_rows().numpy() if cam.instrument is not None else None
    return REF.apply(pre_hist, state, cam.out.numpy(), cam.labels().numpy() if cam.label_rows is not None else None, (1.0 / cam.scale).numpy(),
                     cam.env.episode_length_buf.numpy(), inst, params_of(st), tick, flags)


def test_stereo_artifacts_values_and_text():
    s = sensors.StereoArtifacts(**STEREO)
    assert s.record() == {"baseline": 0.05, "max_disparity": 20.0, "window": None, "max_range": None, "edge_radius": 1, "edge_rel": 0.05, "edge_hole": 0.3,
                          "edge_fatten": 0.3}
    assert sensors.StereoArtifacts(**s.record()) == s and sensors.StereoArtifacts() != s and json.loads(json.dumps(s.record())) == s.record()
    d = sensors.StereoArtifacts()
    assert (d.baseline, d.max_disparity, d.window, d.max_range, d.edge_radius, d.edge_rel, d.edge_hole, d.edge_fatten) == (0.05, None, None, None, 1, 0.05, 0.25, 0.25)
    assert eval("sensors." + repr(s)) == s and sensors.StereoArtifacts.FIELDS == tuple(sensors.StereoArtifacts.TEXT)
    assert sensors.parse_stereo("default") == d and sensors.parse_stereo("") == d
    assert sensors.parse_stereo("baseline=0.05,max_disparity=20,edge_hole=0.3,edge_fatten=0.3") == s
    assert sensors.parse_stereo("window=12,max_range=3.5,edge_radius=3,max_disparity=none") == sensors.StereoArtifacts(window=12, max_range=3.5, edge_radius=3)
    for bad in (dict(baseline=-0.01), dict(baseline=math.nan), dict(max_disparity=0.0), dict(window=0), dict(window=129), dict(edge_radius=4), dict(edge_radius=-1),
                dict(edge_rel=1.0), dict(edge_rel=-0.1), dict(edge_hole=0.6, edge_fatten=0.6), dict(edge_hole=-0.1), dict(max_range=0.0), dict(max_range=math.inf)):
        with pytest.raises(ValueError):
            sensors.StereoArtifacts(**bad)
    for bad in ("baseline", "gain=3", "baseline=0.1,baseline=0.2", "window=1.5"):
        with pytest.raises(ValueError):
            sensors.parse_stereo(bad)


def test_without_the_option_nothing_is_launched_and_the_spec_is_the_one_of_before():
    env, api = _env(), B.EmuApi()
    cam = env.add_sensor("depth", _camera(env, api))
    for _ in range(3):
        env.step_device(torch.zeros(N, 12))
    assert api.calls["lsim_sensor_stereo"] == 0 and cam.stereo is None and cam.stage("stereo") is None and cam.chain() == ("lsim_sensor_capture",)
    with pytest.raises(ValueError):
        cam.stereo_counts()
    assert list(cam.spec()) == ["kind", "width", "height", "dirs", "scale", "near", "far", "env_stride", "see_robot", "labels", "frame", "ignore_bodies",
                                "model", "mount"]


def test_what_the_option_needs():
    env, api = _env(), B.EmuApi()
    s = sensors.StereoArtifacts(**STEREO)
    with pytest.raises(ValueError, match="model"):
        _camera(env, api, model=None, stereo=s)
    with pytest.raises(ValueError, match="camera"):
        sensors.lidar(env, 2, 20.0, 8, api=api, model=sensors.SensorModel(**MODEL), stereo=s)
    with pytest.raises(TypeError):
        _camera(env, api, stereo=STEREO)
    with pytest.raises(ValueError, match="LDS"):
        sensors.depth_camera(env, 128, 100, 87.0, api=api, model=sensors.SensorModel(**MODEL), stereo=s)
    import elevation_map_emu_binding as EB
    from isaacgymloco_amd import lib
    with pytest.raises(lib.LsimError, match="lsim_sensor_stereo"):
        _camera(env, EB.EmuApi(), stereo=s)             # a library from before the entry point
    yaw = _camera(env, api, frame="yaw", stereo=s)       # a gimballed camera is a stereo pair too
    assert yaw.stereo == s
    assert api.calls["lsim_sensor_stereo"] == 0


def test_derived_fields():
    env, api = _env(), B.EmuApi()
    cam = _camera(env, api, stereo=sensors.StereoArtifacts())
    st, sm = cam.stage("stereo").struct, cam.stage("capture").struct
    fb = (W / 2) / math.tan(math.radians(87.0) / 2) * 0.05
    scale = cam.scale.numpy().astype(np.float64)
    assert st.fb == np.float32(fb) and st.max_disparity == np.finfo(np.float32).max
    assert st.window == min(W - 1, 128, math.ceil(fb / (0.05 * scale.min())) + 1) == 14
    assert st.t_lo == np.float32(0.05 * (1 / cam.scale).max().item()) and st.t_hi == np.float32(0.98 * FAR * (1 / cam.scale).min().item())
    assert (st.edge_radius, st.edge_rel, st.p_edge_hole, st.p_edge_cum) == (1, np.float32(0.05), 0.25, 0.5)
    assert all(getattr(st, k) == getattr(sm, k) for k in ("hist", "hist_stride", "latency", "frames", "period", "stagger", "drop_value", "clip_lo", "clip_hi", "offset",
                                                          "gain", "episode_length", "seed", "rank", "stream_id"))
    assert (st.width, st.height, st.num_envs, st.env_stride, st.inst) == (W, H, N, 1, None)
    assert st.depth == cam.out_rows.data_ptr() and st.labels == cam.label_rows.data_ptr() and st.depth_stride == cam.out_rows.shape[1]
    wide = sensors.depth_camera(env, 64, 48, 87.0, near=0.3, far=FAR, api=api, model=sensors.SensorModel(**MODEL), stereo=sensors.StereoArtifacts(window=200 // 2))
    assert wide.stage("stereo").struct.window == 63
    back = sensors.from_spec(env, cam.spec(), api=api)          # a recorded camera has rays, no field of view: fb from the rays
    assert abs(back.stage("stereo").struct.fb - st.fb) <= 4 * np.spacing(np.float32(st.fb)) and back.stage("stereo").struct.window == st.window


@pytest.mark.parametrize("instrument", [False, True], ids=["model", "instrument"])
def test_frames_differ_from_a_twin_at_the_pixels_the_reference_flags(instrument):
    env, api = _env(), B.EmuApi()
    opts = dict(instrument=sensors.InstrumentError(latency=(0, 1), fov=0.02)) if instrument else {}
    cam = _camera(env, api, stereo=sensors.StereoArtifacts(**STEREO), **opts)
    twin = _camera(env, api, **opts)
    assert cam.chain()[-2:] == ("lsim_sensor_capture_inst" if instrument else "lsim_sensor_capture", "lsim_sensor_stereo")
    assert (cam.stage("stereo").struct.inst == cam.instrument_rows().data_ptr()) if instrument else cam.stage("stereo").struct.inst is None
    g = torch.Generator().manual_seed(0)
    seen = np.zeros(3, np.int64)
    state = np.zeros(2, np.int64)
    for step in range(7):
        if step == 0:
            tick, flags = 0, FILL_ALL
        elif step == 4:
            env.reset_idx([2, 5])
            tick, flags = int(env.common_step_counter), RESETS_ONLY
        else:
            env.step_device(torch.randn(N, 12, generator=g) * 0.3)
            tick, flags = int(env.common_step_counter), 0
        twin.history().copy_(cam.history())          # so that the twin's capture leaves what the camera's stage finds
        if instrument:
            twin.instrument_rows().copy_(cam.instrument_rows())
        before = cam.history().clone()
        cam.update(tick=tick, flags=flags)
        twin.update(tick=tick, flags=flags)
        assert np.array_equal(bits(cam.out), bits(twin.out)) and np.array_equal(cam.labels().numpy(), twin.labels().numpy())
        st = cam.stage("stereo").struct
        cap = cam.stage("capture").struct
        assert (st.tick, st.flags, st.seed, st.rank, st.stream_id) == (cap.tick, cap.flags, cap.seed, cap.rank, cap.stream_id) == (tick, flags, cap.seed, cap.rank, 0)
        hist, state, codes = expected(cam, twin.history().numpy()[:, :, :W * H], tick, flags, state)
        assert np.array_equal(bits(cam.history()[:, :, :W * H]), bits(hist)), f"step {step}"
        assert cam.stereo_counts().tolist() == state.tolist()
        differ = bits(cam.frames()) != bits(twin.frames())
        flagged = np.broadcast_to((codes != REF.KEEP)[:, None, :], differ.shape)
        assert not (differ & ~flagged).any(), "a pixel the reference keeps differs from the twin"
        due = (codes != REF.KEEP).any(axis=1)
        assert np.array_equal(bits(cam.history()[~torch.from_numpy(due)]), bits(twin.history()[~torch.from_numpy(due)]))
        seen += [(codes == REF.HOLE).sum(), (codes == REF.FATTEN).sum(), differ.sum()]
        assert cam.frame_images().shape == (N, 2, H, W) and np.array_equal(bits(cam.frame_images().reshape(N, 2, -1)), bits(hist[:, :2]))
        del before
    assert (seen > 0).all(), seen
    assert api.calls["lsim_sensor_stereo"] == 7 and int(cam.nonfinite_rays) == 0


def test_the_chain_order_and_every_consumer_reads_the_artefacts():
    import frames_log_emu_binding  # noqa: F401  (the shim is part of B.EmuApi)
    env, api = _env(), B.EmuApi()
    # every valid pixel is too near: the whole image a hole, so whoever reads a range reads the capture, not the stage
    blank = sensors.StereoArtifacts(max_disparity=1e-6, edge_hole=0.0, edge_fatten=0.0)
    cam = env.add_sensor("depth", _camera(env, api, stereo=blank))
    twin = _camera(env, api)
    twin.refresh(tick=cam.tick)
    enc = DepthEncoder(H, W, 2, **ENC)
    cam.attach_encoder(enc)
    cam.attach_map(sensors.ElevationMap(size=16, source="noisy"))
    twin.attach_map(sensors.ElevationMap(size=16, source="noisy"))
    cam.attach_frames_log(3)
    assert cam.chain() == ("lsim_sensor_capture", "lsim_sensor_stereo", "lsim_sensor_frames_log", "lsim_elevation_map", "lsim_depth_encode")
    cam.refresh()
    cam.begin_rollout()
    for _ in range(3):
        env.step_device(torch.zeros(N, 12))
        twin.update(tick=cam.tick)
    y_hole = REF.y_hole(params_of(cam.stage("stereo").struct))
    st = cam.stage("stereo").struct
    t = cam.out.numpy() / cam.scale.numpy()[None, :]
    valid = (t > st.t_lo * 1.001) & (t < st.t_hi * 0.999) & (cam.labels().numpy() != 0)      # clear of the two limits' rounding
    newest = cam.history().numpy()[:, -1, :W * H]          # the capture `out` belongs to
    assert valid.any() and (newest[valid] == y_hole).all() and int(cam.stereo_counts()[0]) > 0 and int(cam.stereo_counts()[1]) == 0
    # a noisy-source map inserts no hole: the hole value sits at a clip limit.  The twin's map, fed the same captures, knows cells
    assert int((twin.map_state()[1] >= 0).sum()) > 0 and int((cam.map_state()[1] >= 0).sum()) == 0 and int(cam.map_known().sum()) == 0
    # the encoder and the frame log read the rewritten frames
    with torch.no_grad():
        want = enc(cam.frame_images())
    assert torch.allclose(cam.latent(), want, atol=1e-5)
    rows = int(cam.frames_log_state()[0])
    src = cam.frames_log_sources().numpy()[:rows]
    log = cam.frames_log().numpy()[:rows, :, :W * H]
    last = {int(s % N): i for i, s in enumerate(src)}           # the newest logged image of every env
    assert len(last) == N and all(np.array_equal(bits(log[i]), bits(cam.frames().numpy()[e])) for e, i in last.items())
    assert all((log[i] == y_hole).any() for i in last.values())


def test_a_noisy_map_and_the_option_need_a_hole_value_at_a_clip_limit_in_both_orders():
    env, api = _env(), B.EmuApi()
    inside = sensors.SensorModel(**dict(MODEL, drop_value=1.0))             # no dropout: the plain rule lets it pass
    s = sensors.StereoArtifacts(**STEREO)
    cam = _camera(env, api, model=inside)
    cam.attach_map(sensors.ElevationMap(size=16, source="noisy"))
    with pytest.raises(ValueError, match="drop_value"):
        cam.set_stereo(s)
    assert cam.stereo is None and cam.chain() == ("lsim_sensor_capture", "lsim_elevation_map")
    cam2 = _camera(env, api, model=inside, stereo=s)
    with pytest.raises(ValueError, match="drop_value"):
        cam2.attach_map(sensors.ElevationMap(size=16, source="noisy"))
    cam2.attach_map(sensors.ElevationMap(size=16, source="clean"))         # the clean rows hold no hole
    cam3 = _camera(env, api, stereo=s)                                       # drop_value 0 clamps to clip_lo
    cam3.attach_map(sensors.ElevationMap(size=16, source="noisy"))
    assert cam3.chain() == ("lsim_sensor_capture", "lsim_sensor_stereo", "lsim_elevation_map")


def test_setting_it_launches_nothing_and_dropping_it_frees_the_buffers():
    env, api = _env(), B.EmuApi()
    cam = env.add_sensor("depth", _camera(env, api))
    env.step_device(torch.zeros(N, 12))
    before, calls = cam.history().clone(), dict(api.calls)
    cam.set_stereo(sensors.StereoArtifacts(**STEREO))
    assert api.calls == calls and np.array_equal(bits(cam.history()), bits(before)) and cam.stereo_counts().tolist() == [0, 0]
    cam.set_instrument(sensors.InstrumentError(latency=(0, 1)))
    assert cam.stage("stereo").struct.inst == cam.instrument_rows().data_ptr()
    cam.set_instrument(None)
    assert cam.stage("stereo").struct.inst is None
    env.step_device(torch.zeros(N, 12))
    assert api.calls["lsim_sensor_stereo"] == 1
    refs = [weakref.ref(t) for t in cam.stage("stereo").buffers.values()]
    assert len(refs) == 2
    cam.set_stereo(None)
    gc.collect()
    assert all(r() is None for r in refs) and cam.stereo is None and "stereo" not in cam.spec() and cam.chain() == ("lsim_sensor_capture",)
    env.step_device(torch.zeros(N, 12))
    assert api.calls["lsim_sensor_stereo"] == 1


def test_spec_round_trips_the_option():
    env, api = _env(), B.EmuApi()
    s = sensors.StereoArtifacts(**STEREO)
    cam = env.add_sensor("depth", _camera(env, api, stereo=s, instrument=sensors.InstrumentError(fov=0.02)))
    spec = cam.spec()
    assert json.loads(json.dumps(spec)) == spec and spec["stereo"] == s.record() and list(spec)[-1] == "stereo"
    back = sensors.from_spec(env, spec, api=api)
    assert back.stereo == s and back.spec() == spec and back.chain() == cam.chain()
    plain = sensors.from_spec(env, spec, api=api, stereo=None)
    assert plain.stereo is None and plain.spec() == {k: v for k, v in spec.items() if k != "stereo"}
    other = sensors.from_spec(env, plain.spec(), api=api, stereo=sensors.StereoArtifacts(baseline=0.1))
    assert other.spec()["stereo"]["baseline"] == 0.1 and sensors.from_spec(env, plain.spec(), api=api).stereo is None
    with pytest.raises(ValueError):
        sensors.from_spec(env, spec, api=api, stereo="trained")


def _runner(env, cam):
    from isaacgymloco_amd.learn import vision as V
    from isaacgymloco_amd.learn.bench_train import train_cfg_dict
    tc = train_cfg_dict("aliengo")
    tc["runner"]["num_steps_per_env"] = 4
    torch.manual_seed(7)
    return V.VisionOnPolicyRunner(env, tc, sensor=cam, encoder=DepthEncoder(H, W, 2, **ENC), device="cpu")


def _evaluate(env, policy, steps=4, **kw):
    from isaacgymloco_amd.learn.evaluate import Evaluator, evaluate
    return evaluate(env, policy, steps, commands=(0.5, 0.0, 0.0), evaluator=Evaluator(env, api=CB.EmuApi()), **kw)


def test_a_vision_checkpoint_records_the_option_and_evaluate_honours_the_choice(tmp_path):
    api = B.EmuApi()
    s = sensors.StereoArtifacts(**STEREO)
    env = _env()
    cam = env.add_sensor("depth", _camera(env, api, stereo=s))
    run = _runner(env, cam)
    run.learn(1)
    assert api.calls["lsim_sensor_stereo"] == api.calls["lsim_sensor_capture"] >= 1 + 4
    path = str(tmp_path / "vision.pt")
    run.save(path)
    record = torch.load(path, weights_only=False)["vision"]["sensor"]
    assert record == cam.spec() and record["stereo"] == s.record()

    def fresh(**kw):
        e = _env()
        return e, e.add_sensor("depth", sensors.from_spec(e, record, api=api, **kw))

    env2, cam2 = fresh()
    calls = api.calls["lsim_sensor_stereo"]
    res = _evaluate(env2, path, 6).result()
    assert res["conventions"]["camera_stereo"] == dict(s.record(), choice="trained") and cam2.stereo == s
    assert api.calls["lsim_sensor_stereo"] == calls + 6 and res["total"]["columns"]["depth_influence"]["nonfinite"] == 0
    env3, cam3 = fresh(stereo=None)                     # "trained" puts the record's option on a camera that lacks it
    res = _evaluate(env3, path, camera_stereo="trained").result()
    assert res["conventions"]["camera_stereo"] == dict(s.record(), choice="trained") and cam3.stereo == s and int(cam3.stereo_counts()[0]) > 0
    env4, cam4 = fresh()
    calls = api.calls["lsim_sensor_stereo"]
    res = _evaluate(env4, path, camera_stereo=None).result()
    assert res["conventions"]["camera_stereo"] == dict(dict.fromkeys(sensors.StereoArtifacts.FIELDS), choice="off")
    assert cam4.stereo is None and api.calls["lsim_sensor_stereo"] == calls
    env5, cam5 = fresh()
    wide = sensors.StereoArtifacts(baseline=0.1, edge_hole=0.5, edge_fatten=0.5)
    res = _evaluate(env5, path, camera_stereo=wide).result()
    assert res["conventions"]["camera_stereo"] == dict(wide.record(), choice="override") and cam5.stereo == wide
    res = _evaluate(env, run, steps=2).result()         # a runner brings no record: its camera stays as it is
    assert res["conventions"]["camera_stereo"] == dict(s.record(), choice="trained") and cam.stereo == s
    for bad in ("off", 3):
        with pytest.raises((ValueError, TypeError)):
            _evaluate(env, run, steps=1, camera_stereo=bad)
    from isaacgymloco_amd.learn.modules import HIMActorCritic
    torch.manual_seed(0)
    assert "camera_stereo" not in _evaluate(_env(), HIMActorCritic(270, 238, 45, 12), steps=1).result()["conventions"]


def test_the_command_line_reads_the_choice():
    from isaacgymloco_amd.learn.evaluate import parse_args, parse_camera_stereo
    base = ["--task", "aliengo", "--checkpoint", "x.pt", "--out", "y.json"]
    assert parse_args(base).camera_stereo == "trained" and parse_args(base + ["--camera-stereo", "off"]).camera_stereo is None
    text = "baseline=0.05,max_disparity=20,edge_radius=1,edge_rel=0.05,edge_hole=0.3,edge_fatten=0.3"
    assert parse_args(base + ["--camera-stereo", text]).camera_stereo == sensors.StereoArtifacts(**STEREO)
    assert parse_camera_stereo("baseline=0.03") == sensors.StereoArtifacts(baseline=0.03)
    for bad in ("on", "default", "baseline=-1", "edge_radius=7", "gain=3", "baseline=0.1,baseline=0.2", "edge_hole=0.7,edge_fatten=0.7"):
        with pytest.raises(SystemExit):
            parse_args(base + ["--camera-stereo", bad])
