"""CPU: the map policy through the Python surface -- envs/sensors.py OdometryError, RaySensor.attach_map(m, odometry=...), attach_map_rows,
odometry_pose / odometry_state / map_rows, spec() / from_spec(); learn/map_policy.py MapOnPolicyRunner; learn/evaluate.py on a map policy --
on the emulated LeggedRobot, every launch through the CPU builds of the kernel sources.  The two launches themselves are held to their
references in tests/test_odometry.py and tests/test_map_rows.py."""
import json

import numpy as np
import pytest
import torch

import eval_columns_emu_binding as CB
import odometry_emu_binding as OB
from isaacgymloco_amd.envs import sensors
from test_elevation_map_chain import FAR, SPEC_KEYS, _camera, _env, _logged, _truth, bits

ODO = sensors.OdometryError(scale=0.02, yaw_per_m=0.05, z_per_m=0.02, noise=(0.005, 0.002, 0.002))
CHAIN = ["lsim_odometry_step", "lsim_sensor_capture", "lsim_elevation_map", "lsim_map_rows"]
GRID = [[x, y] for x in np.linspace(-0.5, 0.5, 11) for y in np.linspace(-0.4, 0.4, 9)]          # 99 points: two channels fit the fused launch


def test_values_records_and_refusals_of_an_odometry_error():
    o = sensors.OdometryError()
    assert (o.scale, o.yaw_per_m, o.z_per_m, o.noise) == (0.0, 0.0, 0.0, (0.0, 0.0, 0.0)) and o.ranges() == (0.0,) * 6
    assert sensors.OdometryError(**ODO.record()) == ODO and ODO != o and json.loads(json.dumps(ODO.record())) == ODO.record()
    assert "yaw_per_m=0.05" in repr(ODO)
    for bad in (dict(scale=-0.1), dict(yaw_per_m=float("nan")), dict(z_per_m=float("inf")), dict(noise=(0.0, 0.0)), dict(noise=(0.0, -1.0, 0.0))):
        with pytest.raises(ValueError):
            sensors.OdometryError(**bad)
    assert sensors.parse_odometry("scale=0.02,yaw_per_m=0.05,z_per_m=0.02,noise=0.005:0.002:0.002") == ODO and sensors.parse_odometry("") == o


def test_launch_order_is_odometry_capture_map_rows_with_the_captures_tick_and_flags():
    N = 8
    env, api = _env(N), OB.EmuApi()
    log = _logged(api, CHAIN)
    cam = _camera(env, api, 16, 12)
    cam.attach_map(sensors.ElevationMap(size=32, source="clean"), odometry=ODO)
    assert cam.attach_map_rows(("height", "known")) is cam.map_rows() and log == [], "never captured: nothing to integrate, insert or build yet"
    env.add_sensor("depth", cam)
    assert log == CHAIN
    assert cam.stage("odometry").struct.stream_id == cam.stage("capture").struct.stream_id == cam.stream_id and (cam.stage("odometry").struct.seed, cam.stage("odometry").struct.rank) == (cam.stage("capture").struct.seed, cam.stage("capture").struct.rank)
    assert bool((cam.odometry_state()[:, 0:4] == 0).all()) and bool((cam.odometry_state()[:, 4:7] != 0).all()), "add_sensor's refresh made every env fresh"
    g = torch.Generator().manual_seed(0)
    for step in range(4):
        tick = env.common_step_counter
        env.step_device(torch.randn(N, 12, generator=g) * 0.3)
        assert cam.stage("odometry").struct.tick == cam.stage("capture").struct.tick == cam.stage("map").struct.tick == tick and cam.stage("odometry").struct.flags == cam.stage("capture").struct.flags == cam.stage("map").struct.flags
    assert log == CHAIN * 5 and api.calls["lsim_odometry_step"] == 5 and api.calls["lsim_map_rows"] == 5
    odo, est = cam.odometry_state(), cam.odometry_pose()
    moved = env.episode_length_buf > 1
    assert bool(moved.any()) and bool((odo[moved][:, 0:3] != 0).all()), "every env that walked has drifted"
    assert torch.equal(odo[:, 8:10], env.root_states[:, 0:2]) and torch.equal(est[:, 7:13], env.root_states[:, 7:13])
    assert torch.equal(est[:, 0:3], env.root_states[:, 0:3] + odo[:, 0:3])
    assert cam.stage("map").struct.root_states == est.data_ptr() != env.root_states.data_ptr() and cam.stage("capture").struct.rb.rc.root_states == env.root_states.data_ptr()
    assert cam.stage("map_rows").struct.pose == est.data_ptr() and cam.map_pose() is est
    env.reset_idx([1])
    assert log[-4:] == CHAIN and len(log) == 24
    assert bool((cam.odometry_state()[1, 0:4] == 0).all()) and bool((cam.odometry_state()[0, 0:3] != 0).all())
    rows, P = cam.map_rows(), 187
    assert rows.shape == (N, 2 * P) and torch.equal(rows[:, P:], cam.map_known().to(torch.float32)) and bool(torch.isfinite(rows).all())
    scale = float(env.lcfg.obs_scale_height)
    want = (est[:, 2:3] - 0.5 - cam.map_scan()).clamp(-1.0, 1.0) * scale
    np.testing.assert_array_equal(bits(rows[:, :P]), bits(want))
    cam.attach_map_rows(None)
    env.step_device(torch.zeros(N, 12))
    assert log[-3:] == CHAIN[:3] and cam.stage("map_rows") is None
    with pytest.raises(ValueError, match="attach_map_rows"):
        cam.map_rows()


def test_without_odometry_and_rows_nothing_is_allocated_or_launched_and_the_maps_struct_is_the_one_of_before():
    env, api = _env(), OB.EmuApi()
    cam = env.add_sensor("depth", _camera(env, api))
    m = sensors.ElevationMap(size=16)
    cam.attach_map(m)
    plain = bytes(cam.stage("map").struct)
    for _ in range(2):
        env.step_device(torch.zeros(8, 12))
    assert api.calls["lsim_odometry_step"] == 0 and api.calls["lsim_map_rows"] == 0 and api.calls["lsim_elevation_map"] == 3
    assert cam.odometry is None and cam.stage("odometry") is None and cam.stage("map_rows") is None and cam.map_channels is None
    assert cam.stage("map").struct.root_states == env.root_states.data_ptr() and cam.map_pose() is env.root_states
    assert list(cam.spec()) == SPEC_KEYS + ["map"]
    for getter in (cam.odometry_pose, cam.odometry_state):
        with pytest.raises(ValueError, match="odometry"):
            getter()
    with pytest.raises(ValueError, match="attach_map_rows"):
        cam.map_rows()
    # the struct attach_map fills: field for field the one without the parameter, but for the arrays it allocated anew and the tick it ran on
    def fields(em, skip=("pts", "height", "stamp", "cell", "scan", "known", "state", "inv_scale", "tick", "flags")):
        return {f: getattr(em, f) for f, _ in em._fields_ if f not in skip}
    before = fields(cam.stage("map").struct)
    cam.attach_map(m, odometry=None)
    assert fields(cam.stage("map").struct) == before and len(bytes(cam.stage("map").struct)) == len(plain)
    cam.attach_map(m, odometry=ODO)
    with_odo = fields(cam.stage("map").struct)
    assert {k for k in before if before[k] != with_odo[k]} == {"root_states"} and api.calls["lsim_odometry_step"] == 1
    cam.attach_map_rows(("height",))
    assert cam.attach_map(None) is None and cam.stage("odometry") is None and cam.stage("map_rows") is None and cam.odometry is None
    assert list(cam.spec()) == SPEC_KEYS
    with pytest.raises(TypeError):
        cam.attach_map(m, odometry={"scale": 0.1})
    with pytest.raises(ValueError, match="channels"):
        cam.attach_map_rows(("known",))
    with pytest.raises(ValueError, match="attach_map"):
        cam.attach_map_rows(("height",))
    import elevation_map_emu_binding as EB
    from isaacgymloco_amd import lib
    with pytest.raises(lib.LsimError, match="lsim_odometry_step"):
        _camera(env, EB.EmuApi()).attach_map(m, odometry=ODO)           # a library from before the entry points
    old = _camera(env, EB.EmuApi())
    old.attach_map(m)
    with pytest.raises(lib.LsimError, match="lsim_map_rows"):
        old.attach_map_rows(("height",))


def test_all_zero_odometry_builds_the_map_of_no_odometry_bit_for_bit():
    N = 8
    env, api = _env(N), OB.EmuApi()
    a, b = _camera(env, api, 16, 12), _camera(env, api, 16, 12)
    a.attach_map(sensors.ElevationMap(size=32, source="clean"), odometry=sensors.OdometryError())
    b.attach_map(sensors.ElevationMap(size=32, source="clean"))
    env.add_sensor("a", a)
    env.add_sensor("b", b)
    a.attach_map_rows(("height", "known"))
    b.attach_map_rows(("height", "known"))
    g = torch.Generator().manual_seed(2)
    for _ in range(5):
        env.step_device(torch.randn(N, 12, generator=g) * 0.3)
    np.testing.assert_array_equal(bits(a.odometry_pose()[:, 0:7]), bits(env.root_states[:, 0:7] + 0.0))
    for x, y in zip(a.map_state() + (a.map_scan(), a.map_known(), a.map_rows(), a.map_heights()), b.map_state() + (b.map_scan(), b.map_known(), b.map_rows(), b.map_heights())):
        np.testing.assert_array_equal(bits(x), bits(y))
    assert bool((a.map_state()[1] >= 0).any()) and api.calls["lsim_odometry_step"] == 6


def test_a_yaw_drift_bends_the_map_on_a_slope():
    """poses by hand: a walk of 1.5 m across a slope; the map placed with a pose whose heading drifts (up to 0.4 rad per metre) is farther
    from the terrain under the robot's TRUE scan points than the map placed with the true pose.  Only the ordering is asserted."""
    N = 8
    env, api = _env(N, terrain="slope"), OB.EmuApi()
    model = sensors.SensorModel(clip=(0.0, FAR))
    errs = {}
    origins = env.env_origins.numpy()
    poses = np.zeros((N, 7), np.float32)
    poses[:, 6] = 1.0
    poses[:, 0], poses[:, 1] = origins[:, 0] + 1.6, origins[:, 1] - 0.6 + 0.3 * np.arange(N) / N
    for name, odo in (("true", None), ("drift", sensors.OdometryError(yaw_per_m=0.4))):
        cam = _camera(env, api, 32, 24, model=model)
        cam.attach_map(sensors.ElevationMap(size=32, source="clean"), odometry=odo)
        p = poses.copy()
        for k in range(25):
            p[:, 2] = _truth(env, p[:, :2]) + 0.45
            env.root_states[:, :7] = torch.as_tensor(p)
            env.episode_length_buf[:] = 0 if k == 0 else 1
            cam.update(tick=k)
            p[:, 0] += np.float32(0.0442)
            p[:, 1] += np.float32(0.0442)
        p[:, 0] -= np.float32(0.0442)
        p[:, 1] -= np.float32(0.0442)
        known = cam.map_known().numpy().astype(bool)
        world = p[:, None, :2] + cam.stage("map").buffers["pts"].numpy()[None]       # identity orientation: the base-yaw frame is the world's
        err = np.abs(cam.map_scan().numpy() - _truth(env, world))
        assert known.sum() > N * 40
        errs[name] = float(err[known].mean())
        if odo is not None:
            d = cam.odometry_state().numpy()
            assert (np.abs(d[:, 3]) > 1e-3).all() and (np.hypot(d[:, 0], d[:, 1]) > 1e-3).all() and (d[:, 2] == 0).all() and (d[:, 4] == 0).all()
    print(f"mean |map - terrain| at the known scan points after 1.5 m across a slope: true pose {errs['true']:.4f} m, yaw drift up to 0.4 rad/m {errs['drift']:.4f} m")
    assert errs["drift"] > errs["true"]


def test_spec_and_from_spec_carry_the_odometrys_record():
    env, api = _env(), OB.EmuApi()
    m = sensors.ElevationMap(size=16, source="clean", points=GRID)
    cam = env.add_sensor("depth", _camera(env, api))
    cam.attach_map(m, odometry=ODO)
    spec = cam.spec()
    assert list(spec) == SPEC_KEYS + ["map", "odometry"] and spec["odometry"] == ODO.record() and json.loads(json.dumps(spec)) == spec
    back = sensors.from_spec(env, spec, api=api)
    assert back.odometry == ODO and back.map == m and back.spec() == spec and back.stage("map").struct.root_states == back.odometry_pose().data_ptr()
    assert [getattr(back.stage("odometry").struct, n) for n in ("scale_range", "yaw_range", "z_range", "pos_noise", "yaw_noise", "z_noise")] == [np.float32(v) for v in ODO.ranges()]
    assert sensors.from_spec(env, spec, api=api, odometry=None).odometry is None
    other = sensors.OdometryError(scale=0.1)
    assert sensors.from_spec(env, spec, api=api, odometry=other).odometry == other
    with pytest.raises(ValueError, match="odometry"):
        sensors.from_spec(env, spec, api=api, odometry="yes")
    assert sensors.from_spec(env, spec, api=api, elevation_map=None).odometry is None, "without a map the odometry has nothing to act on"


def _runner(env, cam, channels=("height", "known"), T=4):
    from isaacgymloco_amd.learn.bench_train import train_cfg_dict
    from isaacgymloco_amd.learn.map_policy import MapOnPolicyRunner
    tc = train_cfg_dict("aliengo")
    tc["runner"]["num_steps_per_env"] = T
    torch.manual_seed(7)
    return MapOnPolicyRunner(env, tc, sensor=cam, channels=channels, device="cpu")


def _map_env(N=8, terrain="stairs", points=GRID, odometry=ODO):
    env, api = _env(N, terrain=terrain), OB.EmuApi()
    cam = env.add_sensor("depth", _camera(env, api, 16, 12))
    cam.attach_map(sensors.ElevationMap(size=32, source="clean", points=points), odometry=odometry)
    return env, api, cam


def test_the_runner_stores_the_rows_the_actor_read_warm_starts_and_refuses_a_row_too_wide(tmp_path):
    from isaacgymloco_amd.learn.map_policy import MapOnPolicyRunner, MapPPO
    from isaacgymloco_amd.learn.modules import HIMActorCritic
    from isaacgymloco_amd.learn.vision import VisionActorCritic
    T = 4
    env, api, cam = _map_env()
    run = _runner(env, cam, T=T)
    ac, alg = run.alg.actor_critic, run.alg
    assert isinstance(alg, MapPPO) and isinstance(ac, VisionActorCritic) and ac.depth_latent_dim == 198 and ac.actor[0].in_features == 45 + 3 + 16 + 198
    assert (ac.actor[0].in_features + 15) // 16 * 16 == 272 and cam.map_channels == ("height", "known") and alg.latent_source == cam.map_rows and alg.encoder is None
    assert alg.storage.depth_latent.shape == (T, 8, 198) and alg.snapshot_steps() == []
    obs, priv = env.get_observations().clone(), env.get_privileged_observations().clone()
    seen = []
    with torch.inference_mode():
        for t in range(T):
            seen.append(cam.map_rows().clone())
            obs, priv = run._rollout_step(obs, priv)[:2]
    for t in range(T):
        np.testing.assert_array_equal(bits(alg.storage.depth_latent[t]), bits(seen[t]), err_msg=f"step {t}")
    assert len({s.numpy().tobytes() for s in seen}) == T, "the rows moved during the rollout"
    with torch.inference_mode():
        alg.compute_returns(priv)
    out = alg.update()
    assert len(out) == 4 and all(np.isfinite(float(v)) for v in out) and all(bool(torch.isfinite(v).all()) for v in ac.state_dict().values())
    # a HIM policy warm-starts it: with zero map columns it is that policy, bit for bit, whatever the rows hold
    torch.manual_seed(3)
    him = HIMActorCritic(env.num_obs, env.num_privileged_obs, env.num_one_step_obs, env.num_actions).eval()
    ac.load_him_state_dict(him.state_dict())
    ac.eval()
    # (64 rows: torch's CPU GEMM chooses its kernel by shape, and below some 30 rows the 262-column layer goes through one that sums the
    # first 64 columns in another order than the 64-column layer's -- the zero columns add exact zeros either way.  The device launch has
    # one order for every width: tests/test_gpu_map_policy.py holds it to this at the env's own batch)
    o = torch.randn(64, env.num_obs)
    with torch.no_grad():
        for rows in (torch.randn(64, 198), 1e4 * torch.randn(64, 198), cam.map_rows().repeat(8, 1)):
            np.testing.assert_array_equal(bits(ac.act_inference(o, depth_latent=rows)), bits(him.act_inference(o)))
    # the checkpoint's record, and its round trip
    path = str(tmp_path / "map.pt")
    run.save(path)
    d = torch.load(path, weights_only=False)
    assert d["map_policy"] == {"sensor": cam.spec(), "channels": ["height", "known"], "dim": 198} and "vision" not in d and "depth_encoder_state_dict" not in d
    assert d["map_policy"]["sensor"]["odometry"] == ODO.record()
    env2, api2, cam2 = _map_env()
    run2 = _runner(env2, cam2, T=T)
    run2.load(path)
    sa, sb = ac.state_dict(), run2.alg.actor_critic.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    # the width: 187 points take one channel (251 columns), not two (438)
    env3, api3, cam3 = _map_env(points=None)
    with pytest.raises(ValueError, match="at most 272"):
        _runner(env3, cam3, channels=("height", "known"))
    one = _runner(env3, cam3, channels=("height",))
    assert one.alg.actor_critic.actor[0].in_features == 251 and cam3.map_rows().shape == (8, 187)
    with pytest.raises(ValueError, match="elevation map"):
        MapOnPolicyRunner(env3, {}, sensor=_camera(env3, api3))
    with pytest.raises(ValueError, match="channels"):
        _runner(env3, cam3, channels=("known",))


def _evaluate(env, policy, steps=3, **kw):
    from isaacgymloco_amd.learn.evaluate import Evaluator, evaluate
    return evaluate(env, policy, steps, commands=(0.5, 0.0, 0.0), evaluator=Evaluator(env, api=CB.EmuApi()), **kw)


def test_evaluate_on_a_map_policy_blind_the_three_odometry_forms_and_the_scan_error_identity(tmp_path):
    from isaacgymloco_amd.learn.evaluate import parse_args
    from isaacgymloco_amd.learn.vision import height_scan_block
    named = ("depth_influence", "scan_error", "map_scan_error", "map_coverage")
    env, api, cam = _map_env(points=None)
    run = _runner(env, cam, channels=("height",))
    path = str(tmp_path / "map.pt")
    run.save(path)
    res = _evaluate(env, run, vision_metrics=named).result()
    cols = res["total"]["columns"]
    assert list(cols) == ["depth_influence", "map_scan_error", "map_coverage"], "the encoder's metric is dropped, not zero"
    assert cols["depth_influence"]["mean"] > 0.0 and 0.0 < cols["map_coverage"]["mean"] < 1.0 and all(c["nonfinite"] == 0 for c in cols.values())
    assert res["conventions"]["odometry"] == dict(ODO.record(), choice="trained") and cam.odometry == ODO
    # the identity: with odometry the error is the rows' own height block against the privileged one
    off, P = height_scan_block(env.cfg)
    priv = env.get_privileged_observations()
    scale = float(env.lcfg.obs_scale_height)
    block = (cam.odometry_pose()[:, 2:3] - 0.5 - cam.map_scan()).clamp(-1.0, 1.0) * scale
    np.testing.assert_array_equal(bits(cam.map_rows()[:, :P]), bits(block))
    want = float((cam.map_rows()[:, :P] - priv[:, off:off + P]).square().mean(dim=1).to(torch.float64).mean())
    one = _evaluate(env, run, steps=1, vision_metrics=("map_scan_error",)).result()["total"]
    assert list(one["columns"]) == ["map_scan_error"] and one["samples"] == env.num_envs, "nobody fell in that one step"
    assert want > 0.0 and abs(one["columns"]["map_scan_error"]["mean"] - want) <= 1e-6 * want + 2.0 ** -30
    # blind: zeros, so no influence
    blind = _evaluate(env, run, vision_metrics=("depth_influence",), blind=True).result()
    assert blind["total"]["columns"]["depth_influence"] == {"mean": 0.0, "rms": 0.0, "nonfinite": 0}
    # a checkpoint on a fresh env without a sensor: sensor, map, odometry and rows are rebuilt from the record
    env2 = _env()
    from isaacgymloco_amd.envs import sensors as S
    real_from_spec = S.from_spec
    S.from_spec = lambda e, spec, **kw: real_from_spec(e, spec, **dict(kw, api=OB.EmuApi()))     # the CPU builds stand in for the library
    try:
        res2 = _evaluate(env2, path, vision_metrics=named).result()
    finally:
        S.from_spec = real_from_spec
    cam2 = env2.sensors["depth"]
    assert cam2.odometry == ODO and cam2.map == cam.map and cam2.map_channels == ("height",) and cam2.spec() == cam.spec()
    assert list(res2["total"]["columns"]) == ["depth_influence", "map_scan_error", "map_coverage"]
    assert res2["conventions"]["odometry"] == dict(ODO.record(), choice="trained")
    # passing sensor= still works; None and an override change the map's odometry, and the result says so
    env3, api3, cam3 = _map_env(points=None)
    off_ = _evaluate(env3, path, sensor=cam3, odometry=None, vision_metrics=named).result()
    assert off_["conventions"]["odometry"] == {"scale": None, "yaw_per_m": None, "z_per_m": None, "noise": None, "choice": "off"}
    assert cam3.odometry is None and cam3.stage("odometry") is None and cam3.map_pose() is env3.root_states and cam3.map_channels == ("height",)
    wide = sensors.OdometryError(scale=0.2, yaw_per_m=0.5, z_per_m=0.2)
    over = _evaluate(env3, path, sensor=cam3, odometry=wide, vision_metrics=named, steps=6).result()
    assert over["conventions"]["odometry"] == dict(wide.record(), choice="override") and cam3.odometry == wide
    assert over["total"]["columns"]["map_scan_error"]["mean"] > 0.0
    with pytest.raises(ValueError, match="odometry"):
        _evaluate(env3, path, sensor=cam3, odometry="yes")
    with pytest.raises(TypeError, match="odometry"):
        _evaluate(env3, path, sensor=cam3, odometry=0.1)
    # the command line
    base = ["--task", "aliengo", "--checkpoint", "x.pt", "--out", "y.json"]
    assert parse_args(base).odometry == "trained" and parse_args(base + ["--odometry", "off"]).odometry is None
    assert parse_args(base + ["--odometry", "scale=0.02,yaw_per_m=0.05,z_per_m=0.02,noise=0.005:0.002:0.002"]).odometry == ODO
    for bad in ("on", "scale", "drift=0.1", "scale=-1"):
        with pytest.raises(SystemExit):
            parse_args(base + ["--odometry", bad])
