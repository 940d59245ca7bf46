"""CPU: foot scans through the Python surface -- envs/sensors.py FootScan, TerrainFootScan, attach_map_rows with the foot channels, spec() /
from_spec(); learn/map_policy.py and learn/scan_policy.py on foot rows; learn/evaluate.py's foot metrics; learn/distill.py's refusal -- on the
emulated LeggedRobot, every launch through the CPU builds of the kernel sources.  The launch itself is held to its reference in
tests/test_foot_scan.py."""
import ctypes
import json

import numpy as np
import pytest
import torch

import eval_columns_emu_binding as CB
import foot_scan_emu_binding as FB
import foot_scan_reference as FR
from isaacgymloco_amd.envs import sensors
from test_elevation_map_chain import FAR, SPEC_KEYS, _camera, _drive, _env, _truth, bits

FEET = sensors.FootScan()
SMALL = sensors.FootScan(radii=(0.06, 0.12), counts=(4, 6), z_offset=0.02)          # K = 11
ODO = sensors.OdometryError(scale=0.02, yaw_per_m=0.05, z_per_m=0.02, noise=(0.005, 0.002, 0.002))


def _centres(feet, N):
    """[N, 4, 3] foot centres by the launch's own forward kinematics, and which envs it calls bad"""
    out, bad = np.zeros((N, 4, 3), np.float32), np.zeros(N, bool)
    for e in range(N):
        c = np.zeros(12, np.float32)
        rv = FB.lib().emu_foot_scan_centres(ctypes.byref(feet.struct), e, c.ctypes.data)
        assert rv in (0, 1)
        out[e], bad[e] = c.reshape(4, 3), rv == 1
    return out, bad


def _scene(env, feet_struct, option, channels, pose, **source):
    """the reference's scene of a live launch: the env's state as it stands"""
    tabs, _ = sensors._robot_tables(env)
    return dict(pose=pose.numpy().copy(), dof_pos=env.dof_pos.numpy().copy(), tables=tabs, env_robot=None, pattern=np.array(option.pattern(), np.float32),
                env_stride=1, channels=len(channels), z_offset=option.z_offset, scale=float(env.lcfg.obs_scale_height), **source)


def test_values_records_text_and_refusals_of_a_foot_scan():
    assert FEET.num_points == 25 and (FEET.radii, FEET.counts, FEET.centre, FEET.z_offset) == ((0.06, 0.12, 0.2), (6, 8, 10), True, 0.0)
    p = np.array(FEET.pattern())
    assert p.shape == (25, 2) and (p[0] == 0).all() and np.allclose(np.hypot(*p[1:7].T), 0.06) and np.allclose(np.hypot(*p[15:].T), 0.2)
    assert np.allclose(p[1], [0.06, 0.0]) and np.allclose(p[7], [0.12 * np.cos(np.pi / 8), 0.12 * np.sin(np.pi / 8)]), "every other ring is turned half a step"
    assert sensors.FootScan(**FEET.record()) == FEET and SMALL != FEET and json.loads(json.dumps(SMALL.record())) == SMALL.record()
    given = sensors.FootScan(pattern=[[0.0, 0.0], [0.1, -0.05]], z_offset=0.03)
    assert given.num_points == 2 and given.record()["radii"] is None and sensors.FootScan(**given.record()) == given and given.pattern() == [[0.0, 0.0], [0.1, -0.05]]
    assert sensors.parse_foot_scan("default") == FEET == sensors.parse_foot_scan("") and sensors.parse_option(sensors.FootScan, "default") == FEET
    assert sensors.parse_foot_scan("radii:0.06/0.12,counts:4/6,z_offset:0.02") == SMALL == sensors.parse_foot_scan("radii=0.06/0.12,counts=4/6,z_offset=0.02")
    assert sensors.parse_foot_scan("radii:0.1,counts:8,centre:0").num_points == 8
    assert "STATED GUESSES" in sensors.FootScan.__doc__
    for bad in (dict(radii=(0.1,), counts=(4, 4)), dict(radii=(-0.1,), counts=(4,)), dict(counts=(0, 8, 10)), dict(z_offset=float("nan")),
                dict(radii=(0.1, 0.2), counts=(32, 32)), dict(pattern=np.zeros((65, 2))), dict(pattern=np.zeros((0, 2))), dict(pattern=[[float("nan"), 0.0]])):
        with pytest.raises(ValueError):
            sensors.FootScan(**bad)
    with pytest.raises(ValueError):
        sensors.parse_foot_scan("rings:3")


def test_fk_foot_centres_are_the_simulators_and_a_reset_env_stands_under_its_new_base():
    N = 8
    env, api = _env(N), FB.EmuApi()
    feet = env.add_sensor("foot_scan", sensors.TerrainFootScan(env, SMALL, api=api))
    assert api.calls["lsim_foot_scan"] == 1, "launched once when created: the rows exist before the first step"
    g = torch.Generator().manual_seed(0)
    checked = 0
    for step in range(4):
        env.step_device(torch.randn(N, 12, generator=g) * 0.4)
        stayed = ~env.reset_buf.numpy().astype(bool)
        c, bad = _centres(feet, N)
        assert not bad.any()
        err = np.abs(c - env.feet_pos.numpy())[stayed]
        print(f"step {step}: FK foot centres against env.feet_pos, max {err.max():.2e} m over {int(stayed.sum())} envs")
        assert err.max() <= 1e-4, "a wrong link or sign moves a foot by centimetres"
        checked += int(stayed.sum())
    assert checked >= N and api.calls["lsim_foot_scan"] == 5
    # a reset by hand: rigid_body_states keeps the old feet until the next step; the launch's feet are under the NEW base
    env.root_states[2, 0:2] += 3.0          # so that the old and the new place differ by more than a robot
    before = env.root_states[2, 0:2].clone()
    env.reset_idx([2])
    assert api.calls["lsim_foot_scan"] == 6
    c, _ = _centres(feet, N)
    base = env.root_states[2, 0:2].numpy()
    assert np.abs(c[2, :, :2] - base).max() <= 0.6
    assert float((env.root_states[2, 0:2] - before).norm()) > 1.0 and np.abs(env.feet_pos[2, :, :2].numpy() - base).max() > 0.6, "the stale rows are somewhere else"


def test_on_the_plane_the_terrain_rows_are_the_clamped_foot_height_exactly():
    N = 4
    env, api = _env(N, terrain="plane"), FB.EmuApi()
    feet = env.add_sensor("foot_scan", sensors.TerrainFootScan(env, SMALL, ("foot_height", "foot_known"), api=api))
    for _ in range(2):
        env.step_device(torch.zeros(N, 12))
    c, _ = _centres(feet, N)
    K, scale = SMALL.num_points, np.float32(env.lcfg.obs_scale_height)
    want = np.clip(np.repeat(c[:, :, 2], K, axis=1) - np.float32(SMALL.z_offset), -1, 1) * scale
    np.testing.assert_array_equal(bits(feet.rows()[:, :4 * K]), bits(want))
    assert bool((feet.rows()[:, 4 * K:] == 1).all()) and bool((feet.heights() == 0).all()) and bool((feet.known() == 1).all()) and int(feet.nonfinite) == 0
    assert feet.heights().shape == (N, 4, K) and feet.rows().shape == (N, 8 * K)


def _map_env(N=8, terrain="stairs", odometry=None, w=32, h=24):
    env, api = _env(N, terrain=terrain), FB.EmuApi()
    cam = env.add_sensor("depth", _camera(env, api, w, h, model=sensors.SensorModel(clip=(0.0, FAR))))
    cam.attach_map(sensors.ElevationMap(size=32, source="clean"), odometry=odometry)
    return env, api, cam


def test_with_a_clean_map_and_the_true_pose_every_known_foot_point_reads_the_cell_the_map_shows_there():
    N = 8
    env, api, cam = _map_env(N)
    rows = cam.attach_map_rows(("foot_height", "foot_known"), foot_scan=SMALL)
    assert rows is cam.map_rows() and cam.map_channels == ("foot_height", "foot_known") and cam.foot_scan == SMALL and cam.stage("map_rows") is None
    assert cam.chain()[-2:] == ("lsim_elevation_map", "lsim_foot_scan") and api.calls["lsim_foot_scan"] == 1, "the sensor has captured: built once now"
    # a standing robot's camera sees no ground under its own feet: slide it 1.5 m ahead by hand, over what it has seen
    poses = np.zeros((N, 7), np.float32)
    poses[:, 6] = 1.0
    poses[:, :2] = env.env_origins.numpy()[:, :2] + np.array([0.4, -0.3], np.float32) + 0.05 * np.arange(N, dtype=np.float32)[:, None]
    env.dof_pos[:] = torch.tensor([0.0, 0.8, -1.5] * 4)
    for k in range(25):
        poses[:, 2] = _truth(env, poses[:, :2]) + 0.45
        _drive(env, cam, poses, k)
        poses[:, 0] += np.float32(0.0625)
    K = SMALL.num_points
    h, st, ce = cam.map_state()
    fs = cam.stage("foot_rows").struct
    assert fs.pose == env.root_states.data_ptr() and fs.height == h.data_ptr() and fs.size == 32 and fs.unknown_drop == cam.stage("map").struct.unknown_drop
    sc = _scene(env, fs, SMALL, cam.map_channels, cam.map_pose(), source=FR.MAP, G=32, res=0.0625, unknown_drop=float(fs.unknown_drop),
                height=h.numpy(), stamp=st.numpy(), cell=ce.numpy().view(np.uint32))
    ref = FR.reference(sc)
    got = dict(rows=cam.map_rows().numpy(), heights=cam.foot_heights().reshape(N, 4 * K).numpy(), known=cam.foot_known().reshape(N, 4 * K).numpy(), state=int(cam.foot_nonfinite))
    got["before"] = dict(got, state=0)
    FR.check(sc, ref, got, exact=False, label="live map source", cap=None)
    # the same through what a person sees: map_heights() in window order
    shown = cam.map_heights().numpy()
    centre = np.floor(env.root_states[:, :2].numpy().astype(np.float64) / 0.0625).astype(int)
    known = got["known"].astype(bool) & ~ref["ambiguous"]
    assert known.sum() > N * K, "the feet stand on ground the camera has seen"
    for e, i in zip(*np.nonzero(known)):
        ci = np.floor(ref["w"][e, i] / 0.0625).astype(int) - centre[e] + 16
        assert got["heights"][e, i] == shown[e, ci[0], ci[1]]
    assert not got["known"].all(), "and some points lie where it has not"


def test_with_odometry_the_foot_rows_use_the_estimated_pose():
    N = 8
    env, api, cam = _map_env(N, odometry=ODO)
    cam.attach_map_rows(("foot_height",), foot_scan=SMALL)
    g = torch.Generator().manual_seed(1)
    for _ in range(5):
        env.step_device(torch.randn(N, 12, generator=g) * 0.3)
    fs, K = cam.stage("foot_rows").struct, SMALL.num_points
    est = cam.odometry_pose()
    assert fs.pose == est.data_ptr() != env.root_states.data_ptr() and not torch.equal(est[:, :3], env.root_states[:, :3])
    h, st, ce = cam.map_state()
    sc = _scene(env, fs, SMALL, cam.map_channels, est, source=FR.MAP, G=32, res=0.0625, unknown_drop=float(fs.unknown_drop), height=h.numpy(), stamp=st.numpy(),
                cell=ce.numpy().view(np.uint32))
    got = dict(rows=cam.map_rows().numpy(), heights=cam.foot_heights().reshape(N, 4 * K).numpy(), known=cam.foot_known().reshape(N, 4 * K).numpy(), state=0)
    got["before"] = got
    FR.check(sc, FR.reference(sc), got, exact=False, label="estimated pose", cap=None)
    with pytest.raises(AssertionError):           # and not the true one
        true = dict(sc, pose=env.root_states.numpy().copy())
        FR.check(true, FR.reference(true), got, exact=False, label="true pose", cap=None)


def test_without_the_feature_the_launches_are_those_of_before_and_attach_detach_rules():
    N = 8
    env, api, cam = _map_env(N)
    cam.attach_map_rows(("height",))
    for _ in range(3):
        env.step_device(torch.zeros(N, 12))
    assert api.calls["lsim_foot_scan"] == 0 and api.calls["lsim_sensor_capture"] == 4 and api.calls["lsim_elevation_map"] == 4 and api.calls["lsim_map_rows"] == 4
    assert cam.foot_scan is None and cam.stage("foot_rows") is None and list(cam.spec()) == SPEC_KEYS + ["map"]
    assert cam.chain() == ("lsim_sensor_capture", "lsim_elevation_map", "lsim_map_rows")
    for getter in (cam.foot_heights, cam.foot_known):
        with pytest.raises(ValueError, match="foot rows"):
            getter()
    # foot rows and scan rows are not both attached
    cam.attach_map_rows(("foot_height",), foot_scan=SMALL)
    assert cam.stage("map_rows") is None and cam.map_rows().shape == (N, 4 * 11) and list(cam.spec()) == SPEC_KEYS + ["map", "foot_scan"]
    cam.attach_map_rows(("height", "known"))
    assert cam.stage("foot_rows") is None and cam.foot_scan is None and cam.map_rows().shape == (N, 2 * 187)
    cam.attach_map_rows(("foot_height",))
    assert cam.foot_scan == FEET and cam.map_rows().shape == (N, 100)
    # a new map drops them with the other rows; None detaches
    cam.attach_map(cam.map)
    assert cam.stage("foot_rows") is None and cam.map_channels is None
    cam.attach_map_rows(("foot_height",), foot_scan=SMALL)
    assert cam.attach_map_rows(None) is None and cam.stage("foot_rows") is None
    with pytest.raises(ValueError, match="foot_scan"):
        cam.attach_map_rows(("height",), foot_scan=SMALL)
    with pytest.raises(ValueError, match="confidence"):
        cam.attach_map_rows(("foot_height",), foot_scan=SMALL, var_ref=0.1)
    with pytest.raises(TypeError):
        cam.attach_map_rows(("foot_height",), foot_scan={"radii": (0.1,)})
    with pytest.raises(ValueError, match="channels"):
        cam.attach_map_rows(("foot_known",))
    with pytest.raises(ValueError, match="elevation map"):
        _camera(env, api).attach_map_rows(("foot_height",), foot_scan=SMALL)
    with pytest.raises(ValueError, match="channels"):
        sensors.TerrainFootScan(env, SMALL, ("height",), api=api)
    import odometry_emu_binding as OB
    from isaacgymloco_amd import lib
    old = _camera(env, OB.EmuApi())
    old.attach_map(sensors.ElevationMap(size=16))
    with pytest.raises(lib.LsimError, match="lsim_foot_scan"):
        old.attach_map_rows(("foot_height",))             # a library from before the entry point


def test_spec_and_from_spec_carry_the_foot_scans_record():
    env, api, cam = _map_env(odometry=ODO)
    cam.attach_map_rows(("foot_height", "foot_known"), foot_scan=SMALL)
    spec = cam.spec()
    assert list(spec) == SPEC_KEYS + ["map", "odometry", "foot_scan"] and spec["foot_scan"] == SMALL.record() and json.loads(json.dumps(spec)) == spec
    back = sensors.from_spec(env, spec, api=api)
    assert back.foot_scan == SMALL and back.map_channels == ("foot_height",) and back.spec() == spec and back.stage("foot_rows").struct.pose == back.odometry_pose().data_ptr()
    assert sensors.from_spec(env, spec, api=api, foot_scan=None).foot_scan is None
    assert sensors.from_spec(env, spec, api=api, foot_scan=FEET).foot_scan == FEET
    assert sensors.from_spec(env, spec, api=api, elevation_map=None).foot_scan is None, "without a map there is nothing to read"
    with pytest.raises(ValueError, match="foot_scan"):
        sensors.from_spec(env, spec, api=api, foot_scan="yes")


def _train_cfg(T=4):
    from isaacgymloco_amd.learn.bench_train import train_cfg_dict
    tc = train_cfg_dict("aliengo")
    tc["runner"]["num_steps_per_env"] = T
    torch.manual_seed(7)
    return tc


def _evaluate(env, policy, steps=3, **kw):
    from isaacgymloco_amd.learn.evaluate import Evaluator, evaluate
    return evaluate(env, policy, steps, commands=(0.5, 0.0, 0.0), evaluator=Evaluator(env, api=CB.EmuApi()), **kw)


def _emu_from_spec():
    """sensors.from_spec with the CPU builds standing in for the library; returns the undo"""
    real = sensors.from_spec
    sensors.from_spec = lambda e, spec, **kw: real(e, spec, **dict(kw, api=FB.EmuApi()))
    return lambda: setattr(sensors, "from_spec", real)


def test_the_map_runner_on_foot_rows_trains_and_evaluate_rebuilds_it_from_the_checkpoint(tmp_path):
    from isaacgymloco_amd.learn.map_policy import MapOnPolicyRunner
    named = ("depth_influence", "map_scan_error", "map_coverage", "foot_scan_error", "foot_scan_coverage")
    env, api, cam = _map_env(odometry=ODO, w=16, h=12)
    run = MapOnPolicyRunner(env, _train_cfg(), sensor=cam, channels=("foot_height", "foot_known"), foot_scan=FEET, device="cpu")
    ac = run.alg.actor_critic
    assert ac.depth_latent_dim == 200 and ac.actor[0].in_features == 64 + 200 and cam.map_channels == ("foot_height", "foot_known") and cam.foot_scan == FEET
    assert run.alg.latent_source() is cam.map_rows() and run.alg.storage.depth_latent.shape == (4, 8, 200)
    run.learn(2)
    assert all(bool(torch.isfinite(v).all()) for v in ac.state_dict().values())
    path = str(tmp_path / "feet.pt")
    run.save(path)
    d = torch.load(path, weights_only=False)
    assert d["map_policy"] == {"sensor": cam.spec(), "channels": ["foot_height", "foot_known"], "dim": 200} and d["map_policy"]["sensor"]["foot_scan"] == FEET.record()
    res = _evaluate(env, run, vision_metrics=named).result()
    cols = res["total"]["columns"]
    assert list(cols) == ["depth_influence", "map_coverage", "foot_scan_error", "foot_scan_coverage"], "map_scan_error is dropped for foot rows"
    assert np.isfinite(cols["foot_scan_error"]["mean"]) and cols["foot_scan_error"]["mean"] > 0.0 and 0.0 < cols["foot_scan_coverage"]["mean"] <= 1.0
    assert all(c["nonfinite"] == 0 for c in cols.values()) and "foot_scan" not in env.sensors, "the twin is no sensor of the env"
    # the checkpoint on a fresh env without a sensor: sensor, map, odometry and the foot rows with both channels come from the record
    env2 = _env()
    undo = _emu_from_spec()
    try:
        res2 = _evaluate(env2, path, vision_metrics=named).result()
        blind = _evaluate(env2, path, vision_metrics=("depth_influence", "foot_scan_coverage"), blind=True).result()
    finally:
        undo()
    cam2 = env2.sensors["depth"]
    assert cam2.foot_scan == FEET and cam2.map_channels == ("foot_height", "foot_known") and cam2.odometry == ODO and cam2.spec() == cam.spec()
    assert list(res2["total"]["columns"]) == ["depth_influence", "map_coverage", "foot_scan_error", "foot_scan_coverage"]
    assert blind["total"]["columns"]["depth_influence"] == {"mean": 0.0, "rms": 0.0, "nonfinite": 0}
    # the width rule: one channel takes at most K = 52
    env3, api3, cam3 = _map_env(w=16, h=12)
    wide = sensors.FootScan(pattern=[[0.01 * k, 0.0] for k in range(53)])
    with pytest.raises(ValueError, match="at most 272"):
        MapOnPolicyRunner(env3, _train_cfg(), sensor=cam3, channels=("foot_height",), foot_scan=wide, device="cpu")
    ok = MapOnPolicyRunner(env3, _train_cfg(), sensor=cam3, channels=("foot_height",), foot_scan=sensors.FootScan(pattern=wide.pattern()[:52]), device="cpu")
    assert ok.alg.actor_critic.actor[0].in_features == 272
    with pytest.raises(ValueError, match="foot_scan"):
        MapOnPolicyRunner(env3, _train_cfg(), sensor=cam3, channels=("height",), foot_scan=FEET, device="cpu")


def test_on_the_plane_with_a_clean_source_the_foot_scan_error_is_zero():
    """the robot is slid 1.3 m straight ahead by hand, so that every foot point lies on ground the camera has passed over.  The map then
    holds the plane to within the fp32 rounding of its points (tests/elevation_map_reference.py, eps: the bound the map's own plane test
    uses), so the rows differ from the truth by at most scale * that, and the evaluator's 2^-32 fixed-point column reads exactly 0"""
    import elevation_map_reference as ER
    from isaacgymloco_amd.learn.vision import VisionActorCritic
    N, K4 = 4, 44
    env, api = _env(N, terrain="plane"), FB.EmuApi()
    cam = _camera(env, api, 32, 24, model=sensors.SensorModel(clip=(0.0, FAR)))
    cam.attach_map(sensors.ElevationMap(size=32, source="clean"))
    cam.attach_map_rows(("foot_height",), foot_scan=SMALL)
    poses = np.zeros((N, 7), np.float32)
    poses[:, 6], poses[:, 2] = 1.0, 0.45
    poses[:, 0], poses[:, 1] = [0.03, -7.5, 12.01, 190.0], [0.02, 3.3, -4.0, -190.0]
    env.dof_pos[:] = torch.tensor([0.0, 0.8, -1.5] * 4)
    for k in range(22):
        _drive(env, cam, poses, k)
        if k < 21:
            poses[:, 0] += np.float32(0.0625)
    assert bool((cam.foot_known() == 1).all()), "every foot point lies on ground the camera has seen"
    twin = sensors.TerrainFootScan(env, SMALL, api=api)
    scale = float(env.lcfg.obs_scale_height)
    tol = scale * 2.0 * max(ER.eps(poses[e, :3], (0.3, 0.0, 0.05), FAR) for e in range(N))
    err = (cam.map_rows()[:, :K4] - twin.rows()[:, :K4]).abs().max()
    print(f"plane, clean source: max |map foot rows - terrain foot rows| = {float(err):.3e}, allowed {tol:.3e}")
    assert float(err) <= tol
    torch.manual_seed(1)
    ac = VisionActorCritic(env.num_obs, env.num_privileged_obs, env.num_one_step_obs, env.num_actions, depth_latent_dim=K4).eval()
    cols = _evaluate(env, ac, steps=1, sensor=cam, vision_metrics=("foot_scan_error", "foot_scan_coverage")).result()["total"]["columns"]
    assert cols["foot_scan_error"] == {"mean": 0.0, "rms": 0.0, "nonfinite": 0} and cols["foot_scan_coverage"]["mean"] == 1.0


def test_the_scan_runner_on_true_foot_scans_its_record_evaluate_and_the_distill_refusal(tmp_path):
    from isaacgymloco_amd.learn.distill import DistillRunner
    from isaacgymloco_amd.learn.scan_policy import ScanOnPolicyRunner
    env = _env()
    api = FB.EmuApi()
    env.add_sensor("foot_scan", sensors.TerrainFootScan(env, SMALL, ("foot_height",), api=api))        # the CPU build; the runner takes the one that is there
    run = ScanOnPolicyRunner(env, _train_cfg(), foot_scan=SMALL, device="cpu")
    ac = run.alg.actor_critic
    assert ac.depth_latent_dim == 44 and run.alg.latent_source() is env.sensors["foot_scan"].rows() and run.channels == ("foot_height",)
    run.learn(2)
    assert all(bool(torch.isfinite(v).all()) for v in ac.state_dict().values())
    assert run.policy_record() == {"offset": None, "width": 44, "dim": 44, "foot_scan": SMALL.record(), "channels": ["foot_height"]}
    path = str(tmp_path / "teacher.pt")
    run.save(path)
    d = torch.load(path, weights_only=False)
    assert d["scan_policy"] == run.policy_record()
    res = _evaluate(env, path, vision_metrics=()).result()
    assert res["total"]["samples"] > 0
    with pytest.raises(ValueError, match="scan policy"):
        _evaluate(env, path, vision_metrics=("foot_scan_error",))
    with pytest.raises(NotImplementedError, match="foot-scan teacher is not built"):
        DistillRunner(env, _train_cfg(), teacher=path, device="cpu")
    with pytest.raises(NotImplementedError, match="foot-scan teacher is not built"):
        DistillRunner(env, _train_cfg(), teacher=run, device="cpu")
    with pytest.raises(ValueError, match="TerrainFootScan"):
        ScanOnPolicyRunner(env, _train_cfg(), foot_scan=FEET, device="cpu")         # the env's sensor of that name is another pattern's
    with pytest.raises(ValueError, match="channels"):
        ScanOnPolicyRunner(_env(), _train_cfg(), channels=("foot_height",), device="cpu")


def test_records_of_the_old_form_load_unchanged(tmp_path):
    from isaacgymloco_amd.learn import policy_io
    from isaacgymloco_amd.learn.map_policy import MapOnPolicyRunner
    from isaacgymloco_amd.learn.scan_policy import ScanOnPolicyRunner
    env, api, cam = _map_env(w=16, h=12)
    run = MapOnPolicyRunner(env, _train_cfg(), sensor=cam, channels=("height",), device="cpu")
    rec = run.policy_record()
    assert sorted(rec) == ["channels", "dim", "sensor"] and "foot_scan" not in rec["sensor"] and rec["channels"] == ["height"] and rec["dim"] == 187
    path = str(tmp_path / "old.pt")
    run.save(path)
    parts = policy_io.policy_parts(env, path)
    assert parts.kind == "map" and parts.channels == ("height",) and parts.sensor_record == rec["sensor"]
    res = _evaluate(env, path, sensor=cam, vision_metrics=("map_coverage", "foot_scan_error", "foot_scan_coverage")).result()
    assert list(res["total"]["columns"]) == ["map_coverage"], "foot metrics are dropped without foot rows" and cam.foot_scan is None
    env2 = _env()
    scan = ScanOnPolicyRunner(env2, _train_cfg(), device="cpu")
    assert sorted(scan.policy_record()) == ["dim", "offset", "width"] and "foot_scan" not in env2.sensors and scan.foot_scan is None
    spath = str(tmp_path / "old_scan.pt")
    scan.save(spath)
    assert policy_io.policy_parts(env2, spath).scan == scan.policy_record()
    assert _evaluate(env2, spath, vision_metrics=()).result()["total"]["samples"] > 0
