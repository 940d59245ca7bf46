"""The fused elevation map through envs/sensors.py on the CPU (the emulated env and the shims): MapFusion, ElevationMap(fusion=), the
launch in the chain, map_variance(), the confidence rows, the records, and learn/evaluate.py's two columns."""
import json

import numpy as np
import pytest
import torch

import depth_memory_emu_binding as GB
import elevation_fuse_reference as FR
import elevation_map_emu_binding as EB
import elevation_map_reference as ER
import odometry_emu_binding as OB
import sensor_instrument_emu_binding as IB
import sensor_mount_jitter_emu_binding as MB
from isaacgymloco_amd.envs import sensors
from test_elevation_map_chain import FAR, SPEC_KEYS, _camera, _drive, _env, _logged
from test_map_policy_chain import GRID, _evaluate

F = np.float32
COUNTED = ("lsim_sensor_capture", "lsim_elevation_map", "lsim_elevation_map_fused", "lsim_map_rows", "lsim_map_rows_fused", "lsim_odometry_step")
NOISY = dict(clip=(0.0, FAR), noise=(0.01, 0.002))


def FusedApi():
    return GB.EmuApi(MB.lib(), IB.lib(), EB.lib(), OB.lib(), OB.rows_lib(), FR.lib(), count=COUNTED)


def test_map_fusion_values_defaults_and_text():
    f = sensors.MapFusion()
    assert (f.band, f.noise, f.var_floor, f.var_growth, f.gate, f.count_cap, f.var_max, f.camera_height) == (None, None, 2.5e-5, 1e-6, 3.0, 4, 0.25, None)
    assert sensors.MapFusion(**f.record()) == f and sensors.MapFusion(gate=2.0) != f and "gate=3.0" in repr(f)
    s0, s2, z2, band, floor, growth, vmax, gate2, cap = f.resolve((0.01, 0.002), 0.5)
    assert (s0, s2, z2, floor, growth, vmax, gate2, cap) == (0.01, 0.002, 0.25, 2.5e-5, 1e-6, 0.25, 9.0, 4)
    assert band == pytest.approx(5.0 * (0.01 + 0.002 * (2.25 + 0.25))) and f.resolve((0.0, 0.0), 0.5)[3] == 0.02 and f.resolve((0.1, 0.0), 0.5)[3] == 0.25
    assert sensors.MapFusion(band=0.1, noise=(0.02, 0.0), camera_height=0.4).resolve((0.01, 0.002), 0.5)[:4] == (0.02, 0.0, 0.4 * 0.4, 0.1)
    for bad in (dict(band=0.6), dict(band=-0.1), dict(var_floor=0.3), dict(count_cap=0), dict(gate=float("nan")), dict(noise=(-1.0, 0.0)), dict(var_growth=-1e-6)):
        with pytest.raises(ValueError):
            sensors.MapFusion(**bad)
    m = sensors.parse_elevation_map("size=16,fusion=band:0.1/gate:2/noise:0.01:0.002")
    assert m.fusion == sensors.MapFusion(band=0.1, gate=2.0, noise=(0.01, 0.002)) and sensors.parse_elevation_map("fusion=default").fusion == f
    plain = sensors.ElevationMap(size=16)
    assert "fusion" not in plain.record() and plain.fusion is None and plain != m and m.record()["fusion"] == m.fusion.record()
    assert sensors.ElevationMap(**m.record()) == m and "fusion=MapFusion(" in repr(m) and "fusion" not in repr(plain)
    with pytest.raises(TypeError):
        sensors.ElevationMap(fusion=3.0)


def test_the_fused_launch_takes_the_plain_ones_place_and_without_a_fusion_nothing_of_it_exists():
    N = 8
    env, api = _env(N), FusedApi()
    log = _logged(api, ("lsim_odometry_step", "lsim_sensor_capture", "lsim_elevation_map", "lsim_elevation_map_fused", "lsim_map_rows", "lsim_map_rows_fused"))
    cam = _camera(env, api, 16, 12, model=sensors.SensorModel(period=3, stagger=True, **NOISY))
    odo = sensors.OdometryError(scale=0.02, yaw_per_m=0.05)
    m = cam.attach_map(sensors.ElevationMap(size=32, points=GRID, fusion=sensors.MapFusion()), odometry=odo)
    rows = cam.attach_map_rows(("height", "confidence"))
    assert log == [] and cam.map is m and cam.map_channels == ("height", "confidence")
    env.add_sensor("depth", cam)
    chain = ["lsim_odometry_step", "lsim_sensor_capture", "lsim_elevation_map_fused", "lsim_map_rows_fused"]
    assert log == chain and list(cam.chain()) == chain
    st = cam.stage("map")
    assert isinstance(st.struct, sensors.abi.LsimElevationMap) and isinstance(st.outer, sensors.abi.LsimElevationMapFused)
    ef = st.outer
    h = float(cam.mount_nominal[0, 2]) + float(env.cfg.rewards.base_height_target)
    assert (ef.sigma0, ef.sigma2, ef.range_z2, ef.count_cap, ef.var_stride) == (F(0.01), F(0.002), F(h * h), 4, 99) and ef.gate2 == 9.0
    assert ef.em.root_states == cam.odometry_pose().data_ptr() and ef.var == cam.map_state()[3].data_ptr() and ef.scan_var == cam.map_variance().data_ptr()
    for _ in range(4):
        tick = env.common_step_counter
        env.step_device(torch.zeros(N, 12))
        assert ef.em.tick == tick and st.struct.tick == tick
    assert log == chain * 5 and api.calls["lsim_elevation_map"] == 0 and api.calls["lsim_map_rows"] == 0
    var, known = cam.map_variance(), cam.map_known().bool()
    assert known.any() and bool((var[known] >= F(2.5e-5)).all()) and bool((var[known] < 0.25).all()) and bool((var[~known] == 0.25).all())
    P = 99
    assert rows is cam.map_rows() and rows.shape == (N, 2 * P)
    want = FR.rows_fused(cam.map_scan().numpy(), cam.map_known().numpy(), cam.map_pose()[:, 2].numpy(), var.numpy(), 0.5, float(env.lcfg.obs_scale_height), 16 * 2.5e-5)
    np.testing.assert_array_equal(ER.bits(rows.numpy()), ER.bits(want))
    assert bool((rows[:, P:][known] > 0).all()) and bool((rows[:, P:][~known] == 0).all())
    assert cam.stage("map_rows").outer.var_ref == F(4e-4) and cam.attach_map_rows(("height", "confidence"), var_ref=1e-3) is cam.map_rows()
    assert cam.stage("map_rows").outer.var_ref == F(1e-3)
    assert cam.map_heights().shape == (N, 32, 32) and len(cam.map_state()) == 4
    # the same sensor with a plain map: the plain launches, three arrays, no variance
    cam.attach_map(sensors.ElevationMap(size=32, points=GRID))
    cam.attach_map_rows(("height", "known"))
    before = len(log)
    env.step_device(torch.zeros(N, 12))
    assert log[before:] == ["lsim_sensor_capture", "lsim_elevation_map", "lsim_map_rows"] and len(cam.map_state()) == 3
    assert set(cam.stage("map").buffers) == {"pts", "height", "stamp", "cell", "scan", "known", "state", "inv_scale"} and cam.stage("map").outer is None
    with pytest.raises(ValueError, match="fusion"):
        cam.map_variance()


def test_the_three_refusals():
    env, api = _env(), FusedApi()
    cam = env.add_sensor("depth", _camera(env, api))
    cam.attach_map(sensors.ElevationMap(size=16, points=GRID))
    with pytest.raises(ValueError, match="confidence.*fusion"):
        cam.attach_map_rows(("height", "confidence"))
    with pytest.raises(ValueError, match="var_ref"):
        cam.attach_map_rows(("height", "known"), var_ref=1e-3)
    cam.attach_map(sensors.ElevationMap(size=16, points=GRID, fusion=sensors.MapFusion(var_floor=0.0)))
    with pytest.raises(ValueError, match="var_ref"):
        cam.attach_map_rows(("height", "confidence"))
    from isaacgymloco_amd import lib
    from isaacgymloco_amd.learn.map_policy import MapOnPolicyRunner
    old = _camera(env, OB.EmuApi())
    with pytest.raises(lib.LsimError, match="lsim_elevation_map_fused"):
        old.attach_map(sensors.ElevationMap(fusion=sensors.MapFusion()))          # a library from before the entry point
    cam.attach_map(sensors.ElevationMap(size=16, points=GRID))
    with pytest.raises(ValueError, match="confidence"):
        MapOnPolicyRunner(env, {}, sensor=cam, channels=("height", "confidence"))


def test_spec_and_from_spec_carry_the_fusion():
    env, api = _env(), FusedApi()
    m = sensors.ElevationMap(size=16, points=GRID, fusion=sensors.MapFusion(band=0.08, gate=2.5, count_cap=2))
    cam = env.add_sensor("depth", _camera(env, api))
    cam.attach_map(sensors.ElevationMap(size=16, points=GRID))
    assert "fusion" not in cam.spec()["map"] and list(cam.spec()["map"]) == list(sensors.ElevationMap.FIELDS)
    cam.attach_map(m)
    spec = cam.spec()
    assert list(spec) == SPEC_KEYS + ["map"] and spec["map"]["fusion"] == m.fusion.record() and json.loads(json.dumps(spec)) == spec
    back = sensors.from_spec(env, spec, api=api)
    assert back.map == m and back.spec() == spec and back.stage("map").outer.band == F(0.08) and back.stage("map").outer.count_cap == 2


def _inputs(cam, env):
    em = cam.stage("map").struct
    R, N = cam.num_rays, env.num_envs
    stride = em.depth_stride
    flat = cam.history().reshape(-1).numpy()
    off = (em.depth - cam.history().data_ptr()) // 4
    depth = np.stack([flat[off + e * stride: off + e * stride + R] for e in range(N)])
    return {"root_states": env.root_states.numpy().copy(), "mount": cam.mount_nominal.numpy().copy(), "depth": depth.copy(),
            "episode_length": np.ones(N, np.int64), "labels": None}


def test_on_a_plane_with_a_noisy_camera_the_fused_map_is_closer_to_the_plane_than_the_plain_one():
    """A standing robot over the plane, sigma = 0.01 + 0.002 d^2, 8 captures, the same draws for both maps (one sensor, two maps fed its
    history in turn).  RMS of the known scan heights against the plane, fused over plain.  The numpy references alone give the ratio
    0.426 on this scene (plain 0.0132 m, fused 0.0056 m); the launches give 0.426 (0.0132 m, 0.0056 m).  A 64 x 48 image puts 1 to 4
    points into most cells, not the 10 of the one-cell simulation behind 0.07 .. 0.27, and the scan also reads cells at the footprint's
    rim that one or two captures touched.  The assertion: at most twice the references' ratio (the margin is for cells that differ
    between fp32 and fp64 at a band edge), and the references' own under 1/2 -- a condition on the scene."""
    N = 1
    env, api = _env(N, terrain="plane"), FusedApi()
    cam = _camera(env, api, 64, 48, model=sensors.SensorModel(**NOISY))
    poses = np.zeros((N, 7), np.float32)
    poses[:, 6], poses[:, 2] = 1.0, 0.45
    poses[:, 0], poses[:, 1] = [0.03], [0.02]
    fusion = sensors.MapFusion()
    rms, rms_ref = {}, {}
    for name, fu in (("plain", None), ("fused", fusion)):
        cam.attach_map(sensors.ElevationMap(size=32, fusion=fu))
        ref = None
        for k in range(8):
            _drive(env, cam, poses, k)          # tick k draws the same noise for both maps: the Philox counter is (env, tick, site, stream)
            inp, em = _inputs(cam, env), cam.stage("map").struct
            if ref is None:
                par = ER.Params(32, em.res, cam.dirs.numpy(), cam.stage("map").buffers["pts"].numpy(), cam.stage("map").buffers["inv_scale"].numpy(), 1, 1, 0,
                                em.a, em.b, em.t_lo, em.t_hi, em.unknown_drop)
                like = {"height": np.zeros((N, 32, 32), F), "stamp": np.full((N, 32, 32), -1, np.int32), "cell": np.zeros((N, 32, 32), np.uint32),
                        "scan": np.zeros((N, 187), F), "known": np.zeros((N, 187), np.uint8), "state": 0, "var": np.zeros((N, 32, 32), F),
                        "scan_var": np.zeros((N, 187), F)}
                if fu is None:
                    ref = ER.RefMap(N, par, like)
                else:
                    o = cam.stage("map").outer
                    ref = FR.RefFused(N, par, like, {k_: getattr(o, k_) for k_ in FR.FIELDS + ("count_cap",)})
            ref.step(inp, k, 0)
        known = cam.map_known().numpy().astype(bool)
        assert known.sum() > 40
        rms[name] = float(np.sqrt((cam.map_scan().numpy()[known].astype(np.float64) ** 2).mean()))
        kr = ref.known.astype(bool)
        rms_ref[name] = float(np.sqrt((np.asarray(ref.scan, np.float64)[kr] ** 2).mean()))
    ratio, ratio_ref = rms["fused"] / rms["plain"], rms_ref["fused"] / rms_ref["plain"]
    print(f"plane, noisy: plain {rms['plain']:.4f} m, fused {rms['fused']:.4f} m, ratio {ratio:.3f}; references {rms_ref['plain']:.4f}, {rms_ref['fused']:.4f}, ratio {ratio_ref:.3f}")
    assert ratio_ref < 0.5 and ratio <= 2.0 * ratio_ref


def test_the_variance_grows_on_cells_the_camera_has_left_and_not_on_cells_it_looks_at():
    N = 2
    env, api = _env(N, terrain="plane"), FusedApi()
    cam = _camera(env, api, 32, 24, model=sensors.SensorModel(**NOISY))
    cam.attach_map(sensors.ElevationMap(size=32, fusion=sensors.MapFusion(var_growth=1e-5)))
    poses = np.zeros((N, 7), np.float32)
    poses[:, 6], poses[:, 2] = 1.0, 0.45
    for k in range(12):
        _drive(env, cam, poses, k)
        poses[:, 0] += np.float32(0.0625)
    pts = cam.stage("map").buffers["pts"].numpy()
    known, var = cam.map_known().numpy().astype(bool), cam.map_variance().numpy()
    ahead, behind = known & ((pts[:, 0] >= 0.55) & (np.abs(pts[:, 1]) <= 0.3))[None], known & (pts[:, 0] <= 0.2)[None]
    assert ahead.any() and behind.any()
    v0_behind = var[behind].copy()
    poses[:, 0] -= np.float32(0.0625)
    for k in range(12, 40):
        _drive(env, cam, poses, k)           # standing still: the cells under the trunk are not seen again
    var = cam.map_variance().numpy()
    assert (var[behind] >= v0_behind + 27 * 1e-5 * 0.99).all(), "a cell the camera has left ages by var_growth per tick"
    # a cell seen at this tick holds K vm <= vm, one capture's variance: at most (0.01 + 0.002 (1 + 0.25))^2 + 2.5e-5 within 1 m of the base
    assert (var[ahead] <= 0.0125 ** 2 + 2.5e-5).all() and (var[ahead] < var[behind].min()).all(), "a cell the camera looks at does not"


def test_evaluate_reports_the_two_columns_only_with_a_fusion(tmp_path):
    from isaacgymloco_amd.learn.evaluate import MAP_FUSION_METRICS, parse_args
    from test_elevation_map_chain import _runner
    assert MAP_FUSION_METRICS == ("map_variance", "map_z2")
    env, api = _env(terrain="plane"), FusedApi()
    cam = env.add_sensor("depth", _camera(env, api, 16, 12, model=sensors.SensorModel(period=3, stagger=True, latency=1, frames=2, **NOISY)))
    run = _runner(env, cam)
    named = ("map_coverage", "map_variance", "map_z2")
    cam.attach_map(sensors.ElevationMap())
    assert list(_evaluate(env, run, steps=1, vision_metrics=named).result()["total"]["columns"]) == ["map_coverage"], "without a fusion: dropped"
    cam.attach_map(sensors.ElevationMap(fusion=sensors.MapFusion()))
    cols = _evaluate(env, run, steps=3, vision_metrics=named).result()["total"]["columns"]
    assert list(cols) == list(named) and all(c["nonfinite"] == 0 for c in cols.values())
    assert 2.5e-5 <= cols["map_variance"]["mean"] < 0.25 and 0.0 < cols["map_z2"]["mean"] < 100.0, cols
    path = str(tmp_path / "vision.pt")
    run.save(path)
    assert torch.load(path, weights_only=False)["vision"]["sensor"]["map"]["fusion"] == sensors.MapFusion().record()
    base = ["--task", "aliengo", "--checkpoint", "x.pt", "--out", "y.json"]
    assert parse_args(base + ["--vision-metrics", "map_variance,map_z2"]).vision_metrics == ("map_variance", "map_z2")
    with pytest.raises(SystemExit):
        parse_args(base + ["--vision-metrics", "map_var"])


def test_a_map_policy_reads_the_confidence_rows_and_its_checkpoint_rebuilds_them(tmp_path):
    from test_map_policy_chain import _runner
    env, api = _env(), FusedApi()
    cam = env.add_sensor("depth", _camera(env, api, 16, 12, model=sensors.SensorModel(period=3, stagger=True, **NOISY)))
    cam.attach_map(sensors.ElevationMap(size=32, points=GRID, fusion=sensors.MapFusion()))
    run = _runner(env, cam, channels=("height", "confidence"))
    assert cam.map_channels == ("height", "confidence") and run.alg.actor_critic.depth_latent_dim == 198
    run.learn(1)
    path = str(tmp_path / "map.pt")
    run.save(path)
    rec = torch.load(path, weights_only=False)["map_policy"]
    assert rec["channels"] == ["height", "confidence"] and rec["sensor"]["map"]["fusion"] == sensors.MapFusion().record()
    cols = _evaluate(env, run, steps=2, vision_metrics=("map_coverage", "map_variance", "map_z2")).result()["total"]["columns"]
    assert list(cols) == ["map_coverage", "map_variance"], "map_z2 needs the env's own 187 points"
    env2 = _env()
    cam2 = env2.add_sensor("depth", sensors.from_spec(env2, rec["sensor"], api=api))
    res = _evaluate(env2, path, steps=2, vision_metrics=("map_variance",))
    assert cam2.map_channels == ("height", "confidence") and list(res.result()["total"]["columns"]) == ["map_variance"]
