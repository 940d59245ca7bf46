"""The map's visibility clean-up through envs/sensors.py on the CPU (the emulated env and the shims): MapCleanup, ElevationMap(cleanup=),
the stage between the capture and the map's launch, map_cleared(), the records, and learn/evaluate.py's column.  The launch itself is
held to its reference in tests/test_elevation_cleanup.py."""
import json

import numpy as np
import pytest
import torch

import depth_memory_emu_binding as GB
import elevation_cleanup_reference as CR
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
ENTRIES = ("lsim_odometry_step", "lsim_sensor_capture", "lsim_elevation_map_cleanup", "lsim_elevation_map", "lsim_elevation_map_fused", "lsim_map_rows",
           "lsim_map_rows_fused")
NOISY = dict(clip=(0.0, FAR), noise=(0.01, 0.002))


def CleanupApi():
    return GB.EmuApi(MB.lib(), IB.lib(), EB.lib(), OB.lib(), OB.rows_lib(), FR.lib(), CR.lib(), count=ENTRIES)


def test_map_cleanup_values_defaults_and_text():
    c = sensors.MapCleanup()
    assert (c.margin, c.slope, c.sigma, c.min_rays, c.end_gap) == (0.05, 0.05, 3.0, 2, None) and "guess" in sensors.MapCleanup.__doc__.lower()
    assert sensors.MapCleanup(**c.record()) == c and sensors.MapCleanup(margin=0.1) != c and "min_rays=2" in repr(c)
    assert c.resolve(0.0625) == (0.05, 0.05, 3.0, 1.5 * 0.0625, 2) and sensors.MapCleanup(end_gap=0.2).resolve(0.0625)[3] == 0.2
    assert c.margin > np.sqrt(2.0) * 0.0625 * 0.25, "the header's condition for the default map on stairs-steep ground"
    for bad in (dict(margin=-0.01), dict(slope=float("nan")), dict(sigma=float("inf")), dict(min_rays=0), dict(end_gap=-1.0)):
        with pytest.raises(ValueError):
            sensors.MapCleanup(**bad)
    m = sensors.parse_elevation_map("size=16,cleanup=margin:0.05/min_rays:3")
    assert m.cleanup == sensors.MapCleanup(margin=0.05, min_rays=3) and sensors.parse_elevation_map("cleanup=default").cleanup == c
    both = sensors.parse_elevation_map("fusion=band:0.1,cleanup=end_gap:0.2/sigma:2")
    assert both.fusion == sensors.MapFusion(band=0.1) and both.cleanup == sensors.MapCleanup(end_gap=0.2, sigma=2.0)
    plain = sensors.ElevationMap(size=16)
    assert "cleanup" not in plain.record() and plain.cleanup is None and plain != m and m.record()["cleanup"] == m.cleanup.record()
    assert sensors.ElevationMap(**m.record()) == m and "cleanup=MapCleanup(" in repr(m) and "cleanup" not in repr(plain)
    assert sensors.ElevationMap(**both.record()) == both and list(both.record())[-2:] == ["fusion", "cleanup"]
    with pytest.raises(TypeError):
        sensors.ElevationMap(cleanup=3.0)


@pytest.mark.parametrize("fused", [False, True])
def test_the_stage_sits_between_the_capture_and_the_map_and_goes_with_it(fused):
    N = 8
    env, api = _env(N), CleanupApi()
    log = _logged(api, ENTRIES)
    cam = _camera(env, api, 16, 12, model=sensors.SensorModel(period=3, stagger=True, **NOISY))
    fusion = sensors.MapFusion() if fused else None
    m = cam.attach_map(sensors.ElevationMap(size=32, points=GRID, fusion=fusion, cleanup=sensors.MapCleanup(min_rays=3)), odometry=sensors.OdometryError(scale=0.02))
    cam.attach_map_rows(("height", "known"))
    assert log == [] and cam.map is m and cam.map_cleanup == sensors.MapCleanup(min_rays=3)
    env.add_sensor("depth", cam)
    chain = ["lsim_odometry_step", "lsim_sensor_capture", "lsim_elevation_map_cleanup", "lsim_elevation_map_fused" if fused else "lsim_elevation_map", "lsim_map_rows"]
    assert log == chain and list(cam.chain()) == chain
    assert sensors._ORDER == ("rays", "odometry", "mount_jitter", "instrument", "capture", "map", "map_rows", "encoder", "memory")
    st, mp = cam.stage("map_cleanup"), cam.stage("map")
    assert isinstance(st.struct, sensors.abi.LsimElevationMap) and isinstance(st.outer, sensors.abi.LsimElevationMapCleanup)
    ec, em = st.outer, mp.struct
    for name, _ in sensors.abi.LsimElevationMap._fields_:
        if name not in ("tick", "flags"):
            assert getattr(ec.em, name) == getattr(em, name), name
    assert ec.em.root_states == cam.odometry_pose().data_ptr() and ec.cleared == cam.map_cleared().data_ptr()
    assert ec.var == (cam.map_state()[3].data_ptr() if fused else None)
    assert (ec.clear_margin, ec.clear_slope, ec.clear_sigma, ec.end_gap, ec.min_rays) == (F(0.05), F(0.05), 3.0, F(1.5 * 0.0625), 3)
    assert set(st.buffers) == {"cleared"} and cam.map_cleared().dtype == torch.int32 and cam.map_cleared().shape == (N,)
    for _ in range(4):
        tick = env.common_step_counter
        env.step_device(torch.zeros(N, 12))
        assert ec.em.tick == tick and em.tick == tick
    assert log == chain * 5 and bool((cam.map_cleared() >= 0).all()) and int(cam.map_nonfinite) == 0
    # the same sensor without the option: the chain and every array are the ones of before
    cam.attach_map(sensors.ElevationMap(size=32, points=GRID, fusion=fusion))
    before = len(log)
    env.step_device(torch.zeros(N, 12))
    assert log[before:] == [chain[1], chain[3]] and cam.stage("map_cleanup") is None and cam.map_cleanup is None
    want = {"pts", "height", "stamp", "cell", "scan", "known", "state", "inv_scale"} | ({"var", "scan_var"} if fused else set())
    assert set(cam.stage("map").buffers) == want
    with pytest.raises(ValueError, match="clean-up"):
        cam.map_cleared()
    # detach: the stage leaves with the map
    cam.attach_map(sensors.ElevationMap(size=32, cleanup=sensors.MapCleanup()))
    assert cam.stage("map_cleanup") is not None
    assert cam.attach_map(None) is None and cam.stage("map_cleanup") is None and cam.stage("map") is None and list(cam.chain()) == ["lsim_sensor_capture"]
    from isaacgymloco_amd import lib
    with pytest.raises(lib.LsimError, match="lsim_elevation_map_cleanup"):
        _camera(env, OB.EmuApi()).attach_map(sensors.ElevationMap(cleanup=sensors.MapCleanup()))          # a library from before the entry point


def test_spec_from_spec_and_the_checkpoint_records_carry_the_cleanup(tmp_path):
    from test_elevation_map_chain import _runner as vision_runner
    from test_map_policy_chain import _runner as map_runner
    env, api = _env(), CleanupApi()
    m = sensors.ElevationMap(size=32, points=GRID, cleanup=sensors.MapCleanup(margin=0.08, min_rays=3, end_gap=0.1))
    cam = env.add_sensor("depth", _camera(env, api, 16, 12))
    cam.attach_map(sensors.ElevationMap(size=32, points=GRID))
    assert "cleanup" not in cam.spec()["map"] and list(cam.spec()["map"]) == list(sensors.ElevationMap.FIELDS)
    cam.attach_map(m)
    spec = cam.spec()
    assert list(spec) == SPEC_KEYS + ["map"] and spec["map"]["cleanup"] == m.cleanup.record() and json.loads(json.dumps(spec)) == spec
    back = sensors.from_spec(env, spec, api=api)
    assert back.map == m and back.spec() == spec and back.stage("map_cleanup").outer.min_rays == 3 and back.stage("map_cleanup").outer.end_gap == F(0.1)
    path = str(tmp_path / "vision.pt")
    vision_runner(env, cam).save(path)
    assert torch.load(path, weights_only=False)["vision"]["sensor"]["map"]["cleanup"] == m.cleanup.record()
    path = str(tmp_path / "map.pt")
    map_runner(env, cam).save(path)
    rec = torch.load(path, weights_only=False)["map_policy"]
    assert rec["sensor"]["map"]["cleanup"] == m.cleanup.record()
    env2 = _env()
    assert sensors.from_spec(env2, rec["sensor"], api=api).map_cleanup == m.cleanup


# the scan points of the phantom scene: the centres of the 24 x 10 cells ahead of a robot that stands at a cell's centre
AHEAD = [[i / 16.0, j / 16.0] for i in range(10, 34) for j in range(-5, 5)]
PHANTOM = 0.5


def crossed_and_not_hit(cam, poses, e):
    """indices into AHEAD of the cells that, by the float64 reference, at least min_rays rays of env e's next capture certainly pass below
    a height of PHANTOM, and that no ray of it ends in.  On a plane a robot that only translates captures the same depths again:
    cam.out is the next capture's, which the caller asserts afterwards"""
    em, mp = cam.stage("map").struct, cam.stage("map").buffers
    par = ER.Params(32, em.res, cam.dirs.cpu().numpy(), mp["pts"].cpu().numpy(), mp["inv_scale"].cpu().numpy(), 1, 1, 0, em.a, em.b, em.t_lo, em.t_hi, em.unknown_drop)
    N = poses.shape[0]
    rs = np.zeros((N, 13), F)
    rs[:, :7] = poses
    inp = {"root_states": rs, "mount": cam.mount_nominal.cpu().numpy(), "depth": cam.out.cpu().numpy().copy(), "labels": None}
    wix, wiy = CR.window_cells(par, rs[e])
    full = {"stamp": np.zeros((N, 32, 32), np.int32), "cell": np.broadcast_to(ER.pack(wix, wiy), (N, 32, 32)), "height": np.full((N, 32, 32), PHANTOM, F)}
    cp = dict(zip(("clear_margin", "clear_slope", "clear_sigma", "end_gap", "min_rays"), sensors.MapCleanup().resolve(em.res)))
    known, certain, ambiguous = CR.classify(par, {k: (v if k == "min_rays" else float(F(v))) for k, v in cp.items()}, inp, full, e)
    P, valid = ER.points(par, inp, e)
    hit = {(int(x), int(y)) for x, y in np.floor(P[valid, :2] * par.rinv)}
    chosen = []
    for j, (x, y) in enumerate(AHEAD):
        ix, iy = int(np.floor((float(poses[e, 0]) + x) * 16.0)), int(np.floor((float(poses[e, 1]) + y) * 16.0))
        if certain[ix & 31, iy & 31] >= cp["min_rays"] and ambiguous[ix & 31, iy & 31] == 0 and (ix, iy) not in hit:
            chosen.append((j, ix, iy))
    return chosen, inp["depth"]


def phantom_run(env, cam, cleanup, steps=4):
    """a robot walking a cell per tick over flat ground with a clean camera and the true pose; before the last tick the cells of
    crossed_and_not_hit are set to PHANTOM.  Returns per env (the scan points planted, known and scan there afterwards) and cleared or None"""
    N = env.num_envs
    cam.attach_map(sensors.ElevationMap(size=32, source="clean", points=AHEAD, cleanup=cleanup))
    poses = np.zeros((N, 7), F)
    poses[:, 6], poses[:, 2] = 1.0, 0.45
    poses[:, 0], poses[:, 1] = 0.03125 + 3.0 * np.arange(N), 0.03125
    for k in range(steps):
        _drive(env, cam, poses, k)
        poses[:, 0] += F(0.0625)
    h, st, ce = cam.map_state()[:3]
    planted = []
    for e in range(N):
        chosen, depth = crossed_and_not_hit(cam, poses, e)
        for j, ix, iy in chosen:
            s = (e, ix & 31, iy & 31)
            h[s], st[s], ce[s] = PHANTOM, steps - 1, int(np.asarray(ER.pack(ix, iy)).view(np.int32))
        planted.append([j for j, _, _ in chosen])
    _drive(env, cam, poses, steps)
    np.testing.assert_array_equal(cam.out.cpu().numpy(), depth, err_msg="on a plane a translated robot captures the same depths")
    known, scan = cam.map_known().cpu().numpy(), cam.map_scan().cpu().numpy()
    return planted, [known[e, planted[e]] for e in range(N)], [scan[e, planted[e]] for e in range(N)], None if cleanup is None else cam.map_cleared().cpu().numpy().copy()


def check_phantoms(env, cam):
    planted, known, scan, _ = phantom_run(env, cam, None)
    assert all(len(p) >= 4 for p in planted), "a condition on the scene: cells the capture sees through and does not hit"
    assert all((k == 1).all() and (s == F(PHANTOM)).all() for k, s in zip(known, scan)), "without the clean-up the phantoms stay: the policy reads obstacles"
    again, known, scan, cleared = phantom_run(env, cam, sensors.MapCleanup())
    unknown = F(F(0.45) - F(env.cfg.rewards.base_height_target))
    assert again == planted and all((k == 0).all() and (s == unknown).all() for k, s in zip(known, scan)), "with it they are forgotten after the next capture"
    assert all(c == len(p) for c, p in zip(cleared, planted)), "and nothing else is: flat ground, a clean camera, the true pose"
    print(f"phantom cells planted and forgotten per env: {[len(p) for p in planted]}")


def test_planted_phantom_cells_in_front_of_a_walking_robot_are_forgotten_and_stay_without_the_cleanup():
    env, api = _env(2, terrain="plane"), CleanupApi()
    check_phantoms(env, _camera(env, api, 16, 12, model=sensors.SensorModel(clip=(0.0, FAR))))


def test_on_stairs_with_a_clean_camera_and_the_true_pose_the_share_forgotten_is_printed():
    """no value is asserted: nobody has measured what is right.  Recorded in DESIGN.md 7.23"""
    N = 8
    env, api = _env(N), CleanupApi()
    cam = env.add_sensor("depth", _camera(env, api, 32, 24, model=sensors.SensorModel(clip=(0.0, FAR))))
    cam.attach_map(sensors.ElevationMap(size=32, source="clean", cleanup=sensors.MapCleanup()))
    g = torch.Generator().manual_seed(0)
    shares = []
    for _ in range(12):
        before = cam.map_cleared().clone()
        known = int((cam.map_state()[1] >= 0).sum())
        env.step_device(torch.randn(N, 12, generator=g) * 0.3)
        now = cam.map_cleared()
        shares.append(float(torch.where(now >= before, now - before, now).sum()) / max(known, 1))
    print("stairs, clean source, true pose: share of the known cells forgotten per capture " + " ".join(f"{100.0 * s:.3f}%" for s in shares))
    assert all(np.isfinite(shares)) and int(cam.map_nonfinite) == 0


def drifting_run(env, cam, cleanup, ticks=76, lap=60, radius=0.5, z_per_m=0.1):
    """robots walking a circle of `radius` over flat ground, `lap` ticks a round and a quarter round more, the map placed with an
    estimated pose whose height drifts by up to z_per_m per metre, a noisy camera: on the second round the camera looks at ground it
    mapped 3 m of travel ago (a forward camera on a straight path never does: what lies ahead was refreshed by the capture before).
    Returns (the mean over envs and ticks of the mean squared error of the known scan points against the plane as the estimate sees
    it, in m^2; cells forgotten in all)"""
    N = env.num_envs
    cam.attach_map(sensors.ElevationMap(size=32, cleanup=cleanup), odometry=sensors.OdometryError(z_per_m=z_per_m))
    poses = np.zeros((N, 7), F)

    def place(k):
        th = 2.0 * np.pi * k / lap
        poses[:, 0], poses[:, 1], poses[:, 2] = 3.0 * np.arange(N) + radius * np.sin(th), radius * (1.0 - np.cos(th)), 0.45
        poses[:, 5], poses[:, 6] = np.sin(th / 2.0), np.cos(th / 2.0)
    place(0)
    env.root_states[:, :7] = torch.as_tensor(poses)
    cam.refresh(tick=0)                     # every env fresh: the episode's biases are drawn
    errors, forgotten = [], 0
    for k in range(1, ticks):
        place(k)
        before = None if cleanup is None else cam.map_cleared().clone()
        _drive(env, cam, poses, k)
        if cleanup is not None:
            forgotten += int((cam.map_cleared() - before).sum())
        known = cam.map_known().to(torch.float32)
        plane = (cam.map_pose()[:, 2:3] - env.root_states[:, 2:3])          # z = 0 in the estimate's frame
        errors.append(float((((cam.map_scan() - plane).square() * known).sum(dim=1) / known.sum(dim=1).clamp(min=1.0)).mean()))
    assert int(cam.map_nonfinite) == 0
    return float(np.mean(errors)), forgotten


def test_with_a_drifting_height_and_a_noisy_camera_stale_cells_are_forgotten():
    """the scan error over the known points with and without the clean-up, printed and recorded in DESIGN.md 7.23; asserted: both runs are
    finite and the clean-up forgets at least one cell"""
    out = {}
    for name, cleanup in (("without", None), ("with", sensors.MapCleanup())):
        env, api = _env(8, terrain="plane"), CleanupApi()
        cam = _camera(env, api, 32, 24, model=sensors.SensorModel(**NOISY))
        out[name] = drifting_run(env, cam, cleanup)
    print(f"plane, noisy source, z_per_m 0.1, a circle of 0.5 m, 75 captures: mean squared scan error over the known points {out['without'][0]:.6f} m^2 without, "
          f"{out['with'][0]:.6f} m^2 with the clean-up, which forgot {out['with'][1]} cells")
    assert np.isfinite(out["without"][0]) and np.isfinite(out["with"][0]) and out["with"][1] >= 1


def test_evaluate_reports_map_cleared_only_with_a_cleanup():
    from isaacgymloco_amd.learn.evaluate import MAP_CLEANUP_METRICS, parse_args
    from test_elevation_map_chain import _runner
    assert MAP_CLEANUP_METRICS == ("map_cleared",)
    named = ("map_scan_error", "map_coverage", "map_cleared")
    env, api = _env(), CleanupApi()
    cam = env.add_sensor("depth", _camera(env, api, 16, 12, model=sensors.SensorModel(period=3, stagger=True, latency=1, frames=2, **NOISY)))
    run = _runner(env, cam)
    cam.attach_map(sensors.ElevationMap())
    assert list(_evaluate(env, run, steps=1, vision_metrics=named).result()["total"]["columns"]) == list(named[:2]), "without a clean-up: dropped"
    cam.attach_map(sensors.ElevationMap(cleanup=sensors.MapCleanup()), odometry=sensors.OdometryError(z_per_m=0.05))
    cols = _evaluate(env, run, steps=3, vision_metrics=named).result()["total"]["columns"]
    assert list(cols) == list(named) and all(c["nonfinite"] == 0 and np.isfinite(c["mean"]) for c in cols.values()) and cols["map_cleared"]["mean"] >= 0.0
    base = ["--task", "aliengo", "--checkpoint", "x.pt", "--out", "y.json"]
    assert parse_args(base + ["--vision-metrics", "map_cleared"]).vision_metrics == ("map_cleared",)
    with pytest.raises(SystemExit):
        parse_args(base + ["--vision-metrics", "map_clear"])
