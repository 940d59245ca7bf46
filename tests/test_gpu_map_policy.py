"""GPU: the map policy on a real device.  (1) The fused policy launches (lsim_policy_forward_ext, lsim_policy_act_post_at_ext) at the two widths a
map policy has and no test had run -- 187 extra columns (k_in 251, k_pad 256) and 198 (k_in 262, k_pad 272, the limit) -- against the fp64
reference with the tolerance rule of tests/mlp_shapes_rig.py (4 x the distance of the reference's fp32 twins), the store checked.  (2) The
chain odometry -> capture -> map -> rows on 64 Aliengo envs on stairs, a MapOnPolicyRunner iteration through the fused rollout, its
checkpoint and evaluate."""
import ctypes

import numpy as np
import pytest
import torch

import mlp_shapes_reference as R
import mlp_shapes_rig as G
from test_gpu_elevation_map_chain import FAR, N, _camera, _env

pytestmark = pytest.mark.gpu
DEV = G.DEV
SHIPPED = R.POLICY_CASES["shipped"]
WIDTHS = {"map187": (187, 190, 256), "map198": (198, 200, 272)}         # case: extra columns, their row stride (NaN padded), the first layer's k_pad
GRID = [[x, y] for x in np.linspace(-0.5, 0.5, 11) for y in np.linspace(-0.4, 0.4, 9)]


@pytest.fixture
def map_case(request, monkeypatch):
    """the shipped policy's widths with a map policy's extra segment, registered for the extent of one test"""
    case = request.param
    dim, ld, _ = WIDTHS[case]
    monkeypatch.setitem(R.POLICY_CASES, case, dict(SHIPPED, ext=(dim, ld)))
    monkeypatch.setitem(G._SEEDS, case, 23 + dim)
    return case


@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("map_case", list(WIDTHS), indirect=True)
def test_the_policy_launches_at_a_map_policys_widths(map_case, n):
    case = map_case
    dim, ld, k_pad = WIDTHS[case]
    sc = G.general_policy_scene(case)
    pk = G.DevicePolicy(case, sc["net"])
    first = pk.packed["actor"][0]
    assert (first["k_in"], first["k_pad"]) == (45 + 3 + 16 + dim, k_pad)
    obs, priv, ext = sc["obs"][:n], sc["priv"][:n], sc["extra"][:n]
    got = pk.forward(obs, priv, ext)                     # lsim_policy_forward_ext; guards and the NaN padding of the rows checked inside
    for i, what in enumerate(("mean", "values")):
        err = float(np.abs(got[i].astype(np.float64) - sc["ref"][i][:n]).max())
        print(case, n, what, "forward_ext max |device - fp64|", err, "tolerance", sc["tol"][i], "twin distance", sc["twin_dist"][i])
        assert np.isfinite(got[i]).all() and err <= sc["tol"][i], (case, n, what, err, sc["tol"][i])
    # lsim_policy_act_post_at_ext: the same means and values, and row `step` of the store receives the rows the actor read, nothing else
    c = R.POLICY_CASES[case]
    O, P, A, T = c["hist"] * c["n1"], c["P"], c["A"], 3
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    st, gd, S = G.storage(T, n, O, P, A)
    store, sflat = G.guarded((T, n, dim))
    mean, mflat = G.guarded((n, A))
    val, vflat = G.guarded((n, 1))
    act, aflat = G.guarded((n, A))
    rows, std = to(ext), torch.full((A,), 0.5, device=DEV)
    o, p = to(obs), to(priv)
    x = pk.extra_struct(rows, store)
    rc = pk.L.lsim_policy_act_post_at_ext(ctypes.byref(pk.P), ctypes.byref(x), ctypes.byref(S), 1, 7, o.data_ptr(), p.data_ptr(), std.data_ptr(), 5, 1,
                                          mean.data_ptr(), val.data_ptr(), act.data_ptr(), -1, None, None, None, None, ctypes.c_float(0.99),
                                          torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for flat, cnt in ((sflat, T * n * dim), (mflat, n * A), (vflat, n), (aflat, n * A)):
        assert G.guards_intact(flat, cnt), "a write outside an output"
    assert G.storage_guards_intact(gd)
    assert torch.equal(G.bits(store[1]), G.bits(rows[:, :dim])) and bool(torch.isnan(store[0]).all()) and bool(torch.isnan(store[2]).all())
    assert bool(torch.isnan(rows[:, dim:]).all())
    for i, (t, what) in enumerate(((mean, "mean"), (val, "values"))):
        err = float(np.abs(t.cpu().numpy().astype(np.float64) - sc["ref"][i][:n]).max())
        print(case, n, what, "act_post_at_ext max |device - fp64|", err, "tolerance", sc["tol"][i])
        assert err <= sc["tol"][i], (case, n, what, err, sc["tol"][i])
    assert torch.equal(G.bits(st["mu"][1]), G.bits(mean)) and torch.equal(G.bits(st["observations"][1]), G.bits(o)) and bool(torch.isfinite(act).all())
    assert float(st["mu"][0].abs().sum()) == 0 and float(st["mu"][2].abs().sum()) == 0


ODO = dict(scale=0.02, yaw_per_m=0.02, z_per_m=0.02, noise=(0.005, 0.002, 0.002))


def _map_env(seed, points=GRID, odometry=ODO):
    from isaacgymloco_amd.envs import sensors
    env = _env(seed)
    cam = env.add_sensor("depth", _camera(env))
    cam.attach_map(sensors.ElevationMap(size=32, source="clean", points=points), odometry=None if odometry is None else sensors.OdometryError(**odometry))
    return env, cam


def test_on_stairs_with_a_drifting_pose_every_known_scan_value_stays_inside_the_widened_envelope():
    """the map is placed with the estimate: its heights are the terrain's plus the dz of the launch that inserted them, at a place off by
    (dx, dy) and turned by 2 atan h about the robot.  So every known value lies between the lowest and the highest terrain vertex within
    the map's own radius (test_gpu_elevation_map_chain.envelope_violations) + the largest |dxy| + the largest yaw error x the camera's
    reach, widened in z by the largest |dz| -- the largest each was at any step, read from odometry_state()"""
    import elevation_map_reference as ER
    env, cam = _map_env(5, points=None)
    cam.attach_map_rows(("height", "known"))
    g = torch.Generator().manual_seed(2)
    worst = torch.zeros(3, device=DEV)
    for step in range(30):
        env.step_device((torch.randn(N, 12, generator=g) * 0.3).to(DEV))
        o = cam.odometry_state()
        worst = torch.maximum(worst, torch.stack((torch.linalg.vector_norm(o[:, 0:2], dim=1).max(), o[:, 2].abs().max(), o[:, 3].abs().max())))
    torch.cuda.synchronize()
    dxy, dz, h = (float(v) for v in worst)
    assert dxy > 1e-4 and dz > 1e-5 and h > 1e-5, "the estimate drifted"
    t = env.cfg.terrain
    hs, res = float(t.horizontal_scale), cam.map.resolution
    grid = env.terrain.heightsamples.astype(np.float64) * t.vertical_scale
    est = cam.odometry_pose()[:, :7].cpu().numpy().astype(np.float64)
    pts, scan, known = cam.stage("map").buffers["pts"].cpu().numpy().astype(np.float64), cam.map_scan().cpu().numpy(), cam.map_known().cpu().numpy().astype(bool)
    n = 1.0 / np.sqrt(est[:, 5] ** 2 + est[:, 6] ** 2)
    qy = np.stack((np.zeros(N), np.zeros(N), est[:, 5] * n, est[:, 6] * n), axis=1)
    w = est[:, None, :2] + ER.rot(qy[:, None, :], np.concatenate((pts, np.zeros((len(pts), 1))), axis=1)[None])[..., :2]
    eps = ER.eps(np.abs(est[:, :3]).max(axis=0), (0.3, 0.0, 0.05), FAR)
    radius = res * np.sqrt(2.0) + hs + eps + dxy + 2.0 * np.arctan(h) * (FAR + 0.35)
    k = int(np.ceil(radius / hs)) + 1
    off = np.arange(-k, k + 1)
    bad = checked = 0
    for e, j in zip(*np.nonzero(known)):
        c = np.round((w[e, j] + t.border_size) / hs).astype(int)
        a, b = np.clip(c[0] + off, 0, grid.shape[0] - 1), np.clip(c[1] + off, 0, grid.shape[1] - 1)
        near = np.hypot((a * hs - t.border_size - w[e, j, 0])[:, None], (b * hs - t.border_size - w[e, j, 1])[None, :]) <= radius
        hgt = grid[np.ix_(a, b)][near]
        checked += 1
        bad += not (hgt.min() - eps - dz <= scan[e, j] <= hgt.max() + eps + dz)
    print(f"map with odometry on stairs: {checked} known scan points, {bad} outside the envelope; largest |dxy| {dxy:.4f} m, |dz| {dz:.4f} m, |h| {h:.5f}")
    assert checked > N * 10 and bad == 0
    rows = cam.map_rows()
    assert int(cam.map_nonfinite) == 0 and bool(torch.isfinite(rows).all()) and torch.equal(rows[:, 187:], cam.map_known().float())
    want = (cam.odometry_pose()[:, 2:3] - 0.5 - cam.map_scan()).clamp(-1.0, 1.0) * float(env.lcfg.obs_scale_height)
    assert torch.equal(G.bits(rows[:, :187]), G.bits(want))


def _runner(env, channels=("height", "known"), T=6, seed=5):
    from isaacgymloco_amd.learn.bench_train import train_cfg_dict
    from isaacgymloco_amd.learn.map_policy import MapOnPolicyRunner
    tc = train_cfg_dict("aliengo")
    tc["runner"]["num_steps_per_env"] = T
    torch.manual_seed(seed)
    return MapOnPolicyRunner(env, tc, sensor="depth", channels=channels, device=DEV)


def test_map_policy_end_to_end(tmp_path):
    from isaacgymloco_amd.envs import sensors
    from isaacgymloco_amd.learn.evaluate import evaluate
    from isaacgymloco_amd.learn.fused_policy import PackedHimPolicy
    from isaacgymloco_amd.learn.modules import HIMActorCritic
    from isaacgymloco_amd.learn.vision import PackedVisionPolicy, VisionRollout
    T, L = 6, 198
    env, cam = _map_env(5)
    run = _runner(env, T=T)
    ac, alg = run.alg.actor_critic, run.alg
    assert ac.actor[0].in_features == 262 and PackedVisionPolicy.supported(ac)
    assert run.enable_graphs() and isinstance(run.graphs, VisionRollout)
    assert cam.map_rows().shape == (N, L) and alg.storage.depth_latent.shape == (T, N, L)
    env.episode_length_buf[:9] = int(env.max_episode_length) - 3           # these time out, and reset, inside the rollout
    seen = []
    with torch.inference_mode():
        for t in range(T):
            seen.append(cam.map_rows().clone())         # the rows an eager act() would read and store
            run.graphs.step()
    run.graphs.flush()
    torch.cuda.synchronize()
    st = alg.storage
    assert int(st.dones.sum()) >= 9 and len({int(G.bits(s).sum()) for s in seen}) > 1
    for t in range(T):
        assert torch.equal(G.bits(st.depth_latent[t]), G.bits(seen[t])), t
        with torch.no_grad():
            ref = ac.act_inference(st.observations[t], st.depth_latent[t])
        torch.testing.assert_close(st.mu[t], ref, rtol=2e-4, atol=2e-5 * float(ref.abs().max()))
    run.graphs.end_iteration()
    st.clear()
    before = ac.state_dict()["actor.0.weight"].clone()
    run.learn(1)
    assert len(run.last_update) == 4 and all(np.isfinite(float(v)) for v in run.last_update)
    after = ac.state_dict()
    assert all(bool(torch.isfinite(v).all()) for v in after.values()) and bool((after["actor.0.weight"][:, 64:] != before[:, 64:]).any())
    assert int(env.nonfinite_envs) == 0 and int(cam.map_nonfinite) == 0
    # warm start: with zero map columns the launch computes the HIM launch's means bit for bit, whatever the rows hold
    torch.manual_seed(3)
    him = HIMActorCritic(env.num_obs, env.num_privileged_obs, env.num_one_step_obs, env.num_actions).to(DEV).eval()
    ac.load_him_state_dict(him.state_dict())
    obs, priv = env.get_observations(), env.get_privileged_observations()
    m1, m0, v = (torch.empty(N, 12, device=DEV), torch.empty(N, 12, device=DEV), torch.empty(N, 1, device=DEV))
    PackedVisionPolicy(ac).forward(obs, priv, m1, v, rows=cam.map_rows())
    PackedHimPolicy(him).forward(obs, priv, m0, v)
    torch.cuda.synchronize()
    assert torch.equal(G.bits(m1), G.bits(m0)) and bool(cam.map_rows().abs().sum() > 0)
    # the checkpoint, and evaluate on it: an env without a sensor gets sensor, map, odometry and rows from the record
    path = str(tmp_path / "map.pt")
    run.save(path)
    record = torch.load(path, map_location="cpu", weights_only=False)["map_policy"]
    assert record == {"sensor": cam.spec(), "channels": ["height", "known"], "dim": L} and record["sensor"]["odometry"] == sensors.OdometryError(**ODO).record()
    env2 = _env(9)
    named = ("depth_influence", "map_scan_error", "map_coverage")
    res = evaluate(env2, path, 10, commands=(0.8, 0.0, 0.0), vision_metrics=named).result()
    torch.cuda.synchronize()
    cam2 = env2.sensors["depth"]
    assert cam2.spec() == cam.spec() and cam2.map_channels == ("height", "known")
    cols = res["total"]["columns"]
    assert list(cols) == ["depth_influence", "map_coverage"], "99 points are not the privileged scan's 187: its error has no reference"
    assert all(c["nonfinite"] == 0 and np.isfinite(c["mean"]) for c in cols.values()) and 0.0 < cols["map_coverage"]["mean"] <= 1.0
    assert res["conventions"]["odometry"] == dict(sensors.OdometryError(**ODO).record(), choice="trained")
    blind = evaluate(env2, path, 3, commands=(0.8, 0.0, 0.0), vision_metrics=("depth_influence",), blind=True, odometry=None).result()
    assert blind["total"]["columns"]["depth_influence"]["mean"] == 0.0 and blind["conventions"]["odometry"]["choice"] == "off" and cam2.odometry is None
    print("evaluate a map policy:", {k: round(v["mean"], 5) for k, v in cols.items()})
