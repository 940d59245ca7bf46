"""GPU: the foot-scan launch (lsim_foot_scan, isaacgymloco_amd/csrc/ls_foot_scan.h) on a real device: the exact scenes of
tests/foot_scan_scenes.py bit for bit against the float64 reference and the CPU build of the same source, the general scenes inside the
reference's bracket (tests/foot_scan_reference.py: the ambiguity rule and its 1 % cap), a side stream, a repeated launch, the refusals
on device memory, and end to end: 64 envs on stairs with camera, map and foot rows through the fused vision rollout and evaluate, and the
plane, where the map's foot rows are the terrain's.  Every launch covers at most 257 envs."""
import numpy as np
import pytest

import foot_scan_emu_binding as FB
import foot_scan_reference as FR
import foot_scan_scenes as FS

pytestmark = pytest.mark.gpu


def hip_rig(sc, **kw):
    from isaacgymloco_amd import lib
    return FB.Rig(sc, device="cuda:0", entry=lib.load().lsim_foot_scan, **kw)


def test_exact_scenes_on_the_device_equal_the_reference_and_the_cpu_builds_bits():
    for source, N, K, G, stride in FS.EXACT_CASES:
        sc = FS.exact_scene(source, N, K, G=G, env_stride=stride)
        label = f"source {source} N {N} K {K} G {G} stride {stride}"
        ref = FR.reference(sc)
        hip = FS.run(hip_rig, sc, exact=True, label="hip " + label, ref=ref)[0]
        emu = FS.run(FB.Rig, sc, exact=True, label="emu " + label, ref=ref)[0]
        for k in ("rows", "heights", "known"):
            assert np.array_equal(np.ascontiguousarray(hip[k]).view(np.uint8), np.ascontiguousarray(emu[k]).view(np.uint8)), f"{label}: {k}"
        assert hip["state"] == emu["state"] == 0
    sc = FS.exact_scene(FR.TERRAIN, 5, 7, mesh_type=0)
    assert (FS.run(hip_rig, sc, exact=True, label="hip plane")[0]["heights"][:, :28] == 0).all()


@pytest.mark.parametrize("source,K,G", FS.GENERAL_CASES)
def test_general_scenes_at_257_envs_stay_inside_the_references_bracket(source, K, G):
    sc = FS.general_scene(source, 257, K, G=G)
    got, ref, share = FS.run(hip_rig, sc, exact=False, label=f"hip general source {source} K {K} G {G}")
    assert share <= FR.MAX_AMBIGUOUS
    if K == 7:             # one channel, dense rows, heights and known not asked for
        rig = hip_rig(dict(sc, channels=1), outputs=False, ld_pad=0)
        assert rig.launch() == 0
        np.testing.assert_array_equal(rig.read()["rows"], got["rows"][:, :28])


def test_bad_envs_and_env_stride_on_the_device():
    base = FS.general_scene(FR.MAP, 257, 7, env_stride=3)
    sc = dict(base, pose=base["pose"].copy(), dof_pos=base["dof_pos"].copy())
    sc["pose"][3, 0] = np.nan
    sc["dof_pos"][6, 11] = np.inf
    sc["pose"][9, 5:7] = 0.0
    sc["pose"][10, 2] = np.nan                   # not visited: not counted
    got, ref, _ = FS.run(hip_rig, sc, exact=False, label="hip bad envs")
    assert got["state"] == 3 and (got["rows"][[3, 6, 9], :56] == 0).all() and not np.isnan(got["rows"]).any()


def test_a_side_stream_and_a_repeated_launch_give_identical_bits():
    import torch
    sc = FS.general_scene(FR.MAP, 257, 64, G=64)
    ref = FR.reference(sc)
    first = FS.run(hip_rig, sc, exact=False, label="current stream", ref=ref)[0]
    side = torch.cuda.Stream()
    rig = hip_rig(sc)
    with torch.cuda.stream(side):
        a = rig.run(stream=side.cuda_stream)
        assert rig.launch(stream=side.cuda_stream) == 0
    torch.cuda.synchronize()
    b = rig.read()
    for k in ("rows", "heights", "known"):
        assert np.array_equal(a[k].view(np.uint8), first[k].view(np.uint8)) and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    FR.check(sc, ref, a, exact=False, label="side stream")


def test_refusals_on_device_memory_write_nothing():
    from isaacgymloco_amd import lib
    L = lib.load()
    FS.refusals(hip_rig, lambda: L.lsim_foot_scan(None, None))


def test_foot_rows_end_to_end_through_the_fused_rollout_and_evaluate(tmp_path):
    """64 Aliengo envs on stairs with camera, map (odometry) and foot rows: six steps of the fused vision rollout store the rows the actor
    read, bit for bit; the checkpoint's record rebuilds sensor, map and foot rows on a fresh env, where the terrain twin's error is finite"""
    import torch
    from isaacgymloco_amd.envs import sensors
    from isaacgymloco_amd.learn.bench_train import train_cfg_dict
    from isaacgymloco_amd.learn.evaluate import evaluate
    from isaacgymloco_amd.learn.map_policy import MapOnPolicyRunner
    from isaacgymloco_amd.learn.vision import PackedVisionPolicy, VisionRollout
    from test_gpu_elevation_map_chain import N, _camera, _env
    bits = lambda t: t.contiguous().view(torch.int32)
    T, feet, odo = 6, sensors.FootScan(), sensors.OdometryError(scale=0.02, yaw_per_m=0.02, z_per_m=0.02, noise=(0.005, 0.002, 0.002))
    env = _env(5)
    cam = env.add_sensor("depth", _camera(env))
    cam.attach_map(sensors.ElevationMap(size=32, source="clean"), odometry=odo)
    tc = train_cfg_dict("aliengo")
    tc["runner"]["num_steps_per_env"] = T
    torch.manual_seed(5)
    run = MapOnPolicyRunner(env, tc, sensor="depth", channels=("foot_height", "foot_known"), foot_scan=feet, device="cuda:0")
    ac, alg = run.alg.actor_critic, run.alg
    assert ac.actor[0].in_features == 264 and PackedVisionPolicy.supported(ac) and run.enable_graphs() and isinstance(run.graphs, VisionRollout)
    assert cam.map_rows().shape == (N, 200) and cam.chain()[-2:] == ("lsim_elevation_map", "lsim_foot_scan")
    env.episode_length_buf[:9] = int(env.max_episode_length) - 3           # these time out, and reset, inside the rollout
    seen = []
    with torch.inference_mode():
        for t in range(T):
            seen.append(cam.map_rows().clone())
            run.graphs.step()
    run.graphs.flush()
    torch.cuda.synchronize()
    st = alg.storage
    assert int(st.dones.sum()) >= 9 and len({int(bits(s).sum()) for s in seen}) > 1
    for t in range(T):
        assert torch.equal(bits(st.depth_latent[t]), bits(seen[t])), t
    assert torch.equal(cam.map_rows()[:, 100:], cam.foot_known().reshape(N, 100).float()) and int(cam.foot_nonfinite) == 0 and int(env.nonfinite_envs) == 0
    run.graphs.end_iteration()
    st.clear()
    path = str(tmp_path / "feet.pt")
    run.save(path)
    env2 = _env(9)
    named = ("depth_influence", "map_scan_error", "foot_scan_error", "foot_scan_coverage")
    res = evaluate(env2, path, 8, commands=(0.8, 0.0, 0.0), vision_metrics=named).result()
    torch.cuda.synchronize()
    cam2, cols = env2.sensors["depth"], res["total"]["columns"]
    assert cam2.spec() == cam.spec() and cam2.map_channels == ("foot_height", "foot_known") and cam2.foot_scan == feet
    assert list(cols) == ["depth_influence", "foot_scan_error", "foot_scan_coverage"]
    assert all(c["nonfinite"] == 0 and np.isfinite(c["mean"]) for c in cols.values()) and 0.0 <= cols["foot_scan_coverage"]["mean"] <= 1.0
    print("evaluate a foot-row map policy:", {k: round(v["mean"], 6) for k, v in cols.items()})


def test_on_the_plane_with_a_clean_source_the_foot_scan_error_is_zero_on_the_device():
    """the robots are slid 1.3 m straight ahead by hand, so that every foot point lies on ground the camera has passed over; the map then
    holds the plane to within the fp32 rounding of its points (tests/elevation_map_reference.py, eps), the rows differ from the terrain
    twin's by at most scale * 2 eps, and the evaluator's 2^-32 fixed-point column reads exactly 0"""
    import torch
    import elevation_map_reference as ER
    from isaacgymloco_amd.envs import config as C
    from isaacgymloco_amd.envs import sensors
    from isaacgymloco_amd.envs.legged_robot import LeggedRobot
    from isaacgymloco_amd.learn.evaluate import evaluate, play_cfg
    from isaacgymloco_amd.learn.vision import VisionActorCritic
    N, K4, far, small = 4, 44, 5.0, sensors.FootScan(radii=(0.06, 0.12), counts=(4, 6), z_offset=0.02)
    cfg = play_cfg(C.aliengo_cfg())
    cfg.env.num_envs, cfg.terrain.mesh_type = N, "plane"
    env = LeggedRobot(cfg, sim_device="cuda:0", seed=3)
    env.reset()
    cam = sensors.depth_camera(env, 32, 24, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, near=0.05, far=far, model=sensors.SensorModel(clip=(0.0, far)))
    cam.attach_map(sensors.ElevationMap(size=32, source="clean"))
    cam.attach_map_rows(("foot_height",), foot_scan=small)
    poses = np.zeros((N, 7), np.float32)
    poses[:, 6], poses[:, 2] = 1.0, 0.45
    poses[:, 0], poses[:, 1] = [0.03, -7.5, 12.01, 190.0], [0.02, 3.3, -4.0, -190.0]
    env.dof_pos[:] = torch.tensor([0.0, 0.8, -1.5] * 4, device="cuda:0")
    for k in range(22):
        env.root_states[:, :7] = torch.as_tensor(poses, device="cuda:0")
        env.episode_length_buf[:] = 1
        cam.update(tick=k)
        if k < 21:
            poses[:, 0] += np.float32(0.0625)
    assert bool((cam.foot_known() == 1).all()), "every foot point lies on ground the camera has seen"
    twin = sensors.TerrainFootScan(env, small)
    tol = float(env.lcfg.obs_scale_height) * 2.0 * max(ER.eps(poses[e, :3], (0.3, 0.0, 0.05), far) for e in range(N))
    err = float((cam.map_rows()[:, :K4] - twin.rows()[:, :K4]).abs().max())
    print(f"plane, clean source, device: max |map foot rows - terrain foot rows| = {err:.3e}, allowed {tol:.3e}")
    assert err <= tol
    torch.manual_seed(1)
    ac = VisionActorCritic(env.num_obs, env.num_privileged_obs, env.num_one_step_obs, env.num_actions, depth_latent_dim=K4).to("cuda:0").eval()
    cols = evaluate(env, ac, 1, commands=(0.0, 0.0, 0.0), sensor=cam, vision_metrics=("foot_scan_error", "foot_scan_coverage")).result()["total"]["columns"]
    assert cols["foot_scan_error"] == {"mean": 0.0, "rms": 0.0, "nonfinite": 0} and cols["foot_scan_coverage"]["mean"] == 1.0
