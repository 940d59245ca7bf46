"""GPU: the range-sensor launch (lsim_raycast, isaacgymloco_amd/csrc/ls_raycast.h) on a real device against the float64 brute force of
tests/raycast_reference.py on the scenes of tests/raycast_scenes.py -- the acceptance rule and its constants are stated and derived in the
reference's docstring -- and envs/sensors.py on a full LeggedRobot.  Every GPU step is one launch or a few env steps."""
import ctypes

import numpy as np
import pytest

import raycast_emu_binding as EMU
import raycast_reference as REF
import raycast_scenes as S
from helpers import C, abi

pytestmark = pytest.mark.gpu


def hip_cast(sc, rs, mt, dirs, near, far, scale=None, env_stride=1):
    """the HIP launch on device copies of a scene: (out [N, R], state [4])"""
    import torch
    from isaacgymloco_amd import lib
    L = lib.load()
    dev = "cuda:0"
    N, R = rs.shape[0], dirs.shape[0]
    stride = (R + 3) // 4 * 4
    t = {"root_states": torch.from_numpy(np.ascontiguousarray(rs, np.float32)).to(dev), "mount": torch.from_numpy(np.ascontiguousarray(mt, np.float32)).to(dev),
         "dirs": torch.from_numpy(np.ascontiguousarray(dirs, np.float32)).to(dev), "out": torch.full((N, stride), float("nan"), device=dev),
         "state": torch.zeros(abi.DEFINES["LSIM_RAYCAST_STATE_WORDS"], dtype=torch.int64, device=dev)}
    rc = abi.LsimRaycast()
    for k, v in t.items():
        setattr(rc, k, v.data_ptr())
    if scale is not None:
        t["scale"] = torch.from_numpy(np.ascontiguousarray(scale, np.float32)).to(dev)
        rc.scale = t["scale"].data_ptr()
    if sc["words"] is not None:
        t["mesh"] = torch.from_numpy(np.ascontiguousarray(sc["words"])).to(dev)
        rc.mesh = t["mesh"].data_ptr()
        rc.grid_rows, rc.grid_cols = sc["words"].shape
    rc.mesh_type, rc.horizontal_scale, rc.vertical_scale, rc.border_size = sc["mesh_type"], sc["hs"], sc["vs"], sc["border"]
    rc.num_envs, rc.num_rays, rc.env_stride, rc.out_stride, rc.near, rc.far = N, R, env_stride, stride, near, far
    rv = L.lsim_raycast(ctypes.byref(rc), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rv == 0, rv
    torch.cuda.synchronize()
    return t["out"][:, :R].cpu().numpy(), t["state"].cpu().numpy()


@pytest.mark.parametrize("case", S.CASES, ids=[c[0] for c in S.CASES])
def test_hip_launch_matches_the_brute_force(case):
    sc, rs, mt, dirs, scale = S.case_inputs(case)
    got, state = hip_cast(sc, rs, mt, dirs, S.NEAR, S.FAR, scale=scale)
    assert state[0] == 0
    REF.check(sc, rs, mt, dirs, S.NEAR, S.FAR, got, scale=scale, label="hip " + case[0])


def test_hip_env_stride_and_nonfinite():
    sc, rs, mt, dirs, scale = S.case_inputs(("stairs_up", "stairs_up", 2, None, S.BORDER))
    plain, _ = hip_cast(sc, rs, mt, dirs, S.NEAR, S.FAR, scale=scale)
    strided, _ = hip_cast(sc, rs, mt, dirs, S.NEAR, S.FAR, scale=scale, env_stride=2)
    np.testing.assert_array_equal(strided[0::2], plain[0::2])
    assert np.isnan(strided[1::2]).all()
    rs[1, 0] = np.nan
    got, state = hip_cast(sc, rs, mt, dirs, S.NEAR, S.FAR, scale=scale)
    assert np.isfinite(got).all() and state[0] == len(dirs)
    np.testing.assert_array_equal(got[1], np.float32(S.FAR) * scale)
    np.testing.assert_array_equal(got[[0, 2, 3, 4]], plain[[0, 2, 3, 4]])


MOUNTS = {"aliengo": (0.30, 0.0, 0.05), "go2": (0.25, 0.0, 0.03)}


def stairs_env(num_envs=256):
    """Aliengo + Go2 on one small staircase block (border 2 m: 120 x 120 vertices, so that the brute force can take the whole mesh)"""
    from isaacgymloco_amd.envs.legged_robot import LeggedRobot
    cfg = C.mixed_cfg("aliengo", {"aliengo": 0.5, "go2": 0.5})[0]
    cfg.env.num_envs = num_envs
    cfg.terrain.num_rows, cfg.terrain.num_cols, cfg.terrain.border_size = 1, 1, 2
    cfg.terrain.terrain_proportions = [0.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    cfg.terrain.curriculum = False
    cfg.terrain.max_init_terrain_level = 0
    env = LeggedRobot(cfg, sim_device="cuda:0", seed=5)
    env.reset()
    return env


def test_sensors_on_a_mixed_robot_env_on_stairs():
    """N = 256 after 12 steps of random actions: env.sensors through add_sensor with per-robot mounts; HIP against the LS_EMU build of the same
    source on every ray (two fp32 implementations that contract differently: they may differ only where the ray is unstable), and HIP and the
    emulation both against the brute force, envelope rule, on every 16th env"""
    import torch
    from isaacgymloco_amd.envs import sensors
    env = stairs_env()
    assert env.sensors == {}
    cam = env.add_sensor("depth", sensors.depth_camera(env, 12, 8, 87.0, mount_pos=MOUNTS, pitch_deg=30.0, near=0.05, far=5.0))
    lid = env.add_sensor("lidar", sensors.lidar(env, 2, 20.0, 24, mount_pos=(0.0, 0.0, 0.12), far=6.0))
    g = torch.Generator().manual_seed(2)
    for _ in range(12):
        env.step_device((torch.randn(256, 12, generator=g) * 0.5).to("cuda:0"))
    torch.cuda.synchronize()
    assert int(cam.nonfinite_rays) == 0 and int(lid.nonfinite_rays) == 0 and int(env.nonfinite_envs) == 0
    rs = env.root_states.cpu().numpy()
    sc = {"mesh_type": int(env.lcfg.mesh_type), "words": env.buf["terrain_mesh"].cpu().numpy(), "hs": env.lcfg.horizontal_scale,
          "vs": env.lcfg.vertical_scale, "border": env.lcfg.border_size}
    assert sc["words"].shape[0] <= 130 and ((sc["words"].view(np.uint32) >> 20) & 1).any()
    ids = env.robot_ids.cpu().numpy()
    assert set(ids) == {0, 1}
    for s, far in ((cam, 5.0), (lid, 6.0)):
        hip = s.out.cpu().numpy()
        mt = s.mount.cpu().numpy()
        if s is cam:
            for k, name in enumerate(env.robot_names):
                np.testing.assert_array_equal(mt[ids == k, :3], np.broadcast_to(np.float32(MOUNTS[name]), ((ids == k).sum(), 3)))
            assert cam.image().shape == (256, 8, 12)
        scale = None if s.scale is None else s.scale.cpu().numpy()
        emu, _ = EMU.cast(sc, rs, mt, s.dirs.cpu().numpy(), 0.05, far, scale=scale)
        differ = np.abs(hip - emu) > 1e-4
        print(f"hip vs emu: {differ.mean():.4%} of {hip.size} rays differ by more than 1e-4 m; hits {np.mean(hip < far * 0.99):.2%}")
        assert differ.mean() <= REF.MAX_UNSTABLE
        assert (hip < far * 0.99).mean() > 0.3, "most rays of a camera pitched down / a lidar 0.4 m above ground must hit"
        sub = slice(0, 256, 16)
        for what, got in (("hip", hip), ("emu", emu)):
            REF.check(sc, rs[sub], mt[sub], s.dirs.cpu().numpy(), 0.05, far, got[sub], scale=scale, label=f"{what} env stairs {'camera' if s is cam else 'lidar'}")


def test_captured_graph_replay_equals_eager_bit_for_bit():
    """the launch captured in a graph reads the live root_states at replay: after more steps a replay gives what an eager launch gives"""
    import torch
    from isaacgymloco_amd.envs import sensors
    env = stairs_env(64)
    cam = sensors.depth_camera(env, 16, 12, 87.0, mount_pos=MOUNTS, pitch_deg=30.0, near=0.05, far=5.0)
    cam.update()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cam.update()
    g = torch.Generator().manual_seed(3)
    for _ in range(5):
        env.step_device((torch.randn(64, 12, generator=g) * 0.5).to("cuda:0"))
    cam.out_rows.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    replayed = cam.out.clone()
    assert bool((replayed > 0).all())
    cam.out_rows.fill_(-1.0)
    eager = cam.update().clone()
    torch.cuda.synchronize()
    assert torch.equal(replayed.view(torch.int32), eager.view(torch.int32))
    assert bool((eager < 4.9).any())
