"""GPU: the body-aware range-sensor launch (lsim_raycast_bodies, isaacgymloco_amd/csrc/ls_raycast_bodies.h) on a real device against the float64
reference of tests/raycast_bodies_reference.py on the scenes of tests/raycast_bodies_scenes.py (the rule and its constants: that reference's
docstring), against the CPU build of the same source, against lsim_raycast, in a captured graph, and through envs/sensors.py on a full
mixed-robot LeggedRobot.  Every GPU step is one launch or a few env steps and runs once."""
import ctypes

import numpy as np
import pytest

import raycast_bodies_emu_binding as BE
import raycast_bodies_reference as RB
import raycast_bodies_scenes as BS
import raycast_reference as REF
import raycast_scenes as S
from helpers import abi
from test_gpu_raycast import MOUNTS, hip_cast, stairs_env

pytestmark = pytest.mark.gpu


def hip_cast_bodies(sc, tables, env_robot, rs, th, mt, dirs, near, far, scale=None, body_mask=0x1FFFF, flags=0):
    """the HIP launch on device copies of a scene: (out [N, R], labels [N, R], state [4])"""
    import torch
    from isaacgymloco_amd import lib
    L = lib.load()
    dev = "cuda:0"
    rb, a = BE.fill(sc, tables, env_robot, rs, th, mt, dirs, near, far, scale=scale, body_mask=body_mask, flags=flags)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in a.items() if isinstance(v, np.ndarray)}
    t["robots"] = torch.from_numpy(np.frombuffer(a["robots"], dtype=np.uint8).copy()).to(dev)
    for k in ("root_states", "mount", "dirs", "out", "state", "scale", "mesh"):
        if k in t:
            setattr(rb.rc, k, t[k].data_ptr())
    rb.dof_state, rb.robots, rb.labels = t["dof_state"].data_ptr(), t["robots"].data_ptr(), t["labels"].data_ptr()
    if "env_robot" in t:
        rb.env_robot = t["env_robot"].data_ptr()
    rv = L.lsim_raycast_bodies(ctypes.byref(rb), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rv == 0, rv
    torch.cuda.synchronize()
    R = dirs.shape[0]
    return t["out"][:, :R].cpu().numpy(), t["labels"][:, :R].cpu().numpy(), t["state"].cpu().numpy()


@pytest.mark.parametrize("case", BS.CASES, ids=[c[0] for c in BS.CASES])
def test_hip_launch_matches_the_reference_and_the_cpu_build(case):
    sc, tabs, rs, th, mt, dirs, scale, flags = BS.case_inputs(case)
    out, lab, state = hip_cast_bodies(sc, tabs, BS.ENV_ROBOT, rs, th, mt, dirs, BS.NEAR, BS.FAR, scale=scale, flags=flags)
    assert state[0] == 0
    RB.check(sc, [RB.robot_dict(t) for t in tabs], BS.ENV_ROBOT, rs, th, mt, dirs, BS.NEAR, BS.FAR, out, lab, scale=scale, flags=flags, label="hip " + case[0])
    emu, elab, _, _ = BE.cast(sc, tabs, BS.ENV_ROBOT, rs, th, mt, dirs, BS.NEAR, BS.FAR, scale=scale, flags=flags)
    differ = np.abs(out - emu) > 1e-4
    print(f"hip vs emu {case[0]}: {differ.mean():.4%} of {out.size} rays differ by more than 1e-4 m, {np.mean(lab != elab):.4%} labels differ")
    assert differ.mean() <= REF.MAX_UNSTABLE and np.mean(lab != elab) <= REF.MAX_UNSTABLE


@pytest.mark.parametrize("case", [S.CASES[0], S.CASES[7], S.CASES[-1]], ids=lambda c: c[0])
def test_without_primitives_the_device_output_is_lsim_raycasts_bit_for_bit(case):
    sc, rs, mt, dirs, scale = S.case_inputs(case)
    want, _ = hip_cast(sc, rs, mt, dirs, S.NEAR, S.FAR, scale=scale)
    tabs = BS.tables()[0]
    empty = abi.LsimRaycastRobot.from_buffer_copy(tabs[0])
    empty.num_prims = 0
    th = np.tile(BS.STAND.astype(np.float32), (rs.shape[0], 1))
    for tables, mask in (([empty], 0x1FFFF), ([tabs[0]], 0)):
        out, lab, state = hip_cast_bodies(sc, tables, None, rs, th, mt, dirs, S.NEAR, S.FAR, scale=scale, body_mask=mask)
        np.testing.assert_array_equal(out.view(np.int32), want.view(np.int32))
        assert set(lab.reshape(-1).tolist()) <= {0, 1} and state[0] == 0


def _reference_check(env, s, sub, what):
    rs, th = env.root_states.cpu().numpy(), env.dof_pos.cpu().numpy()
    sc = {"mesh_type": int(env.lcfg.mesh_type), "words": env.buf["terrain_mesh"].cpu().numpy(), "hs": env.lcfg.horizontal_scale,
          "vs": env.lcfg.vertical_scale, "border": env.lcfg.border_size}
    robots = [RB.robot_dict(t) for t in s._robots_host]
    ids = env.robot_ids.cpu().numpy()
    scale = None if s.scale is None else s.scale.cpu().numpy()
    flags = RB.FRAME_YAW if s.frame == "yaw" else 0
    return RB.check(sc, robots, ids[sub], rs[sub], th[sub], s.mount.cpu().numpy()[sub], s.dirs.cpu().numpy(), s.near, s.far, s.out.cpu().numpy()[sub],
                    s.labels().cpu().numpy()[sub], scale=scale, body_mask=s.body_mask, flags=flags, label=what)


def test_see_robot_sensors_on_a_mixed_robot_env_on_stairs():
    """N = 256, Aliengo + Go2 on stairs, random actions until some envs have reset in the very step the sensors are read after: images and labels
    through add_sensor against the reference evaluated on a copy of that step's root_states / dof_state, on every 16th env and on the envs that reset"""
    import torch
    from isaacgymloco_amd.envs import sensors
    env = stairs_env()
    # three groups of envs close to their time-out, one step apart: whichever convention the counter follows, one group resets in step 12
    k = torch.arange(256, device="cuda:0") % 32
    near_end = torch.where((k >= 5) & (k <= 7), int(env.max_episode_length) - 5 - k, torch.zeros_like(k))
    env.episode_length_buf = near_end.to(env.episode_length_buf.dtype)
    cam = env.add_sensor("depth", sensors.depth_camera(env, 12, 8, 87.0, mount_pos={k: (-0.1, 0.0, 0.02) for k in MOUNTS}, pitch_deg=35.0, near=0.05, far=5.0,
                                                       see_robot=True, labels=True))
    chase = env.add_sensor("chase", sensors.depth_camera(env, 12, 8, 60.0, mount_pos=(-1.2, 0.0, 0.7), pitch_deg=28.0, near=0.05, far=5.0,
                                                         see_robot=True, labels=True, frame="yaw", ignore_bodies=("FL_calf",)))
    g = torch.Generator().manual_seed(2)
    reset_seen = None
    for _ in range(12):
        env.step_device((torch.randn(256, 12, generator=g) * 0.5).to("cuda:0"))
        reset_seen = env.reset_buf.clone()
    torch.cuda.synchronize()
    assert int(cam.nonfinite_rays) == 0 and int(chase.nonfinite_rays) == 0 and int(env.nonfinite_envs) == 0
    reset_ids = reset_seen.nonzero().flatten().cpu().numpy()
    assert len(reset_ids) > 0, "some envs must have reset in the step the sensors ran after"
    sub = np.unique(np.concatenate((np.arange(0, 256, 16), reset_ids[:8])))
    for name, s in (("camera", cam), ("chase", chase)):
        share, on_body = _reference_check(env, s, sub, f"hip env stairs {name}")
        assert on_body > 0.02
    assert cam.label_image().shape == (256, 8, 12) and not bool((chase.labels() == 2 + 3).any())


def test_captured_graph_replay_equals_eager_bit_for_bit():
    import torch
    from isaacgymloco_amd.envs import sensors
    env = stairs_env(64)
    cam = sensors.depth_camera(env, 16, 12, 87.0, mount_pos={k: (-0.1, 0.0, 0.02) for k in MOUNTS}, pitch_deg=35.0, near=0.05, far=5.0, see_robot=True, labels=True)
    cam.update()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cam.update()
    g = torch.Generator().manual_seed(3)
    for _ in range(5):
        env.step_device((torch.randn(64, 12, generator=g) * 0.5).to("cuda:0"))
    cam.out_rows.fill_(-1.0)
    cam.label_rows.fill_(255)
    graph.replay()
    torch.cuda.synchronize()
    replayed, rlab = cam.out.clone(), cam.labels().clone()
    assert bool((replayed > 0).all()) and bool((rlab < 19).all()) and bool((rlab >= 2).any())
    cam.out_rows.fill_(-1.0)
    eager = cam.update().clone()
    torch.cuda.synchronize()
    assert torch.equal(replayed.view(torch.int32), eager.view(torch.int32)) and torch.equal(rlab, cam.labels())
