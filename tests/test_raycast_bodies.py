"""CPU: the body-aware range-sensor source (isaacgymloco_amd/csrc/ls_raycast_bodies.h) compiled by g++ under LS_EMU, against the float64
reference of tests/raycast_bodies_reference.py (whose docstring states the acceptance rule), against closed forms, against lsim_raycast's
emulated launch, and through envs/sensors.py.  The same scenes run on the HIP launch in tests/test_gpu_raycast_bodies.py."""
import ctypes
import math

import numpy as np
import pytest

import raycast_bodies_emu_binding as BE
import raycast_bodies_reference as RB
import raycast_bodies_scenes as BS
import raycast_emu_binding as EMU
import raycast_reference as REF
import raycast_scenes as S
from helpers import abi

ID = np.array([0, 0, 0, 1], np.float32)


@pytest.mark.parametrize("case", BS.CASES, ids=[c[0] for c in BS.CASES])
def test_emulated_launch_matches_the_reference(case):
    sc, tabs, rs, th, mt, dirs, scale, flags = BS.case_inputs(case)
    out, lab, state, _ = BE.cast(sc, tabs, BS.ENV_ROBOT, rs, th, mt, dirs, BS.NEAR, BS.FAR, scale=scale, flags=flags)
    assert state[0] == 0
    share, on_body = RB.check(sc, [RB.robot_dict(t) for t in tabs], BS.ENV_ROBOT, rs, th, mt, dirs, BS.NEAR, BS.FAR, out, lab, scale=scale, flags=flags,
                              label=case[0])
    assert on_body > 0.02, "the scene must show the robot"


# ---- closed forms: one primitive on the base at a known pose
def one_prim(kind, pos, quat, size, body=0):
    t = abi.LsimRaycastRobot.from_buffer_copy(BS.tables()[0][0])
    t.num_prims = 1
    p = t.prims[0]
    p.kind, p.body = kind, body
    for k in range(3):
        p.pos[k], p.size[k] = pos[k], size[k]
    for k in range(4):
        p.quat[k] = quat[k]
    return t


def shoot(table, origin, dirs, near=0.05, far=5.0, base=(0.0, 0.0, 2.0), mask=0x1FFFF, scene=None, th=None):
    """rays from base + origin (identity base orientation) over the plane z = 0 (or `scene`): (out [R], labels [R])"""
    rs = np.zeros((1, 13), np.float32)
    rs[0, :3], rs[0, 3:7] = base, ID
    mt = np.array([list(origin) + [0, 0, 0, 1]], np.float32)
    d = np.asarray(dirs, np.float64)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    out, lab, state, _ = BE.cast(scene or REF.plane_scene(), [table], None, rs, np.zeros((1, 12), np.float32) if th is None else th, mt, d, near, far, body_mask=mask)
    assert state[0] == 0
    return out[0], lab[0]


TOL = REF.ATOL + REF.C_TOL * 2.0 ** -23 * 2.0      # the reference's tolerance at coordinate + t = 2 m, normal incidence


def test_each_kind_under_a_vertical_and_an_oblique_ray():
    s = math.sqrt(0.5)
    rot_y90 = (0.0, s, 0.0, s)              # local z -> world x
    # sphere r = 0.1 at the base origin, sensor 1 m above: vertical 0.9; oblique through the centre from (-1, 0, 1): sqrt(2) - 0.1
    out, lab = shoot(one_prim(RB.SPHERE, (0, 0, 0), ID, (0.1, 0, 0)), (0, 0, 1), [(0, 0, -1)])
    assert abs(out[0] - 0.9) <= TOL and lab[0] == 2
    out, lab = shoot(one_prim(RB.SPHERE, (0, 0, 0), ID, (0.1, 0, 0)), (-1, 0, 1), [(1, 0, -1)])
    assert abs(out[0] - (math.sqrt(2) - 0.1)) <= TOL and lab[0] == 2
    # box half extents (0.3, 0.1, 0.05): top face at 0.05; oblique (1, 0, -1) from (-0.5, 0, 0.5) meets the top at x = -0.05, t = 0.45 sqrt 2
    box = one_prim(RB.BOX, (0, 0, 0), ID, (0.3, 0.1, 0.05))
    out, lab = shoot(box, (0, 0, 1), [(0, 0, -1)])
    assert abs(out[0] - 0.95) <= TOL and lab[0] == 2
    out, lab = shoot(box, (-0.5, 0, 0.5), [(1, 0, -1)])
    assert abs(out[0] - 0.45 * math.sqrt(2)) <= TOL / s and lab[0] == 2
    # the same box turned by 90 degrees about y: half extents along world (z, y, x) = (0.3, 0.1, 0.05): top at 0.3
    out, lab = shoot(one_prim(RB.BOX, (0, 0, 0), rot_y90, (0.3, 0.1, 0.05)), (0, 0, 1), [(0, 0, -1)])
    assert abs(out[0] - 0.7) <= TOL and lab[0] == 2
    # capsule r = 0.05, half length 0.2, axis along world x: vertical onto the side 0.95; vertical at x = 0.23 onto the end sphere;
    # oblique (1, 0, -1) from (-0.6, 0, 0.4) towards the centre line point (-0.2, 0, 0): the end sphere's centre, t = 0.4 sqrt 2 - 0.05
    cap = one_prim(RB.CAPSULE, (0, 0, 0), rot_y90, (0.05, 0.2, 0))
    out, lab = shoot(cap, (0, 0, 1), [(0, 0, -1)])
    assert abs(out[0] - 0.95) <= TOL and lab[0] == 2
    out, lab = shoot(cap, (0.23, 0, 1), [(0, 0, -1)])
    assert abs(out[0] - (1.0 - math.sqrt(0.05 ** 2 - 0.03 ** 2))) <= TOL and lab[0] == 2
    out, lab = shoot(cap, (-0.6, 0, 0.4), [(1, 0, -1)])
    assert abs(out[0] - (0.4 * math.sqrt(2) - 0.05)) <= TOL and lab[0] == 2
    # flat-capped cylinder, same pose: the side as the capsule's; at x = 0.23 nothing (the plane 2 m below the base: 3.0);
    # along the axis from (-1, 0, 0.02): the cap at x = -0.2, t = 0.8; oblique (1, 0, -1) from (-0.5, 0, 0.5): the side at x = -0.05, z = 0.05, t = 0.45 sqrt 2
    cyl = one_prim(RB.CYLINDER, (0, 0, 0), rot_y90, (0.05, 0.2, 0))
    out, lab = shoot(cyl, (0, 0, 1), [(0, 0, -1)])
    assert abs(out[0] - 0.95) <= TOL and lab[0] == 2
    out, lab = shoot(cyl, (0.23, 0, 1), [(0, 0, -1)])
    assert abs(out[0] - 3.0) <= TOL and lab[0] == 1
    out, lab = shoot(cyl, (-1, 0, 0.02), [(1, 0, 0)])
    assert abs(out[0] - 0.8) <= TOL and lab[0] == 2
    out, lab = shoot(cyl, (-0.5, 0, 0.5), [(1, 0, -1)])
    assert abs(out[0] - 0.45 * math.sqrt(2)) <= TOL / s and lab[0] == 2


def test_inside_near_mask_order_and_tie_rules():
    box = one_prim(RB.BOX, (0, 0, 0), ID, (0.3, 0.1, 0.05))
    # a ray that starts inside the box reports what lies behind it: the plane 2 m below the base
    out, lab = shoot(box, (0.1, 0, 0.01), [(0, 0, -1), (0.6, 0, -0.8)])
    np.testing.assert_allclose(out, [2.01, 2.01 / 0.8], atol=TOL / 0.8)
    assert (lab == 1).all()
    # an entry before `near` is ignored: from 0.03 above the top face with near = 0.05
    out, lab = shoot(box, (0, 0, 0.08), [(0, 0, -1)])
    assert abs(out[0] - 2.08) <= TOL and lab[0] == 1
    out, lab = shoot(box, (0, 0, 0.08), [(0, 0, -1)], near=0.02)
    assert abs(out[0] - 0.03) <= TOL and lab[0] == 2
    # a masked body is invisible; the label carries the body index
    on_calf = one_prim(RB.SPHERE, (0, 0, 0), ID, (0.1, 0, 0), body=3)
    th = np.zeros((1, 12), np.float32)
    tabs = RB.robot_dict(on_calf)
    P, _ = RB.fk(tabs, ID.astype(np.float64), np.zeros(12))
    above = (float(P[3][0]), float(P[3][1]), float(P[3][2]) + 1.0)
    out, lab = shoot(on_calf, above, [(0, 0, -1)], th=th)
    assert abs(out[0] - 0.9) <= TOL and lab[0] == 2 + 3
    out, lab = shoot(on_calf, above, [(0, 0, -1)], th=th, mask=0x1FFFF & ~(1 << 3))
    assert abs(out[0] - (2.0 + above[2])) <= 2 * TOL and lab[0] == 1
    # a body in front of the terrain wins, a body behind the terrain does not: base 0.02 m above the plane, box bottom 0.03 below it
    out, lab = shoot(box, (0, 0, 1), [(0, 0, -1)], base=(0, 0, 0.02))
    assert abs(out[0] - 0.95) <= TOL and lab[0] == 2
    out, lab = shoot(box, (0.5, 0, 1), [(0, 0, -1)], base=(0, 0, 0.02))       # straight down beside it
    assert abs(out[0] - 1.02) <= TOL and lab[0] == 1
    # from (0.6, 0, 0.12) through the ground at x = 0.32 into the buried part of the side face x = 0.3 (met at z = -0.0086): the ground wins
    out, lab = shoot(box, (0.6, 0, 0.1), [(-0.28, 0, -0.12)], base=(0, 0, 0.02))
    assert abs(out[0] - math.hypot(0.28, 0.12)) <= TOL * math.hypot(0.28, 0.12) / 0.12 and lab[0] == 1
    # a tie gives the body label: the box's top face in the plane z = 0 exactly (all values exact in fp32)
    out, lab = shoot(one_prim(RB.BOX, (0, 0, 0), ID, (0.25, 0.125, 0.0625)), (0, 0, 1), [(0, 0, -1)], base=(0, 0, -0.0625))
    assert out[0] == np.float32(0.9375) and lab[0] == 2
    # nothing within [near, far]: label 0
    out, lab = shoot(box, (0, 0, 1), [(0, 0, 1)])
    assert out[0] == np.float32(5.0) and lab[0] == 0


# ---- equalities
@pytest.mark.parametrize("case", S.CASES, ids=[c[0] for c in S.CASES])
def test_without_primitives_or_with_an_empty_mask_the_output_is_lsim_raycasts(case):
    sc, rs, mt, dirs, scale = S.case_inputs(case)
    want, _ = EMU.cast(sc, rs, mt, dirs, S.NEAR, S.FAR, scale=scale)
    tabs = BS.tables()[0]
    empty = abi.LsimRaycastRobot.from_buffer_copy(tabs[0])
    empty.num_prims = 0
    th = np.tile(BS.STAND.astype(np.float32), (rs.shape[0], 1))
    for tables, mask in (([empty], 0x1FFFF), ([tabs[0]], 0)):
        out, lab, state, _ = BE.cast(sc, tables, None, rs, th, mt, dirs, S.NEAR, S.FAR, scale=scale, body_mask=mask)
        np.testing.assert_array_equal(out.view(np.int32), want.view(np.int32))
        assert set(lab.reshape(-1).tolist()) <= {0, 1} and state[0] == 0
        far_s = np.float32(S.FAR) * scale[None, :]
        assert ((lab == 1) == (out < far_s)).all()


def test_yaw_frame_on_a_level_base_equals_the_base_frame():
    sc, tabs, rs, th, mt, dirs, scale, _ = BS.case_inputs(BS.CASES[0])
    for e in range(4):
        rs[e, 3:7] = S.quat_rpy(0.0, 0.0, 0.3 + e)
    a, la, _, _ = BE.cast(sc, tabs, BS.ENV_ROBOT, rs, th, mt, dirs, BS.NEAR, BS.FAR, scale=scale, flags=0)
    b, lb, _, _ = BE.cast(sc, tabs, BS.ENV_ROBOT, rs, th, mt, dirs, BS.NEAR, BS.FAR, scale=scale, flags=RB.FRAME_YAW)
    # the yaw frame re-normalises (0, 0, z, w): one more rounding of the quaternion, at most 2^-23 rad -- far inside the envelope's EPS_ANG; on rays
    # that are not at a silhouette the two agree to the reference's tolerance at 5 m
    same = np.abs(a - b) <= REF.ATOL + REF.C_TOL * 2.0 ** -23 * 10.0
    assert same.mean() >= 1 - REF.MAX_UNSTABLE and (la == lb).mean() >= 1 - REF.MAX_UNSTABLE
    rs[:, 3:7] = ID                          # the identity quaternion normalises to itself: bit for bit
    a, la, _, _ = BE.cast(sc, tabs, BS.ENV_ROBOT, rs, th, mt, dirs, BS.NEAR, BS.FAR, scale=scale, flags=0)
    b, lb, _, _ = BE.cast(sc, tabs, BS.ENV_ROBOT, rs, th, mt, dirs, BS.NEAR, BS.FAR, scale=scale, flags=RB.FRAME_YAW)
    np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))
    np.testing.assert_array_equal(la, lb)


def test_forward_kinematics_equal_the_simulators_body_positions():
    """the launch's FK from (root_states, dof_state) against rigid_body_states of the lane emulator of kernels A / B after steps of random
    actions, on the envs that did not reset in the last step, and against the float64 FK of the reference"""
    import torch
    import eval_emu_binding
    from helpers import C
    cfg = C.mixed_cfg("aliengo", {"aliengo": 0.5, "go2": 0.5})[0]
    cfg.env.num_envs = 4
    cfg.terrain.num_rows, cfg.terrain.num_cols = 2, 2
    cfg.terrain.terrain_proportions = [0.0, 0.0, 0.0, 0.0, 0.5, 0.5]
    env = eval_emu_binding.emu_mixed_env(cfg)
    env.reset()
    g = torch.Generator().manual_seed(4)
    for _ in range(3):
        env.step_device(torch.randn(4, 12, generator=g) * 0.5)
    keep = ~env.reset_buf.numpy().astype(bool)
    assert keep.any()
    rs, th = env.root_states.numpy().copy(), env.dof_pos.numpy().copy()
    tabs = BS.tables()[0]
    ids = env.robot_ids.numpy().astype(np.uint8)
    mt = np.tile(np.array([0, 0, 0, 0, 0, 0, 1], np.float32), (4, 1))
    _, _, _, bodies = BE.cast(REF.plane_scene(), tabs, ids, rs, th, mt, np.array([[0, 0, -1]], np.float32), 0.05, 5.0)
    world = bodies[:, :, 0:3].astype(np.float64) + rs[:, None, 0:3]
    want = env.buf["rigid_body_states"].numpy().reshape(4, 17, 13)[:, :, 0:3]
    # two fp32 evaluations of the same chain (rotation matrices in the simulator, quaternions here) at world coordinates of a few metres: the
    # bound the model tests use for the toe positions of one leg chain (tests/test_model.py), 1e-5 m
    err = np.abs(world - want)[keep].max()
    print(f"FK vs rigid_body_states: max {err:.2e} m over {keep.sum()} envs")
    assert err <= 1e-5
    for e in range(4):
        P, Q = RB.fk(RB.robot_dict(tabs[ids[e]]), rs[e, 3:7].astype(np.float64), th[e].astype(np.float64))
        assert np.abs(bodies[e, :, 0:3] - P).max() <= 2e-6
        assert np.abs(np.abs((bodies[e, :, 3:7] * Q).sum(-1)) - 1.0).max() <= 1e-6


# ---- non-finite joints, arguments
def test_nonfinite_joint_state_is_counted_and_gives_far():
    sc, tabs, rs, th, mt, dirs, scale, flags = BS.case_inputs(BS.CASES[0])
    clean, lclean, _, _ = BE.cast(sc, tabs, BS.ENV_ROBOT, rs, th, mt, dirs, BS.NEAR, BS.FAR, scale=scale)
    th[1, 7] = np.nan
    th[3, 0] = np.inf
    rs[2, 4] = np.nan
    out, lab, state, _ = BE.cast(sc, tabs, BS.ENV_ROBOT, rs, th, mt, dirs, BS.NEAR, BS.FAR, scale=scale)
    assert np.isfinite(out).all() and state[0] == 3 * len(dirs)
    np.testing.assert_array_equal(out[1:], np.broadcast_to(np.float32(BS.FAR) * scale, (3, len(dirs))))
    assert (lab[1:] == 0).all()
    np.testing.assert_array_equal(out[0], clean[0])
    np.testing.assert_array_equal(lab[0], lclean[0])


def test_every_invalid_argument_is_refused_and_nothing_is_written():
    sc, tabs, rs, th, mt, dirs, scale, flags = BS.case_inputs(BS.CASES[0])
    L = BE.lib()

    def rv(edit, edit_table=None):
        tt = [abi.LsimRaycastRobot.from_buffer_copy(t) for t in tabs]
        if edit_table:
            edit_table(tt[1])
        rb, keep = BE.fill(sc, tt, BS.ENV_ROBOT, rs, th, mt, dirs, BS.NEAR, BS.FAR, scale=scale, out_fill=-7.0)
        if edit:
            edit(rb)
        r = L.emu_raycast_bodies(ctypes.byref(rb), None)
        if r != 0:
            assert (keep["out"] == -7.0).all() and (keep["labels"] == 255).all() and (keep["state"] == 0).all()
        return r

    assert rv(None) == 0
    assert L.emu_raycast_bodies(None, None) == abi.E_INVALID
    a, b = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.emu_raycast_bodies_sizes(None, ctypes.byref(b)) == abi.E_INVALID and L.emu_raycast_bodies_sizes(ctypes.byref(a), None) == abi.E_INVALID
    assert L.emu_raycast_bodies_sizes(ctypes.byref(a), ctypes.byref(b)) == 0 and b.value == ctypes.sizeof(abi.LsimRaycastRobot)
    assert abi.DEFINES["LSIM_RAYCAST_MAX_PRIMS"] >= 29

    def both(rb, v):
        rb.robots = rb.robots_host = v
    edits = {
        "dof_state NULL": lambda rb: setattr(rb, "dof_state", None), "dof_state misaligned": lambda rb: setattr(rb, "dof_state", rb.dof_state + 2),
        "robots NULL": lambda rb: setattr(rb, "robots", None), "robots_host NULL": lambda rb: setattr(rb, "robots_host", None),
        "robots misaligned": lambda rb: setattr(rb, "robots", rb.robots + 1), "robots_host misaligned": lambda rb: setattr(rb, "robots_host", rb.robots_host + 2),
        "num_robots 0": lambda rb: setattr(rb, "num_robots", 0), "num_robots 5": lambda rb: setattr(rb, "num_robots", abi.DEFINES["LSIM_MAX_ROBOTS"] + 1),
        "two robots without env_robot": lambda rb: setattr(rb, "env_robot", None), "label_stride short": lambda rb: setattr(rb, "label_stride", rb.rc.num_rays - 1),
        "unknown flag": lambda rb: setattr(rb, "flags", 2), "rc: out NULL": lambda rb: setattr(rb.rc, "out", None), "rc: near = far": lambda rb: setattr(rb.rc, "near", rb.rc.far),
        "rc: R 0": lambda rb: setattr(rb.rc, "num_rays", 0),
    }
    for what, edit in edits.items():
        assert rv(edit) == abi.E_INVALID, what
    table_edits = {
        "num_prims -1": lambda t: setattr(t, "num_prims", -1), "num_prims too large": lambda t: setattr(t, "num_prims", abi.DEFINES["LSIM_RAYCAST_MAX_PRIMS"] + 1),
        "body 17": lambda t: setattr(t.prims[2], "body", 17), "body -1": lambda t: setattr(t.prims[0], "body", -1), "kind 4": lambda t: setattr(t.prims[1], "kind", 4),
        "size 0": lambda t: t.prims[0].size.__setitem__(0, 0.0), "size negative": lambda t: t.prims[0].size.__setitem__(1, -0.1),
        "size nan": lambda t: t.prims[0].size.__setitem__(2, math.nan), "size inf": lambda t: t.prims[0].size.__setitem__(0, math.inf),
        "pos nan": lambda t: t.prims[3].pos.__setitem__(1, math.nan), "quat inf": lambda t: t.prims[3].quat.__setitem__(0, math.inf),
        "parent": lambda t: setattr(t.bodies[6], "parent", 1), "dof 12": lambda t: setattr(t.bodies[2], "dof", 12), "joint_pos nan": lambda t: t.bodies[5].joint_pos.__setitem__(0, math.nan),
    }
    assert tabs[1].prims[0].kind == RB.BOX, "the edits of size[1], size[2] need a box first"
    for what, edit in table_edits.items():
        assert rv(None, edit) == abi.E_INVALID, what
    # the unused size entries of a sphere are not looked at; primitives beyond num_prims neither
    def tail(t):
        t.prims[t.num_prims].body = 99
    assert rv(None, tail) == 0


# ---- envs/sensors.py
class _FakeEnv:
    """what RaySensor reads of a LeggedRobot: root_states, dof_state, lcfg, buf["terrain_mesh"], num_envs, robot names / ids, the sensor tables"""

    def __init__(self, sc, rs, th, robot_ids):
        import torch
        self.num_envs = rs.shape[0]
        self.root_states = torch.from_numpy(rs.copy())
        ds = np.zeros((rs.shape[0], 12, 2), np.float32)
        ds[:, :, 0] = th
        self.dof_state = torch.from_numpy(ds).view(-1, 2)
        self.buf = {"terrain_mesh": torch.from_numpy(np.ascontiguousarray(sc["words"]))}
        lc = abi.LsimConfig()
        lc.mesh_type, lc.horizontal_scale, lc.vertical_scale, lc.border_size = sc["mesh_type"], sc["hs"], sc["vs"], sc["border"]
        lc.grid_rows, lc.grid_cols = sc["words"].shape
        self.lcfg = lc
        self._L = None
        self.robot_names, self.robot_ids = ["aliengo", "go2"], torch.as_tensor(robot_ids, dtype=torch.long)
        self.sensor_tables = BS.tables()


def test_sensors_module_defaults_keywords_and_mixed_mounts():
    from isaacgymloco_amd import lib
    from isaacgymloco_amd.envs import sensors
    sc, tabs, rs, th, mt, dirs, scale, flags = BS.case_inputs(BS.CASES[1])
    env = _FakeEnv(sc, rs, th, BS.ENV_ROBOT)
    api = BE.EmuApi()
    # the defaults: lsim_raycast exactly as before, nothing of the new path allocated or called
    plain = sensors.depth_camera(env, S.CAM_W, S.CAM_H, S.CAM_HFOV, mount_pos=BS.MOUNTS, pitch_deg=30.0, near=BS.NEAR, far=BS.FAR, api=api)
    terrain_only = plain.update().clone()
    assert api.calls == {"lsim_raycast": 1, "lsim_raycast_bodies": 0} and plain.bodies_struct is None and plain.label_rows is None
    with pytest.raises(ValueError):
        plain.labels()
    mt0 = plain.mount.numpy()
    want, _ = EMU.cast(sc, rs, mt0, plain.dirs.numpy(), BS.NEAR, BS.FAR, scale=scale)
    np.testing.assert_array_equal(terrain_only.numpy(), want)

    class Old:                                # a library from before the entry point
        lsim_raycast = lsim_raycast_sizes = None
    with pytest.raises(lib.LsimError):
        sensors.depth_camera(env, 4, 3, 87.0, see_robot=True, api=Old())
    with pytest.raises(ValueError):
        sensors.depth_camera(env, 4, 3, 87.0, labels=True, api=api)
    with pytest.raises(ValueError):
        sensors.depth_camera(env, 4, 3, 87.0, frame="world", api=api)
    with pytest.raises(ValueError):
        sensors.depth_camera(env, 4, 3, 87.0, see_robot=True, ignore_bodies=("tail",), api=api)
    # see_robot with labels, per-robot mounts of the mixed instance
    mount = {"aliengo": (-0.1, 0.0, 0.02), "go2": (-0.1, 0.0, 0.02)}
    cam = sensors.depth_camera(env, S.CAM_W, S.CAM_H, S.CAM_HFOV, mount_pos=mount, pitch_deg=35.0, near=BS.NEAR, far=BS.FAR, api=api, see_robot=True, labels=True)
    img = cam.update()
    assert api.calls["lsim_raycast_bodies"] == 1 and api.calls["lsim_raycast"] == 1
    assert cam.label_image().shape == (4, S.CAM_H, S.CAM_W) and cam.label_image().data_ptr() == cam.labels().data_ptr()
    out, lab, _, _ = BE.cast(sc, tabs, BS.ENV_ROBOT, rs, th, cam.mount.numpy(), cam.dirs.numpy(), BS.NEAR, BS.FAR, scale=scale)
    np.testing.assert_array_equal(img.numpy(), out)
    np.testing.assert_array_equal(cam.labels().numpy(), lab)
    assert (lab >= 2).mean() > 0.05 and int(cam.nonfinite_rays) == 0
    assert cam.body_names[0] == "base" and len(cam.body_names) == 17
    # ignore_bodies by name (a substring selects every body that carries it) and by index
    hidden = sensors.depth_camera(env, S.CAM_W, S.CAM_H, S.CAM_HFOV, mount_pos=mount, pitch_deg=35.0, near=BS.NEAR, far=BS.FAR, api=api, see_robot=True, labels=True,
                                  ignore_bodies=("FL_thigh", "calf", 0))
    want_mask = 0x1FFFF & ~(1 << 2) & ~sum(1 << b for b in (3, 7, 11, 15)) & ~1
    assert hidden.body_mask == want_mask
    hidden.update()
    out, lab, _, _ = BE.cast(sc, tabs, BS.ENV_ROBOT, rs, th, cam.mount.numpy(), cam.dirs.numpy(), BS.NEAR, BS.FAR, scale=scale, body_mask=want_mask)
    np.testing.assert_array_equal(hidden.out.numpy(), out)
    assert not np.isin(hidden.labels().numpy(), [2, 4, 5, 9, 13, 17]).any() and (hidden.labels().numpy() >= 2).any()
    # frame="yaw" lidar
    li = sensors.lidar(env, 4, 20.0, 30, mount_pos=(0.0, 0.0, 0.3), far=4.0, api=api, see_robot=True, frame="yaw")
    rng = li.update().numpy()
    out, _, _, _ = BE.cast(sc, tabs, BS.ENV_ROBOT, rs, th, li.mount.numpy(), li.dirs.numpy(), 0.05, 4.0, flags=RB.FRAME_YAW)
    np.testing.assert_array_equal(rng, out)
