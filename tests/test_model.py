"""Robot model table: derived constants (mass after Isaac Gym's fixed-joint collapse) and, when the reference
checkout is present (build container only), a re-derivation from its URDF."""
import os

import numpy as np
import pytest

from helpers import aliengo

URDF = "/root/reference/legged_gym/resources/robots/aliengo/urdf/aliengo.urdf"


def test_masses_and_topology():
    m = aliengo.build_model()
    masses = [b.mass for b in m.bodies]
    assert abs(sum(masses) - 24.937) < 1e-3                      # 24.94 kg
    assert abs(masses[0] - 12.229) < 1e-3 and abs(masses[1] - 2.139) < 1e-3 and abs(masses[2] - 0.771) < 1e-3
    assert [m.bodies[i].parent for i in range(17)] == [-1, 0, 1, 2, 3, 0, 5, 6, 7, 0, 9, 10, 11, 0, 13, 14, 15]
    assert [m.bodies[i].dof for i in range(17)] == [-1, 0, 1, 2, -1, 3, 4, 5, -1, 6, 7, 8, -1, 9, 10, 11, -1]
    assert list(m.feet_bodies) == [4, 8, 12, 16]
    assert m.termination_body_mask == 1 and bin(m.penalised_body_mask).count("1") == 9
    assert m.num_collision_points == 64       # every URDF collision primitive incl. the rotor housings (robots/common.py rules)


def test_table_matches_reference_urdf():
    """the hand table against the values of the reference's aliengo.urdf (tests/golden/urdf_aliengo_values.json, tools/gen_golden_urdf.py)"""
    import json
    ref = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "urdf_aliengo_values.json")))
    bodies = aliengo.body_table()
    for leg in aliengo.LEGS:
        r = ref["legs"][leg]
        b = bodies[aliengo.BODY_NAMES.index(f"{leg}_hip")]
        assert abs(b["mass"] - (r["hip_mass"] + r["thigh_rotor_mass"])) < 1e-9
        np.testing.assert_allclose(b["joint_pos"], r["hip_joint_origin"], atol=1e-12)
        assert r["calf_limit_lower"] == aliengo.LIMITS["calf"][0] and r["calf_limit_effort"] == aliengo.LIMITS["calf"][3]
        c = bodies[aliengo.BODY_NAMES.index(f"{leg}_calf")]
        np.testing.assert_allclose(c["com"], r["calf_com"], atol=1e-12)
        # thigh inertia products mirror with the leg side
        assert np.sign(r["thigh_ixy"]) == np.sign(aliengo._mirror(aliengo.THIGH, 1.0, aliengo._SY[leg])["inertia"][1])
    assert abs(bodies[0]["mass"] - (ref["trunk_mass"] + 0.001 + 4 * 0.146)) < 1e-9


def test_stored_tables_build_and_aliengo_table_equals_hand_table():
    """robots/tables/*.json (written by tools/gen_robot_tables.py through the URDF loader) build valid models; the Aliengo one is
    byte-identical to the hand-checked table of robots/aliengo.py"""
    from isaacgymloco_amd.robots import urdf
    m, names, dofs = urdf.build_model_from_table("aliengo")
    assert bytes(m) == bytes(aliengo.build_model())
    assert dofs == aliengo.DOF_NAMES and names == aliengo.BODY_NAMES
    for robot, mass in (("go1", 11.31), ("a1", 12.454)):
        g, gn, gd = urdf.build_model_from_table(robot)
        assert abs(sum(g.bodies[i].mass for i in range(17)) - mass) < 5e-3
        assert gd == aliengo.DOF_NAMES and list(g.feet_bodies) == [4, 8, 12, 16]
        assert 40 <= g.num_collision_points <= 64 and g.termination_body_mask == 1
        assert all(g.dof_pos_lower[j] < g.dof_pos_upper[j] for j in range(12))


@pytest.mark.skipif(not os.path.exists(URDF), reason="reference checkout not present")
def test_urdf_loader_reproduces_tables():
    """the generic loader (fixed-joint collapse, Isaac ordering, collision rules) on the reference's URDFs == the shipped tables"""
    import json
    from isaacgymloco_amd.robots import urdf
    m, _, _ = urdf.build_model(URDF)
    assert bytes(m) == bytes(aliengo.build_model())
    for robot in ("go1", "a1"):
        a, _, _ = urdf.build_model(URDF.replace("aliengo", robot))
        b, _, _ = urdf.build_model_from_table(robot)
        assert bytes(a) == bytes(b)


def _fk_toe_error(cfg, joint_pos, toe_pos_base):
    """largest |toe position by the build's forward kinematics - toe position stored in the reference's mocap frame| (m)"""
    import ctypes
    from helpers import make_oracle
    N = 64
    orc, lc, model, ter = make_oracle(cfg, N, seed=1)
    L = orc._L
    L.orc_refresh_body_states.argtypes = [ctypes.c_void_p, ctypes.c_int]
    feet = list(model.feet_bodies)
    worst = 0.0
    for i0 in range(0, len(joint_pos), N):
        n = len(joint_pos[i0:i0 + N])
        root = np.zeros((N, 13), np.float32); root[:, 6] = 1.0            # base frame = world frame
        orc.buf["root_states"][...] = root
        dof = np.zeros((N, 12, 2), np.float32); dof[:n, :, 0] = joint_pos[i0:i0 + n]
        orc.buf["dof_state"][...] = dof
        for e in range(n):
            L.orc_refresh_body_states(orc._h, e)
        got = orc.buf["rigid_body_states"][:n][:, feet, 0:3]
        worst = max(worst, float(np.abs(got - toe_pos_base[i0:i0 + n].reshape(n, 4, 3)).max()))
    orc.close()
    return worst


def test_leg_kinematics_reproduce_the_reference_mocap_toe_positions():
    """P1 pinned to reference DATA: every frame of the reference's Aliengo mocap clips (datasets/mocap_motions_aliengo/*.txt, re-packed
    unchanged in isaacgymloco_amd/data/mocap_aliengo.npz: the 7 clips AGA:34-36 selects) stores the 12 joint angles AND the toe positions in the
    base frame that the reference's retargeting tool computed from ITS kinematic model of the URDF (columns 7:19 and 19:31 of the 61,
    motion_loader.py:26-48).  The forward kinematics of the build -- the model table (joint origins, axes, foot offsets) through the oracle's
    body-state refresh, which the HIP kernels are compared with elsewhere -- must land on them: 658 frames x 4 feet, measured 7e-6 m.
    (Leg slots of the files are FL, FR, RL, RR by the sign of the toes' y, i.e. already Isaac Gym's order.)"""
    from helpers import quiet_cfg
    data = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "isaacgymloco_amd", "data", "mocap_aliengo.npz"), allow_pickle=True)
    frames = np.concatenate([data[f"frames_{c}"] for c in range(int(data["num_clips"]))])
    assert frames.shape[1] == 61 and len(frames) > 600
    want = frames[:, 19:31].reshape(-1, 4, 3)
    assert np.all(np.sign(want[:, [0, 2], 1]) > 0) and np.all(np.sign(want[:, [1, 3], 1]) < 0)     # slots 0 / 2 are left legs
    worst = _fk_toe_error(quiet_cfg("aliengo"), frames[:, 7:19], frames[:, 19:31])
    assert worst < 3e-5, worst


def test_a1_table_kinematics_reproduce_the_reference_a1_mocap_toe_positions():
    """the same pin for a second model table (robots/tables/a1.json, from the reference's a1.urdf through the generic loader): every 4th frame
    of the reference's 13 A1 clips (datasets/mocap_motions_a1, tests/golden/mocap_a1_frames.npz by tools/pack_mocap_fixture.py; 323 frames;
    all 1274: the same 7e-6 m).  Catches a wrong hip / thigh / calf origin, axis or foot offset of the table."""
    from helpers import quiet_cfg
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mocap_a1_frames.npz"))
    assert fx["joint_pos"].shape == (323, 12) and len(set(fx["clip"].tolist())) == 13
    cfg = quiet_cfg("go1")
    cfg.asset.name = "a1"
    worst = _fk_toe_error(cfg, fx["joint_pos"], fx["toe_pos_base"])
    assert worst < 3e-5, worst
    cfg.asset.name = "go1"      # negative control: Go1's table (8 mm shorter thighs, different hip offsets) does not fit A1's data
    assert _fk_toe_error(cfg, fx["joint_pos"][:64], fx["toe_pos_base"][:64]) > 3e-3


def test_go2_table_kinematics_reproduce_the_reference_go2_mocap_toe_positions():
    """BASELINE config 5's second robot: robots/tables/go2.json -- kinematics FITTED to the reference's Go2 clips (tools/gen_go2_table.py; the
    reference has no Go2 URDF) -- against every 4th frame of the 13 clips (datasets/mocap_motions_go2, tests/golden/mocap_go2_frames.npz):
    the forward kinematics of the table through the oracle lands on the stored toe positions to the text's rounding.  Go1's table (hips
    5 mm further in, 15 mm shorter thigh offset) misses by > 3 mm: the data tells the two robots apart."""
    from helpers import quiet_cfg
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mocap_go2_frames.npz"))
    assert fx["joint_pos"].shape == (323, 12) and len(set(fx["clip"].tolist())) == 13
    worst = _fk_toe_error(quiet_cfg("go2"), fx["joint_pos"], fx["toe_pos_base"])
    assert worst < 3e-5, worst
    assert _fk_toe_error(quiet_cfg("go1"), fx["joint_pos"][:64], fx["toe_pos_base"][:64]) > 3e-3


def test_go2_table_states_its_provenance_and_is_a_plausible_robot():
    import json
    from isaacgymloco_amd.robots import urdf
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "isaacgymloco_amd", "robots", "tables", "go2.json")
    d = json.load(open(path))
    assert "fitted" in d["provenance"]["kinematics"] and "NOMINAL" in d["provenance"]["inertial_limits_collision"]
    m, names, dofs = urdf.build_model_from_table("go2")
    assert dofs == aliengo.DOF_NAMES and list(m.feet_bodies) == [4, 8, 12, 16]
    assert abs(sum(m.bodies[i].mass for i in range(17)) - 15.017) < 1e-3
    assert 40 <= m.num_collision_points <= 64 and m.termination_body_mask == 1
    for i in range(17):      # every inertia tensor positive definite
        I = m.bodies[i].inertia
        assert np.all(np.linalg.eigvalsh(np.array([[I[0], I[1], I[2]], [I[1], I[3], I[4]], [I[2], I[4], I[5]]])) > 0)
