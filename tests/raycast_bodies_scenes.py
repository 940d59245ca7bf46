"""TEST INFRASTRUCTURE -- the robots, poses, sensors and scenes shared by tests/test_raycast_bodies.py (CPU shim) and
tests/test_gpu_raycast_bodies.py (HIP launch).  Four envs per scene: Aliengo standing and mid-stride, Go2 standing and mid-stride (joint angles
from a fixed seed), the base at the height at which the lowest foot sphere sinks 2 mm into the ground under the base (so that feet and ground
meet in a curve), level / pitched / rolled."""
import numpy as np

import raycast_bodies_reference as RB
import raycast_reference as REF
import raycast_scenes as S
from helpers import C

NEAR, FAR = 0.05, 5.0
STAND = np.array([0.0, 0.8, -1.5] * 4)
MOUNTS = {"aliengo": (0.30, 0.0, 0.05), "go2": (0.25, 0.0, 0.03)}       # the README's camera: inside the Aliengo trunk box (envs 0 and 2)
ENV_ROBOT = np.array([0, 0, 1, 1], np.uint8)
_cache = {}


def tables(capsule=True):
    """([lsim_raycast_robot of Aliengo, of Go2], body names)"""
    if capsule not in _cache:
        from isaacgymloco_amd.robots import model
        cfg = C.mixed_cfg("aliengo", {"aliengo": 0.5, "go2": 0.5})[0]
        out = []
        for k in range(2):
            asset = C.robot_cfg(cfg, k).asset
            asset.replace_cylinder_with_capsule = capsule
            out.append(model.build_sensor_table(asset))
        _cache[capsule] = ([t for t, _ in out], out[0][1])
    return _cache[capsule]


def joint_angles():
    g = np.random.RandomState(11)
    th = np.stack([STAND, STAND + g.uniform(-0.35, 0.35, 12), STAND, STAND + g.uniform(-0.35, 0.35, 12)])
    return th.astype(np.float32)


def robot_poses(ground_z, centre=(0.0, 0.0)):
    """(root_states [4, 13], dof_pos [4, 12]): ground_z(x, y) -> height of the ground there"""
    tabs, _ = tables()
    th = joint_angles()
    rs = np.zeros((4, 13), np.float32)
    cx, cy = centre
    xy = [(cx - 1.0, cy + 0.03), (cx - 0.8, cy - 0.21), (cx + 0.9, cy + 0.4), (cx - 0.3, cy + 1.1)]
    rpy = [(0.0, 0.0, 0.2), (0.08, 0.15, -0.4), (0.0, 0.0, 2.6), (0.2, -0.1, 1.0)]
    for e in range(4):
        q = np.array(S.quat_rpy(*rpy[e]), np.float32).astype(np.float64)
        rob = RB.robot_dict(tabs[ENV_ROBOT[e]])
        P, _ = RB.fk(rob, q, th[e].astype(np.float64))
        feet = [p for p in rob["prims"] if p["kind"] == RB.SPHERE and p["body"] in (4, 8, 12, 16)]
        low = min(P[p["body"]][2] - p["size"][0] for p in feet)
        rs[e, :7] = [xy[e][0], xy[e][1], ground_z(*xy[e]) - low - 0.002] + list(q)
    return rs, th


def camera(frame="base"):
    """(mount [4, 7], dirs, scale, flags): the README camera per robot, or the chase camera of frame="yaw" (behind and above, looking down at the robot)"""
    from isaacgymloco_amd.envs.sensors import pinhole_dirs, quat_from_pitch
    dirs, scale = pinhole_dirs(S.CAM_W, S.CAM_H, S.CAM_HFOV)
    mt = np.zeros((4, 7), np.float32)
    if frame == "yaw":
        mt[:] = [-1.2, 0.0, 0.7] + list(quat_from_pitch(28.0))
        return mt, dirs, scale, RB.FRAME_YAW
    for e in range(4):
        mt[e] = list(MOUNTS["aliengo" if ENV_ROBOT[e] == 0 else "go2"]) + list(quat_from_pitch(30.0))
    for e in (1, 3):          # a second camera further back in the trunk, pitched 35 degrees: the front hips, thighs and calves cross its image
        mt[e] = [-0.1, 0.0, 0.02] + list(quat_from_pitch(35.0))
    return mt, dirs, scale, 0


def lidar():
    from isaacgymloco_amd.envs.sensors import ring_dirs
    mt = np.zeros((4, 7), np.float32)
    mt[:] = [0.1, 0.0, 0.10, 0, 0, 0, 1]
    return mt, ring_dirs(16, 30.0, 360), None, 0


def ground(name, border=S.BORDER):
    """(scene dict, ground_z(x, y)) of a scene name of tests/raycast_scenes.py"""
    if name == "plane":
        return REF.plane_scene(), lambda x, y: 0.0
    sc = S.scene(name, 2, border)
    hf = S.height_grid(name).astype(np.float64) * S.VS

    def z(x, y):
        i, j = int(round((x + border) / S.HS)), int(round((y + border) / S.HS))
        return float(hf[max(i - 4, 0):i + 5, max(j - 4, 0):j + 5].max())          # the highest ground under the robot: feet never start below the surface
    return sc, z


# (label, ground, border, sensor, capsule)
CASES = [("plane-camera", "plane", S.BORDER, "camera", True), ("stairs_up-camera", "stairs_up", S.BORDER, "camera", True),
         ("ramp-190m-camera", "ramp", -185.0, "camera", True), ("plane-lidar-16x360", "plane", S.BORDER, "lidar", True),
         ("stairs_up-chase-yaw", "stairs_up", S.BORDER, "chase", True), ("plane-camera-flat-cylinders", "plane", S.BORDER, "camera", False)]


def case_inputs(case):
    """(scene, tables, root_states, dof_pos, mount, dirs, scale, flags)"""
    label, name, border, sensor, capsule = case
    sc, gz = ground(name, border)
    centre = (0.0, 0.0) if border == S.BORDER else (-border + 3.2, -border + 3.2)
    rs, th = robot_poses(gz, centre)
    mt, dirs, scale, flags = lidar() if sensor == "lidar" else camera("yaw" if sensor == "chase" else "base")
    return sc, tables(capsule)[0], rs, th, mt, dirs, scale, flags
