"""CPU: the range-sensor kernel source (isaacgymloco_amd/csrc/ls_raycast.h) compiled by g++ under LS_EMU, against the float64 brute force of
tests/raycast_reference.py (whose docstring states the acceptance rule and derives its constants), against closed forms, and through
envs/sensors.py.  The same scenes run on the HIP launch in tests/test_gpu_raycast.py."""
import ctypes
import math

import numpy as np
import pytest

import raycast_emu_binding as EMU
import raycast_reference as REF
import raycast_scenes as S
from helpers import abi


@pytest.mark.parametrize("case", S.CASES, ids=[c[0] for c in S.CASES])
def test_emulated_launch_matches_the_brute_force(case):
    sc, rs, mt, dirs, scale = S.case_inputs(case)
    got, state = EMU.cast(sc, rs, mt, dirs, S.NEAR, S.FAR, scale=scale)
    assert state[0] == 0
    REF.check(sc, rs, mt, dirs, S.NEAR, S.FAR, got, scale=scale, label=case[0])


def test_slow_path_words_give_the_packed_grid_results():
    """dz = 255 everywhere / bit 20 everywhere only disable shortcuts: the same depths as the properly packed words (to the tolerance of a
    ray-plane intersection at 5 m, since a wider neighbourhood may meet the same surface through another triangle of it)"""
    for name in ("stairs_up", "obstacles"):
        sc, rs, mt, dirs, scale = S.case_inputs((name, name, 2, None, S.BORDER))
        base, _ = EMU.cast(sc, rs, mt, dirs, S.NEAR, S.FAR)
        flags = (sc["words"].view(np.uint32) >> 20) & 1
        assert 0 < flags.mean() < 1, "the packed grid must have both kinds of cells"
        for slow in ("dz", "bit20"):
            alt, _ = EMU.cast(S.scene(name, 2, S.BORDER, slow), rs, mt, dirs, S.NEAR, S.FAR)
            stable = np.abs(alt - base) <= 1e-4
            assert stable.mean() >= 1 - REF.MAX_UNSTABLE, (name, slow, stable.mean())


# ---- closed forms
def _closed_tol(coord, t, ndot):
    return REF.ATOL + REF.C_TOL * 2.0 ** -23 * (coord + t) / ndot


def test_plane_flat_and_ramp_closed_form():
    dirs, _ = S.ray_table()
    for name, z_of in (("plane", lambda x: 0.0 * x), ("flat", lambda x: 0.2 + 0.0 * x), ("ramp", lambda x: 0.1 * (x + S.BORDER))):
        sc = S.scene(name, 0 if name == "plane" else 2)
        rs, mt = S.poses(S.origin_height(name))
        got, _ = EMU.cast(sc, rs, mt, dirs, S.NEAR, S.FAR)
        o, d = REF.rays(rs, mt, dirs)
        slope = 0.1 if name == "ramp" else 0.0
        n = np.array([-slope, 0.0, 1.0]) / math.hypot(slope, 1.0)
        z0 = z_of(np.zeros(1))[0]                         # plane through (0, 0, z0) with normal n (ramp: z = 0.1 x + 0.32)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((np.array([0.0, 0.0, z0]) - o) @ n) / (d @ n)
            hit = o + t[..., None] * d
        inside = (hit[..., 0] >= -S.BORDER) & (hit[..., 0] <= -S.BORDER + 6.3) & (hit[..., 1] >= -S.BORDER) & (hit[..., 1] <= -S.BORDER + 6.3)
        ok = np.isfinite(t) & (t >= S.NEAR) & (t <= S.FAR) & (inside if name != "plane" else True)
        edge = np.minimum(np.abs(hit[..., :2] + S.BORDER), np.abs(hit[..., :2] + S.BORDER - 6.3)).min(-1) < 1e-3 if name != "plane" else np.zeros_like(ok)
        want = np.where(ok, t, S.FAR)
        tol = _closed_tol(np.abs(o).max(-1) + S.FAR, S.FAR, np.maximum(np.abs(d @ n), 1e-12))
        sel = ~edge & ~(np.abs(t - S.FAR) < 1e-4) & ~(np.abs(t - S.NEAR) < 1e-4)
        assert sel.mean() > 0.95 and ok[sel].mean() > 0.5, name
        assert (np.abs(got - want)[sel] <= np.where(ok, tol, REF.ATOL)[sel]).all(), (name, np.abs(got - want)[sel].max())


@pytest.mark.parametrize("name,wall_x,look", [("step_up", 32 * S.HS - S.BORDER, 1.0), ("step_down", 31 * S.HS - S.BORDER, -1.0)])
def test_riser_is_a_vertical_wall_at_the_displaced_x(name, wall_x, look):
    """one 0.3 m step: slope 3 > slope_threshold, so the LOWER vertex row moves one cell towards the higher one and the riser is the vertical
    plane x = wall_x; horizontal and slightly tilted rays from the low side must meet it there (from -x for step_up, from +x for step_down)"""
    sc = S.scene(name)
    P = REF.vertices(sc)
    np.testing.assert_allclose(P[31 if look > 0 else 32, :, 0], wall_x, atol=1e-12)
    rs = np.zeros((1, 13), np.float32)
    rs[0, :7] = [wall_x - look * 1.25, 0.07, 0.15, 0, 0, 0, 1]
    mt = np.array([[0, 0, 0, 0, 0, 0, 1]], np.float32)
    ang = np.radians(np.array([[0, 0], [10, 3], [-20, -5], [35, 4], [-35, 2]], np.float64))       # yaw, pitch: all meet the riser between z = 0 and 0.3
    d = np.stack((look * np.cos(ang[:, 0]) * np.cos(ang[:, 1]), np.sin(ang[:, 0]) * np.cos(ang[:, 1]), np.sin(ang[:, 1])), axis=1)
    got, _ = EMU.cast(sc, rs, mt, d.astype(np.float32), S.NEAR, S.FAR)
    o, dd = REF.rays(rs, mt, d.astype(np.float32))
    t = (wall_x - o[0, :, 0]) / dd[0, :, 0]
    z = o[0, :, 2] + t * dd[0, :, 2]
    assert ((z > 0.01) & (z < 0.29)).all()
    tol = _closed_tol(np.abs(o).max() + t, t, np.abs(dd[0, :, 0]))
    assert (np.abs(got[0] - t) <= tol).all(), (got[0], t)


def test_pit_and_pillar_closed_form():
    dirs = np.array([[0, 0, -1]], np.float32)
    mt = np.array([[0, 0, 0, 0, 0, 0, 1]] * 3, np.float32)
    rs = np.zeros((3, 13), np.float32)
    rs[:, 6] = 1
    # pit: bottom vertices 24..39 at -0.5 m; its floor between the displaced walls
    rs[:, :3] = [[0.0, 0.0, 0.4], [-1.5, -1.5, 0.4], [0.33, -0.21, 0.9]]
    got, _ = EMU.cast(S.scene("pit"), rs, mt, dirs, S.NEAR, S.FAR)
    np.testing.assert_allclose(got[:, 0], [0.9, 0.4, 1.4], atol=REF.ATOL + REF.C_TOL * 2.0 ** -23 * 5)
    # pillar: cell (32, 32) raised to 0.5 m, x, y in [0, 0.1]
    rs[:, :3] = [[0.05, 0.05, 0.9], [0.03, 0.08, 0.9], [0.5, 0.5, 0.9]]
    got, _ = EMU.cast(S.scene("pillar"), rs, mt, dirs, S.NEAR, S.FAR)
    np.testing.assert_allclose(got[:, 0], [0.4, 0.4, 0.9], atol=REF.ATOL + REF.C_TOL * 2.0 ** -23 * 5)


# ---- scale, env_stride, miss, non-finite
def test_scale_env_stride_and_miss():
    sc, rs, mt, dirs, scale = S.case_inputs(("stairs_up", "stairs_up", 2, None, S.BORDER))
    plain, _ = EMU.cast(sc, rs, mt, dirs, S.NEAR, S.FAR)
    scaled, _ = EMU.cast(sc, rs, mt, dirs, S.NEAR, S.FAR, scale=scale)
    np.testing.assert_array_equal(scaled, plain * scale[None, :])
    up = len(dirs) - 16 + 1                       # the vertical ray upwards: a miss
    assert (plain[:, up] == np.float32(S.FAR)).all() and (scaled[:, 0] <= np.float32(S.FAR) * scale[0]).all()
    strided, _ = EMU.cast(sc, rs, mt, dirs, S.NEAR, S.FAR, env_stride=2)
    np.testing.assert_array_equal(strided[0::2], plain[0::2])
    assert np.isnan(strided[1::2]).all(), "rows of the envs in between are not touched"
    short, _ = EMU.cast(sc, rs, mt, dirs, S.NEAR, 0.2)
    assert (short == np.float32(0.2)).all(), "nothing within 0.2 m of origins 0.4 m above the highest vertex"


def test_nonfinite_pose_is_counted_and_clean():
    sc, rs, mt, dirs, scale = S.case_inputs(("flat", "flat", 2, None, S.BORDER))
    rs[1, 0] = np.nan
    rs[2, 5] = np.inf
    mt[3, 2] = -np.inf
    got, state = EMU.cast(sc, rs, mt, dirs, S.NEAR, S.FAR, scale=scale)
    assert np.isfinite(got).all()
    np.testing.assert_array_equal(got[1:4], np.broadcast_to(np.float32(S.FAR) * scale, (3, len(dirs))))
    assert state[0] == 3 * len(dirs)
    clean, state0 = EMU.cast(sc, *S.case_inputs(("flat", "flat", 2, None, S.BORDER))[1:4], S.NEAR, S.FAR, scale=scale)
    np.testing.assert_array_equal(got[[0, 4]], clean[[0, 4]])
    assert state0[0] == 0


def test_every_invalid_argument_is_refused():
    sc, rs, mt, dirs, scale = S.case_inputs(("flat", "flat", 2, None, S.BORDER))
    L = EMU.lib()

    def rv(edit):
        rc, keep = EMU.fill(sc, rs, mt, dirs, S.NEAR, S.FAR, scale=scale)
        edit(rc)
        return L.emu_raycast(ctypes.byref(rc), None)

    assert rv(lambda rc: None) == 0
    assert L.emu_raycast(None, None) == abi.E_INVALID
    assert L.emu_raycast_sizes(None) == abi.E_INVALID
    nbytes = ctypes.c_size_t()
    assert L.emu_raycast_sizes(ctypes.byref(nbytes)) == 0 and nbytes.value == 8 * abi.DEFINES["LSIM_RAYCAST_STATE_WORDS"]
    edits = {
        "root_states NULL": lambda rc: setattr(rc, "root_states", None), "mount NULL": lambda rc: setattr(rc, "mount", None),
        "dirs NULL": lambda rc: setattr(rc, "dirs", None), "out NULL": lambda rc: setattr(rc, "out", None),
        "state NULL": lambda rc: setattr(rc, "state", None), "mesh NULL": lambda rc: setattr(rc, "mesh", None),
        "root_states misaligned": lambda rc: setattr(rc, "root_states", rc.root_states + 2), "dirs misaligned": lambda rc: setattr(rc, "dirs", rc.dirs + 1),
        "mount misaligned": lambda rc: setattr(rc, "mount", rc.mount + 2), "scale misaligned": lambda rc: setattr(rc, "scale", rc.scale + 2),
        "mesh misaligned": lambda rc: setattr(rc, "mesh", rc.mesh + 2), "out misaligned": lambda rc: setattr(rc, "out", rc.out + 4),
        "state misaligned": lambda rc: setattr(rc, "state", rc.state + 4),
        "N 0": lambda rc: setattr(rc, "num_envs", 0), "R 0": lambda rc: setattr(rc, "num_rays", 0),
        "R too large": lambda rc: (setattr(rc, "num_rays", abi.DEFINES["LSIM_RAYCAST_MAX_RAYS"] + 1), setattr(rc, "out_stride", abi.DEFINES["LSIM_RAYCAST_MAX_RAYS"] + 4)),
        "env_stride 0": lambda rc: setattr(rc, "env_stride", 0), "out_stride short": lambda rc: setattr(rc, "out_stride", rc.num_rays - 4),
        "out_stride odd": lambda rc: setattr(rc, "out_stride", rc.num_rays + 1), "mesh_type 3": lambda rc: setattr(rc, "mesh_type", 3),
        "mesh_type -1": lambda rc: setattr(rc, "mesh_type", -1), "rows 1": lambda rc: setattr(rc, "grid_rows", 1), "cols 1": lambda rc: setattr(rc, "grid_cols", 1),
        "hs 0": lambda rc: setattr(rc, "horizontal_scale", 0.0), "hs nan": lambda rc: setattr(rc, "horizontal_scale", math.nan),
        "vs 0": lambda rc: setattr(rc, "vertical_scale", 0.0), "border inf": lambda rc: setattr(rc, "border_size", math.inf),
        "near < 0": lambda rc: setattr(rc, "near", -0.1), "near = far": lambda rc: setattr(rc, "near", rc.far), "near nan": lambda rc: setattr(rc, "near", math.nan),
        "far inf": lambda rc: setattr(rc, "far", math.inf), "far nan": lambda rc: setattr(rc, "far", math.nan),
    }
    for what, edit in edits.items():
        assert rv(edit) == abi.E_INVALID, what
    assert abi.DEFINES["LSIM_RAYCAST_MAX_RAYS"] >= 64 * 48
    # a plane needs no mesh and no grid
    rc, keep = EMU.fill(REF.plane_scene(), rs, mt, dirs, S.NEAR, S.FAR)
    assert L.emu_raycast(ctypes.byref(rc), None) == 0


# ---- envs/sensors.py
def test_direction_tables():
    from isaacgymloco_amd.envs import sensors
    for w, h, fov in ((64, 48, 87.0), (5, 3, 60.0), (24, 18, 110.0)):
        d, sc = sensors.pinhole_dirs(w, h, fov)
        assert d.shape == (w * h, 3) and sc.shape == (w * h,) and d.dtype == np.float32
        np.testing.assert_allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1.0, atol=2e-7)
        np.testing.assert_allclose(sc, d[:, 0], atol=1e-7)                   # z-depth = range * cos to the optical axis (+x)
        img = d.reshape(h, w, 3).astype(np.float64)
        if w % 2 and h % 2:
            np.testing.assert_allclose(img[h // 2, w // 2], [1, 0, 0], atol=1e-7)
        np.testing.assert_allclose(img[:, ::-1, 1], -img[:, :, 1], atol=1e-7)     # symmetric about the axis; left column looks to +y, top row to +z
        np.testing.assert_allclose(img[::-1, :, 2], -img[:, :, 2], atol=1e-7)
        assert img[0, 0, 1] > 0 and img[0, 0, 2] > 0
        # pixel centres: the outer EDGES of the image span the field of view, so the outermost centres are at tan = (1 - 1/w) tan(fov / 2)
        mid = img[h // 2] if h % 2 else 0.5 * (img[h // 2 - 1] + img[h // 2])
        np.testing.assert_allclose(mid[0, 1] / mid[0, 0], (1 - 1 / w) * math.tan(math.radians(fov) / 2), rtol=1e-6)
        np.testing.assert_allclose(img[0, 0, 2] / img[0, 0, 0], (1 - 1 / h) * math.tan(math.radians(fov) / 2) * h / w, rtol=1e-6)
    d = sensors.ring_dirs(16, 30.0, 360).astype(np.float64).reshape(16, 360, 3)
    np.testing.assert_allclose(np.linalg.norm(d, axis=2), 1.0, atol=2e-7)
    np.testing.assert_allclose(np.degrees(np.arcsin(d[:, 0, 2])), np.linspace(-15, 15, 16), atol=1e-5)
    np.testing.assert_allclose(np.degrees(np.arctan2(d[3, :, 1], d[3, :, 0])) % 360, np.arange(360), atol=1e-4)
    np.testing.assert_allclose(sensors.ring_dirs(1, (-10.0, 0.0), 4)[0], [math.cos(math.radians(5)), 0, -math.sin(math.radians(5))], atol=1e-7)
    q = sensors.quat_from_pitch(30.0)
    np.testing.assert_allclose(REF.quat_rotate(np.array(q), np.array([1.0, 0, 0])), [math.cos(math.radians(30)), 0, -math.sin(math.radians(30))], atol=1e-12)


class _FakeEnv:
    """what RaySensor reads of a LeggedRobot: root_states, lcfg, buf["terrain_mesh"], num_envs, robot names / ids"""

    def __init__(self, sc, rs, robot_ids=None):
        import torch
        self.num_envs = rs.shape[0]
        self.root_states = torch.from_numpy(rs.copy())
        self.buf = {"terrain_mesh": torch.from_numpy(np.ascontiguousarray(sc["words"]))}
        lc = abi.LsimConfig()
        lc.mesh_type, lc.horizontal_scale, lc.vertical_scale, lc.border_size = sc["mesh_type"], sc["hs"], sc["vs"], sc["border"]
        lc.grid_rows, lc.grid_cols = sc["words"].shape
        self.lcfg = lc
        self._L = None
        if robot_ids is not None:
            self.robot_names, self.robot_ids = ["aliengo", "go2"], torch.as_tensor(robot_ids, dtype=torch.long)


def test_ray_sensor_over_the_emulated_entry():
    from isaacgymloco_amd.envs import sensors
    from isaacgymloco_amd import lib
    sc, rs, mt, dirs, scale = S.case_inputs(("stairs_up", "stairs_up", 2, None, S.BORDER))
    env = _FakeEnv(sc, rs, robot_ids=[0, 1, 0, 1, 1])
    with pytest.raises(lib.LsimError):
        sensors.RaySensor(env, dirs, api=object())              # no lsim_raycast: an error, not a fall-back
    # per-env mounts
    s = sensors.RaySensor(env, dirs, mt[:, :3], mt[:, 3:], S.NEAR, S.FAR, scale=scale, api=EMU.EmuApi())
    assert (s.out.numpy() == np.float32(S.FAR) * scale).all(), "before the first update: the miss value"
    out = s.update()
    want, _ = EMU.cast(sc, rs, mt, dirs, S.NEAR, S.FAR, scale=scale)
    np.testing.assert_array_equal(out.numpy(), want)
    assert int(s.nonfinite_rays) == 0
    # one pose for all, and one per robot name
    cam = sensors.depth_camera(env, S.CAM_W, S.CAM_H, S.CAM_HFOV, mount_pos={"aliengo": (0.3, 0.0, 0.05), "go2": (0.25, 0.0, 0.03)}, pitch_deg=30.0,
                               near=S.NEAR, far=S.FAR, api=EMU.EmuApi())
    img = cam.update()
    assert cam.image().shape == (5, S.CAM_H, S.CAM_W) and cam.image().data_ptr() == cam.out.data_ptr()
    mt2 = mt.copy()
    mt2[:, :3] = np.where(np.array([0, 1, 0, 1, 1])[:, None] == 0, [0.3, 0.0, 0.05], [0.25, 0.0, 0.03])
    mt2[:, 3:] = sensors.quat_from_pitch(30.0)
    d, scl = sensors.pinhole_dirs(S.CAM_W, S.CAM_H, S.CAM_HFOV)
    want, _ = EMU.cast(sc, rs, mt2, d, S.NEAR, S.FAR, scale=scl)
    np.testing.assert_array_equal(img.numpy(), want)
    li = sensors.lidar(env, 4, 20.0, 30, mount_pos=(0.0, 0.0, 0.1), far=4.0, env_stride=2, api=EMU.EmuApi())
    rng = li.update().numpy()
    assert rng.shape == (5, 120) and (rng[1::2] == np.float32(4.0)).all() and (rng[0::2] < 4.0).any()
    with pytest.raises(ValueError):
        sensors.RaySensor(env, dirs, mount_pos=np.zeros((2, 3)), api=EMU.EmuApi())
    with pytest.raises(ValueError):
        sensors.RaySensor(env, dirs, mount_pos={"aliengo": (0, 0, 0)}, api=EMU.EmuApi())


def test_env_sensors_through_the_emulated_robot():
    """LeggedRobot.add_sensor on the lane emulator of kernels A / B: nothing is launched without a sensor; with one, every step and reset ends
    with its launch on the post-step root_states"""
    import eval_emu_binding
    from helpers import C
    from isaacgymloco_amd.envs import sensors
    cfg = C.mixed_cfg("aliengo", {"aliengo": 0.5, "go2": 0.5})[0]
    cfg.env.num_envs = 4
    cfg.terrain.num_rows, cfg.terrain.num_cols = 2, 2
    cfg.terrain.terrain_proportions = [0.0, 0.0, 0.0, 0.0, 0.5, 0.5]
    env = eval_emu_binding.emu_mixed_env(cfg)
    assert env.sensors == {}
    env.reset()
    # the numpy packer of the reference's scenes restates what lsim_create builds from the height grid
    words = env.buf["terrain_mesh"].numpy()
    mine = REF.pack_words(env.terrain.heightsamples, env.lcfg.horizontal_scale, env.lcfg.vertical_scale, env.lcfg.mesh_type, env.lcfg.slope_threshold)
    np.testing.assert_array_equal(words.view(np.uint32), mine.view(np.uint32))
    assert ((words.view(np.uint32) >> 20) & 1).any()
    cam = env.add_sensor("depth", sensors.depth_camera(env, 8, 6, 87.0, mount_pos={"aliengo": (0.3, 0, 0.05), "go2": (0.25, 0, 0.03)}, pitch_deg=30.0,
                                                       near=0.05, far=5.0, api=EMU.EmuApi()))
    with pytest.raises(ValueError):
        env.add_sensor("depth", cam)
    import torch
    env.step_device(torch.zeros(4, 12))
    live = env.sensors["depth"].image().clone()
    assert live.shape == (4, 6, 8) and bool((live < 5.0).any()) and bool(torch.isfinite(live).all())
    again = cam.update().clone()                  # the step's own launch saw the same post-step root_states
    assert torch.equal(again.reshape(4, 6, 8), live)
    sc = {"mesh_type": int(env.lcfg.mesh_type), "words": env.buf["terrain_mesh"].numpy(), "hs": env.lcfg.horizontal_scale, "vs": env.lcfg.vertical_scale,
          "border": env.lcfg.border_size}
    want, _ = EMU.cast(sc, env.root_states.numpy(), cam.mount.numpy(), cam.dirs.numpy(), 0.05, 5.0, scale=cam.scale.numpy())
    np.testing.assert_array_equal(live.reshape(4, -1).numpy(), want)
