"""TEST INFRASTRUCTURE -- the scenes of the foot-scan launch (lsim_foot_scan), run by tests/test_foot_scan.py on the CPU shim and by
tests/test_gpu_foot_scan.py on the HIP launch.  A scene is a dict of the launch's inputs (tests/foot_scan_reference.py reads it,
tests/foot_scan_emu_binding.py turns it into a struct); `run(make_rig, scene, exact)` launches it once and applies the reference's rule.

EXACT scenes: every joint angle 0, a robot table whose joint offsets are multiples of 1/16 m, the identity pose or a yaw of 90 degrees, a
pattern of multiples of 1/16 m, horizontal_scale 1/8, res 1/16 and a base position whose x and y are ODD multiples of 1/32.  Every foot and
every point then sits on an odd multiple of 1/32: in the middle of a map cell and a quarter into a terrain cell, so the 2^-24 that the fp32
yaw quaternion (0, 0, sqrt(1/2), sqrt(1/2)) is off by moves no point into another cell; the heights are stored values, and the foot's z
(R(q) keeps z exactly for a yaw-only q: u x v has no z for u along z) and with it every row value is exact.  Everything is compared bit
for bit.

GENERAL scenes: Aliengo's and Go2's tables in one launch, random poses with |p| <= 8 m, roll and pitch up to 0.5 rad, any yaw, joint angles
within 0.4 rad of the standing pose (inside both robots' limits); the reference's ambiguity rule applies."""
import numpy as np

import foot_scan_emu_binding as FB
import foot_scan_reference as FR

F = np.float32
SQH = np.sqrt(F(0.5))                       # fp32
STAND = np.array([0.0, 0.8, -1.5] * 4, F)
_cache = {}


def real_tables():
    """[lsim_raycast_robot of Aliengo, of Go2]"""
    import raycast_bodies_scenes as BS
    return BS.tables()[0]


def dyadic_table(zero_legs=False):
    """Aliengo's table with joint offsets that are multiples of 1/16 m (zero_legs: all zero, every foot is the base)"""
    from helpers import abi
    t = abi.LsimRaycastRobot.from_buffer_copy(real_tables()[0])
    for l in range(4):
        sx, sy = (1.0 if l < 2 else -1.0), (1.0 if l % 2 == 0 else -1.0)
        offs = [(0.25 * sx, 0.0625 * sy, 0.0), (0.0, 0.0625 * sy, 0.0), (0.0, 0.0, -0.25), (0.0625 * sx, 0.0, -0.1875)]
        for k in range(4):
            for c in range(3):
                t.bodies[1 + 4 * l + k].joint_pos[c] = 0.0 if zero_legs else offs[k][c]
    return t


def dyadic_pattern(K):
    """[K, 2] multiples of 1/16 m: the centre, a cross, far points that leave the terrain grid and the map window, then a spiral of small steps"""
    pts = [(0.0, 0.0), (0.0625, 0.0), (0.0, -0.125), (-0.1875, 0.0625), (0.25, 0.25), (-6.0, 0.5), (0.5, 9.0)]
    k = 0
    while len(pts) < K:
        k += 1
        pts.append((0.0625 * ((k * 3) % 9 - 4), 0.0625 * ((k * 5) % 7 - 3)))
    return np.array(pts[:K], F)


def exact_poses(N):
    """[N, 13]: odd multiples of 1/32 in x and y, identity and 90-degree yaw alternating, one env near the terrain grid's corner"""
    pose = np.zeros((N, 13), F)
    for e in range(N):
        pose[e, :3] = [0.53125 + 0.4375 * e, -0.21875 + 0.3125 * e, 0.4375 + 0.0625 * e]
        pose[e, 3:7] = [0, 0, 0, 1] if e % 2 == 0 else [0, 0, SQH, SQH]
    if N > 2:
        pose[2, :2] = [-0.84375, -0.90625]
    return pose


def window_map(pose, G, res, seed, centres=None):
    """(height, stamp, cell) [N, G, G]: per env the window of G x G cells centred on the pose; a third of the slots know their cell, a third
    hold a cell that has scrolled out (the same slot, G cells away) and a third were never written.  `centres` [N, 4, 2]: the slot under
    foot 0 knows its cell, under foot 1 is left over, under foot 2 never written"""
    g = np.random.RandomState(seed)
    N = pose.shape[0]
    height = g.uniform(-1.2, 1.4, (N, G, G)).astype(F)          # past both limits of the clamp
    stamp = np.full((N, G, G), -1, np.int32)
    cell = np.zeros((N, G, G), np.uint32)
    kind = g.randint(0, 3, (N, G, G))
    for e in range(N):
        if not np.isfinite(pose[e, :2]).all():
            continue
        c = np.floor(pose[e, :2].astype(np.float64) / res).astype(np.int64)
        w0 = c - G // 2
        if centres is not None and np.isfinite(centres[e]).all():
            for l in range(3):
                ci = np.floor(centres[e, l] / res).astype(np.int64)
                kind[e, ci[0] & (G - 1), ci[1] & (G - 1)] = l
        for sx in range(G):
            for sy in range(G):
                ix, iy = w0[0] + ((sx - w0[0]) & (G - 1)), w0[1] + ((sy - w0[1]) & (G - 1))
                if kind[e, sx, sy] == 1:
                    ix -= G
                if kind[e, sx, sy] != 2:
                    stamp[e, sx, sy] = g.randint(0, 1000)
                    cell[e, sx, sy] = ((ix + 32768) << 16) | (iy + 32768)
    return height, stamp, cell


def exact_scene(source, N, K, G=16, env_stride=1, channels=2, mesh_type=1):
    pose = exact_poses(N)
    sc = dict(source=source, pose=pose, dof_pos=np.zeros((N, 12), F), tables=[dyadic_table()], env_robot=None, pattern=dyadic_pattern(K),
              env_stride=env_stride, channels=channels, z_offset=0.0625, scale=5.0)
    if source == FR.TERRAIN:
        g = np.random.RandomState(3)
        sc.update(mesh_type=mesh_type, height_grid=g.randint(-60, 120, (28, 22)).astype(np.int16), hs=0.125, vs=0.005, border=1.0)
    else:
        res = 0.0625
        centres = pose[:, None, :2].astype(np.float64) + np.stack([FR.feet(FR.bodies_of(sc["tables"][0]), pose[e, 3:7].astype(np.float64), np.zeros(12))[:, :2]
                                                                   for e in range(N)])
        h, s, c = window_map(pose, G, res, seed=5 + G, centres=centres)
        sc.update(G=G, res=res, unknown_drop=0.5, height=h, stamp=s, cell=c)
    return sc


EXACT_CASES = [(src, N, K, G, stride) for src in (FR.TERRAIN, FR.MAP) for N, stride in ((1, 1), (5, 1), (5, 3)) for K in (1, 7, 64)
               for G in ((16, 64) if src == FR.MAP else (16,))]


GENERAL_CASES = [(FR.TERRAIN, 7, 16), (FR.TERRAIN, 64, 16)] + [(FR.MAP, K, G) for K in (7, 64) for G in (16, 64)]       # the terrain source has no G


def quat_rpy(r, p, y):
    cr, sr, cp, sp, cy, sy = np.cos(r / 2), np.sin(r / 2), np.cos(p / 2), np.sin(p / 2), np.cos(y / 2), np.sin(y / 2)
    return [sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy]


def ring_pattern(K, seed=2):
    g = np.random.RandomState(seed)
    r, a = g.uniform(0.0, 0.22, K), g.uniform(0, 2 * np.pi, K)
    pts = np.stack((r * np.cos(a), r * np.sin(a)), -1)
    pts[0] = 0.0
    return pts.astype(F)


def general_scene(source, N, K, G=16, env_stride=1, channels=2, seed=1):
    key = (source, N, K, G, env_stride, channels, seed)
    if key in _cache:
        return _cache[key]
    g = np.random.RandomState(seed + 13 * K + G)
    pose = np.zeros((N, 13), F)
    pose[:, 0:2] = g.uniform(-8.0, 8.0, (N, 2))
    pose[:, 2] = g.uniform(0.25, 0.6, N)
    for e in range(N):
        pose[e, 3:7] = quat_rpy(g.uniform(-0.5, 0.5), g.uniform(-0.5, 0.5), g.uniform(-np.pi, np.pi))
    th = (STAND[None, :] + g.uniform(-0.4, 0.4, (N, 12))).astype(F)
    sc = dict(source=source, pose=pose, dof_pos=th, tables=real_tables(), env_robot=g.randint(0, 2, N).astype(np.uint8), pattern=ring_pattern(K),
              env_stride=env_stride, channels=channels, z_offset=0.02, scale=5.0)
    if source == FR.TERRAIN:
        sc.update(mesh_type=1, height_grid=g.randint(-300, 300, (200, 200)).astype(np.int16), hs=0.1, vs=0.005, border=10.0)
    else:
        h, s, c = window_map(pose, G, 0.0625, seed=seed + G)
        sc.update(G=G, res=0.0625, unknown_drop=0.4, height=h, stamp=s, cell=c)
    _cache[key] = sc
    return sc


def run(make_rig, sc, exact, label="", stream=None, ref=None):
    """one launch of `sc` against the reference; returns (what the rig read, the reference, the ambiguous share)"""
    ref = ref or FR.reference(sc)
    rig = make_rig(sc)
    got = rig.run(stream=stream)
    share = FR.check(sc, ref, got, exact, label)
    if not exact:
        print(f"{label}: {share:.4%} of {int(ref['visited'].sum()) * ref['heights'].shape[1]} points ambiguous")
    return got, ref, share


def refusals(make_rig, null_call, launches=True):
    """every LSIM_E_INVALID of the header for both sources, nothing written by any of them (the bits before and after)"""
    from helpers import abi
    E = abi.E_INVALID
    assert null_call() == E
    nan, inf = float("nan"), float("inf")

    def field(name, value):
        def edit(fs):
            setattr(fs, name, value)
        return edit

    def shifted(name, by):
        def edit(fs):
            setattr(fs, name, getattr(fs, name) + by)
        return edit

    def no_robot_table(fs):
        fs.env_robot, fs.num_robots = None, 2

    common = [field(n, None) for n in ("pose", "dof_state", "robots", "robots_host", "pattern", "rows", "state")] + \
             [shifted(n, 2) for n in ("pose", "dof_state", "robots", "robots_host", "pattern", "rows", "heights")] + [shifted("state", 4)] + \
             [field("source", 2), field("source", -1), field("num_envs", 0), field("env_stride", 0), field("num_robots", 0), field("num_robots", 5), no_robot_table,
              field("num_points", 0), field("num_points", 65), field("channels", 0), field("channels", 3), field("ld", 2 * 4 * 7 - 1),
              field("heights_stride", 27), field("known_stride", 27), field("z_offset", nan), field("z_offset", inf), field("scale", nan), field("scale", -inf)]
    terrain = [field("height_grid", None), shifted("height_grid", 1), field("grid_rows", 1), field("grid_cols", 1), field("grid_rows", 1 << 30),
               field("horizontal_scale", 0.0), field("horizontal_scale", -0.1), field("horizontal_scale", nan), field("horizontal_scale", inf),
               field("vertical_scale", 0.0), field("vertical_scale", nan), field("vertical_scale", inf), field("border_size", nan), field("border_size", inf)]
    amap = [field("height", None), field("stamp", None), field("cell", None), shifted("height", 2), shifted("stamp", 2), shifted("cell", 2),
            field("size", 0), field("size", 8), field("size", 48), field("size", 128), field("res", 0.0), field("res", -1.0), field("res", nan), field("res", inf),
            field("unknown_drop", nan), field("unknown_drop", inf)]
    for source, own in ((FR.TERRAIN, terrain), (FR.MAP, amap)):
        sc = exact_scene(source, 3, 7)
        rig = make_rig(sc)
        before = {k: rig.raw(k).copy() for k in ("rows", "heights", "known", "state")}
        for e in common + own:
            assert rig.launch(edit=e) == E, (source, e)
        # a robot table whose tree is not the one lsim_raycast_bodies accepts, or with a non-finite joint offset: checked in robots_host
        for body, name, value in ((5, "parent", 3), (0, "dof", 0), (3, "dof", 12), (3, "dof", -2)):
            old = getattr(rig._tables[0].bodies[body], name)
            setattr(rig._tables[0].bodies[body], name, value)
            assert rig.launch() == E, (body, name, value)
            setattr(rig._tables[0].bodies[body], name, old)
        for body, name in ((2, "joint_pos"), (7, "joint_axis")):
            old = getattr(rig._tables[0].bodies[body], name)[1]
            getattr(rig._tables[0].bodies[body], name)[1] = nan
            assert rig.launch() == E, (body, name)
            getattr(rig._tables[0].bodies[body], name)[1] = old
        for k, v in before.items():
            assert np.array_equal(rig.raw(k).view(np.uint8), v.view(np.uint8)), f"a refused launch wrote {k}"
        rig.assert_guards()
        if launches:
            def optional_off(fs):                  # heights, known and their strides play no part when the pointers are NULL
                fs.heights, fs.known, fs.heights_stride, fs.known_stride = None, None, 0, 0
            assert rig.launch(edit=optional_off) == 0 and rig.launch(edit=field("channels", 1)) == 0
            if source == FR.TERRAIN:
                def plane(fs):                     # the plane reads no grid
                    fs.mesh_type, fs.height_grid, fs.grid_rows, fs.horizontal_scale = 0, None, 0, 0.0
                assert rig.launch(edit=plane) == 0
            rig.assert_guards()
