"""TEST INFRASTRUCTURE -- the scenarios of the map-rows launch (lsim_map_rows), run by tests/test_map_rows.py on the CPU shim and by
tests/test_gpu_map_rows.py on the HIP launch: each takes `make_rig`, a RowsRig factory of tests/odometry_emu_binding.py.  The reference is
fp32 numpy written from the header's comment: two subtractions, a clamp and one product have one rounding each and nothing to fuse, so every
comparison is bit for bit."""
import numpy as np

import odometry_emu_binding as OB

F = np.float32
CASES = [(N, P, C) for N in (1, 3) for P in (1, 99, 187, 256) for C in (1, 2)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def reference(scan, known, pose_z, P, channels, z_offset, scale, rows_before, env_stride=1):
    """rows [N, ld] fp32 after the launch: include/lsim.h, lsim_map_rows"""
    out = np.array(rows_before, F)
    for e in range(0, out.shape[0], env_stride):
        z, s = F(pose_z[e]), np.asarray(scan[e, :P], F)
        with np.errstate(invalid="ignore", over="ignore"):
            t = (z - F(z_offset)) - s
            v = np.minimum(np.maximum(t, F(-1.0)), F(1.0)) * F(scale)
        out[e, :P] = np.where(np.isfinite(z) & np.isfinite(s), v, F(0.0))
        if channels == 2:
            out[e, P:2 * P] = np.where(np.asarray(known[e, :P]) != 0, F(1.0), F(0.0))
    return out


def inputs(N, P, seed=5):
    """scan around a base height with values past both clip limits, known of every byte value, one env's z and some scan values not finite"""
    g = np.random.RandomState(seed + 7 * N + P)
    z = g.uniform(0.2, 0.8, N).astype(F)
    scan = (z[:, None] - 0.5 + g.uniform(-1.6, 1.6, (N, P))).astype(F)
    known = g.randint(0, 256, (N, P)).astype(np.uint8)
    known[:, ::3] = 0
    flat = scan.reshape(-1)
    bad = g.choice(flat.size, size=min(3, flat.size), replace=False)
    flat[bad] = np.array([np.nan, np.inf, -np.inf], F)[:len(bad)]
    return z, scan, known


def case(make_rig, N, P, channels, env_stride=1, bad_z=None, stream=None, **kw):
    """one launch against the reference: the written block, the columns past it, the rows of envs not visited, the NaN padding of scan (an
    input: it must not leak) and the guard.  Returns the rows"""
    rig = make_rig(N, P, channels, env_stride=env_stride, **kw)
    z, scan, known = inputs(N, P)
    if bad_z is not None:
        z[N - 1] = bad_z
    s, k, pose = rig.get("scan"), rig.get("known"), rig.get("pose")
    s[:, :P], k[:, :P], pose[:, 2] = scan, known, z
    rig.put("scan", s)
    rig.put("known", k)
    rig.put("pose", pose)
    before = rig.read()
    assert rig.launch(stream=stream) == 0
    got = rig.read()
    want = reference(scan, known, z, P, channels, rig.mr.z_offset, rig.mr.scale, before, env_stride)
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=f"N {N} P {P} channels {channels} stride {env_stride}")
    assert np.isfinite(got).all() and (got[:, channels * P:] == OB.RowsRig.ROWS_INITIAL).all()
    assert np.isnan(rig.get("scan")[:, P:]).all() and (rig.get("known")[:, P:] == 0x7E).all()
    vis = np.arange(N) % env_stride == 0
    assert (got[~vis] == OB.RowsRig.ROWS_INITIAL).all()
    block = got[vis][:, :P]
    assert (np.abs(block) <= abs(F(rig.mr.scale))).all()
    if N * P >= 99 and bad_z is None:
        assert (block == F(rig.mr.scale)).any() and (block == -F(rig.mr.scale)).any() and (np.abs(block) < abs(F(rig.mr.scale))).any()
    return got


def refusals(make_rig, null_call, launches=True):
    """every LSIM_E_INVALID of the header, and nothing written by any of them"""
    from helpers import abi
    rig = make_rig(3, 7, 2)
    before = bits(rig.read())
    E = abi.E_INVALID
    assert null_call() == E

    def field(name, value):
        def edit(mr):
            setattr(mr, name, value)
        return edit

    def shifted(name, by):
        def edit(mr):
            setattr(mr, name, getattr(mr, name) + by)
        return edit

    edits = [field("scan", None), field("pose", None), field("rows", None), field("known", None), shifted("scan", 2), shifted("pose", 1), shifted("rows", 2),
             field("num_points", 0), field("num_points", 257), field("channels", 0), field("channels", 3), field("scan_stride", 6), field("known_stride", 6),
             field("ld", 13), field("z_offset", float("nan")), field("z_offset", float("inf")), field("scale", float("nan")), field("scale", -float("inf")),
             field("num_envs", 0), field("env_stride", 0)]
    for e in edits:
        assert rig.launch(edit=e) == E
    np.testing.assert_array_equal(before, bits(rig.read()))
    if launches:
        def one_channel(mr):                   # known and its stride play no part with one channel
            mr.channels, mr.known, mr.known_stride = 1, None, 0
        assert rig.launch(edit=one_channel) == 0 and rig.launch(edit=field("ld", 14)) == 0
