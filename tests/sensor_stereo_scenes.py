"""TEST INFRASTRUCTURE -- hand-built depth rows for lsim_sensor_stereo.  The launch reads `depth`, so a scene needs no ray cast: it is the
image itself.  Where a width is asserted the scene is DYADIC -- fb and every Z a power of two, so delta = fb / Z is exact -- and `holes`
states the band by hand; everywhere else the reference of tests/sensor_stereo_reference.py is the expectation.

A scene: dict(name, width, height, depth [N, R], labels [N, R] | None, inv_scale [R] | None, inst [N, 8] | None, params (the struct's
by-value fields over sensor_stereo_emu_binding.DEFAULTS), holes: [N, H, W] bool | None -- the exact set of holes, asserted by hand)."""
import numpy as np

F = np.float32
PLANE, BOX, FB = 4.0, 1.0, 8.0            # delta 2 and 8: a band of 6 columns


def _plane(N, W, H, Z=PLANE):
    return np.full((N, H, W), Z, F)


def _scene(name, depth, params, labels=None, inv_scale=None, inst=None, holes=None):
    N, H, W = depth.shape
    return dict(name=name, width=W, height=H, depth=depth.reshape(N, -1), labels=None if labels is None else labels.reshape(N, -1),
                inv_scale=inv_scale, inst=inst, params=params, holes=holes)


def _inst(N, latency):
    """rows {lat, 1, 0, 0, tan_scale, 0, 0, 0}: per-env latency 0 .. 2 (at most `latency`) and tan_scale 0.98 / 1 / 1.02"""
    rows = np.zeros((N, 8), F)
    rows[:, 0] = np.minimum(np.arange(N) % 3, latency)
    rows[:, 1] = 1.0
    rows[:, 4] = np.array([0.98, 1.0, 1.02], F)[np.arange(N) % 3]
    return rows


def box(window, W=16, H=6, c_box=9, latency=0, frames=1, env_stride=1, inst=False, mirrored=False):
    """a fronto-parallel box (Z = 1, three columns wide, rows 1 .. H - 2) in front of a plane (Z = 4), fb = 8: the plane's pixels in the
    box's rows are shadowed exactly in the columns c_box - 6 <= c < c_box that also have c' <= c + window for the box's first column c'"""
    N = 3
    d = _plane(N, W, H)
    d[:, 1:H - 1, c_box:c_box + 3] = BOX
    holes = np.zeros((N, H, W), bool)
    lo = max(c_box - 6, c_box - window, 0)
    holes[:, 1:H - 1, lo:c_box] = True
    holes[np.arange(N) % env_stride != 0] = False
    params = dict(fb=FB, window=window, latency=latency, frames=frames, env_stride=env_stride, max_disparity=64.0, edge_radius=1, drop_value=-1.0,
                  clip_lo=0.125, clip_hi=8.0, offset=4.0625, gain=0.125)
    name = f"{'mirrored_' if mirrored else ''}box_{W}x{H}_w{window}_K{latency + frames}_s{env_stride}{'_inst' if inst else ''}"
    return _scene(name, d, params, inst=_inst(N, latency) if inst else None, holes=None if inst else holes)


def slanted(W=20, H=5):
    """a plane slanted along the columns, disparity 2 + c / 2 (a slope of half a pixel per pixel): u rises by about 1 / 2 per column, no shadow"""
    N = 3
    delta = 2.0 + 0.5 * np.arange(W)
    d = np.broadcast_to((FB / delta).astype(F)[None, None, :], (N, H, W)).copy()
    params = dict(fb=FB, window=W - 1, latency=1, frames=2, edge_radius=0, edge_rel=0.0)
    return _scene("slanted_20x5", d, params, holes=np.zeros((N, H, W), bool))


def per_pixel(p_hole, p_cum, latency=1, frames=2, radius=1):
    """a plane with a miss, a NaN, a near pixel whose label is 0 (it must occlude nobody) and a too-near pixel that still occludes:
    16 x 6, labels, max_disparity 16.  Env 1 has no special pixel at all, env 2 only the too-near one"""
    N, W, H = 3, 16, 6
    d, lab = _plane(N, W, H), np.ones((N, H, W), np.uint8)
    d[0, 1, 5], d[0, 2, 6] = 100.0, np.nan                  # a miss beyond t_hi, a NaN
    d[0, 3, 9], lab[0, 3, 9] = 0.5, 0                       # delta 16, but nothing is there
    d[0, 4, 12], d[2, 4, 12] = 0.25, 0.25                   # delta 32 > 16: a hole, and the plane left of it is shadowed (c >= 12 - 30)
    lab[0, 4, 12] = lab[2, 4, 12] = 3
    holes = None
    if p_hole == 0.0 and p_cum == 0.0:
        holes = np.zeros((N, H, W), bool)
        holes[0, 4, 4:13] = holes[2, 4, 4:13] = True        # window 8: columns 4 .. 11 shadowed, 12 too near
    params = dict(fb=FB, window=8, latency=latency, frames=frames, max_disparity=16.0, edge_radius=radius, p_edge_hole=p_hole, p_edge_cum=p_cum,
                  drop_value=-1.0, clip_lo=0.125, clip_hi=8.0, offset=4.0625, gain=0.125)
    return _scene(f"per_pixel_h{p_hole}_c{p_cum}_r{radius}", d, params, labels=lab, holes=holes)


def tie():
    """two foreground pixels of the same Z side by side above a background pixel, every edge pixel fattened: the foreground is the LEFT one
    (the smaller index), and the two hold different values in hist"""
    N, W, H = 3, 16, 6
    d = _plane(N, W, H)
    d[:, 2, 5:7] = 2.0                                      # delta 4: not too near
    params = dict(fb=FB, window=8, latency=0, frames=3, edge_radius=1, p_edge_hole=0.0, p_edge_cum=1.0)
    return _scene("tie", d, params)


def general(seed=11):
    """64 x 48, N = 3 with env_stride 2: a pinhole's inv_scale, labels, boxes of several depths on a slanted floor, K = 8, per-env
    instrument rows, radius 3, probabilities 0.3 / 0.3"""
    N, W, H = 3, 64, 48
    rng = np.random.default_rng(seed)
    d = np.broadcast_to((0.6 + 3.0 * (1.0 - np.arange(H) / H))[None, :, None], (N, H, W)).astype(F).copy()
    lab = np.ones((N, H, W), np.uint8)
    for e in range(N):
        for _ in range(6):
            y, x, h, w = rng.integers(0, H - 8), rng.integers(0, W - 8), rng.integers(3, 16), rng.integers(2, 12)
            d[e, y:y + h, x:x + w] = F(rng.uniform(0.15, 1.5))
            lab[e, y:y + h, x:x + w] = 2 + rng.integers(0, 5)
        miss = rng.random((H, W)) < 0.03
        d[e][miss], lab[e][miss] = 5.0, 0
    tx = np.tan(np.radians(87.0) / 2.0)
    ys, zs = (1.0 - (2.0 * np.arange(W) + 1.0) / W) * tx, (1.0 - (2.0 * np.arange(H) + 1.0) / H) * tx * H / W
    inv_scale = np.sqrt(1.0 + ys[None, :] ** 2 + zs[:, None] ** 2).reshape(-1).astype(F)
    params = dict(fb=F(32.0 / tx * 0.05), window=40, latency=2, frames=6, env_stride=2, max_disparity=10.0, t_lo=F(0.05 * inv_scale.max()),
                  t_hi=F(4.9 * inv_scale.min()), edge_radius=3, edge_rel=0.05, p_edge_hole=0.3, p_edge_cum=F(F(0.3) + F(0.3)), drop_value=0.0,
                  clip_lo=0.05, clip_hi=5.0, offset=2.525, gain=F(1.0 / 4.95))
    return _scene("general_64x48", d, params, labels=lab, inv_scale=inv_scale, inst=_inst(N, 2))


def scenes():
    return [box(window=8), box(window=3), box(window=8, W=20, H=5, c_box=3, latency=1, frames=2, mirrored=True),
            box(window=8, latency=2, frames=1, env_stride=2), box(window=8, latency=2, frames=1, inst=True), slanted(),
            per_pixel(0.0, 0.0), per_pixel(1.0, 1.0), per_pixel(0.0, 1.0), per_pixel(0.3, 0.6, radius=3), per_pixel(0.0, 1.0, latency=0, frames=1, radius=0),
            tie(), general()]
