"""TEST INFRASTRUCTURE -- numpy reference of the two instrument launches, written from the comments of lsim_sensor_instrument and
lsim_sensor_capture_inst in include/lsim.h (not from the kernel source): which rows are written, the five draws and the row they give; and,
for the capture, the field-of-view transform of a ray, the per-ray model under a row and the history state machine with a per-env latency.

THE DRAW LAUNCH.  u_k = (x_k >> 8) * 2^-24 and 2 u_k - 1 are exact in fp32, and so is the set of rows written.  j = min(span, floor(u_0 (span + 1)))
is one fp32 product of two given floats, with no sum to fuse into, then floor and min: the reference forms the same product in fp32 and gets the
same integer, so `lat` is compared exactly.
Bounds of the other four, evaluated here in fp64 from the fp32 inputs; the launch is fp32 with one rounding per operation (u = 2^-24
relative), a product and a sum possibly fused (fewer roundings, never more):
  noise_gain  = lo + u_1 (hi - lo): the difference d errs by u d, the product by u d more, the sum by u (lo + d (1 + 2 u))   -> 4 u (lo + d)
  depth_scale = (2 u_2 - 1) r: the factor is exact, one rounding of a product of magnitude <= r                              -> u r
  depth_quad  likewise                                                                                                        -> u r
  tan_scale   = 1 + (2 u_4 - 1) f: the product errs by u f, the sum by u (1 + f (1 + u))                                      -> 2 u (1 + f)
Neither bound has seen the kernel's output.

THE CAPTURE.  As in tests/sensor_model_reference.py the ray cast is not repeated: `raw` (the clean frame) and `hit` are taken from the launch
under test; the field-of-view tests check them against tests/raycast_reference.py at the directions `scaled_dirs` gives.
  model_inst: fp32, one rounding per operation, left to right.  Its tolerance extends that module's 8 u M |gain|: the line for v has five more
  operations (depth_quad * raw, + depth_scale, 1 +, raw *, noise_gain *), each of which rounds a value no larger than
  M' = max(|clip_lo|, |clip_hi|, far (1 + c) + 3 g_max (sigma0 + sigma2 far^2)),  c = |depth_scale| + |depth_quad| far  -> 13 u M' |gain|   (atol_inst).
  scaled_dirs: fp64 from the fp32 dirs and tan_scale.  The launch forms s' in fp32: y' = s.y T and z' = s.z T (1 rounding each), the radicand
  (3 products, 2 sums: relative 2.5 u on a sum of positive terms, + 2 u from y', z' squared), its correctly rounded root (half of that, + u),
  the correctly rounded quotient q (+ u), and the three products with q (+ u, + u for y', z'): every component of s' within 6 u relatively,
  so s' is tilted from the fp64 direction by at most 6 u sqrt(2) < 5.1e-7 rad (`TILT_BOUND`)."""
import numpy as np

import philox_np
import sensor_model_reference as SR
from helpers import abi

TAG = abi.RNG_TAGS["sensor_instrument"]
FILL_ALL, RESETS_ONLY = SR.FILL_ALL, SR.RESETS_ONLY
F = np.float32
U = 2.0 ** -24
TILT_BOUND = 6.0 * U * np.sqrt(2.0)


def fresh_set(num_envs, env_stride, flags, episode_length):
    """[N] bool: the rows the draw launch writes"""
    e = np.arange(num_envs, dtype=np.int64)
    return (e % env_stride == 0) & (bool(flags & FILL_ALL) | (np.asarray(episode_length) == 0))


def uniforms(seed, rank, envs, tick, stream_id):
    """u [len(envs), 5] float32, exact: block 0's four words and block 1's first"""
    e = np.asarray(envs, np.uint32)
    blocks = []
    for b in (0, 1):
        x = philox_np.philox4x32_10(e, np.uint32(tick & 0xFFFFFFFF), np.uint32(TAG), np.uint32((stream_id << 16) | b), seed, rank)
        blocks.append(np.stack([(w >> np.uint32(8)).astype(F) * F(U) for w in x], axis=1))
    return np.concatenate(blocks, axis=1)[:, :5]


def latency(u0, lat_lo, lat_hi):
    """the integer latency of each env, exact (module docstring)"""
    span = lat_hi - lat_lo
    j = np.floor((np.asarray(u0, F) * F(span + 1)).astype(F)).astype(np.int64)
    return lat_hi - np.minimum(span, j)


def rows(u, r):
    """fp64 [len(u), 8]: the rows of the envs whose uniforms are given; r: dict of the struct's seven range fields (as the struct holds them)"""
    u = np.asarray(u, F).astype(np.float64)
    f = lambda k: float(F(r[k]))
    out = np.zeros((u.shape[0], 8))
    out[:, 0] = latency(u[:, 0], int(r["lat_lo"]), int(r["lat_hi"]))
    out[:, 1] = f("gain_lo") + u[:, 1] * (f("gain_hi") - f("gain_lo"))
    out[:, 2] = (2.0 * u[:, 2] - 1.0) * f("scale_range")
    out[:, 3] = (2.0 * u[:, 3] - 1.0) * f("quad_range")
    out[:, 4] = 1.0 + (2.0 * u[:, 4] - 1.0) * f("fov_range")
    return out


def bound(r):
    """[8]: per column, the distance the launch may be from rows() (module docstring); 0 where the value is exact"""
    f = lambda k: float(F(r[k]))
    return np.array([0.0, 4.0 * U * (f("gain_lo") + (f("gain_hi") - f("gain_lo"))), U * f("scale_range"), U * f("quad_range"),
                     2.0 * U * (1.0 + f("fov_range")), 0.0, 0.0, 0.0])


def expected(before, fresh, seed, rank, tick, stream_id, r):
    """(want fp64 [N, 8], tol [N, 8]) of a launch over `before`: rows that are not fresh keep what they held"""
    want, tol = np.asarray(before, F).astype(np.float64), np.zeros(np.shape(before))
    envs = np.nonzero(fresh)[0]
    want[envs] = rows(uniforms(seed, rank, envs, tick, stream_id), r)
    tol[envs] = bound(r)[None, :]
    return want, tol


# ---- the capture
def scaled_dirs(dirs, scale, tan_scale):
    """(s' [R, 3], sc' [R]) fp64 of the header's field-of-view transform for one tan_scale; rays with s.x <= 0 and tan_scale == 1: untouched"""
    s = np.asarray(dirs, F).astype(np.float64)
    sc = np.ones(s.shape[0]) if scale is None else np.asarray(scale, F).astype(np.float64)
    T = float(F(tan_scale))
    if T == 1.0:
        return s, sc
    v = s * np.array([1.0, T, T])
    n = np.linalg.norm(v, axis=1)
    on = s[:, 0] > 0.0
    return np.where(on[:, None], v / n[:, None], s), np.where(on, sc / n, sc)


def atol_inst(p, far, rows, raw_max=None):
    """13 u M' |gain| (module docstring) for the rows in use; raw_max: the largest clean value (far times the largest scale)"""
    rows = np.atleast_2d(np.asarray(rows, np.float64))
    d = far if raw_max is None else raw_max
    c = np.abs(rows[:, 2]).max() + np.abs(rows[:, 3]).max() * d
    m = max(abs(p["clip_lo"]), abs(p["clip_hi"]), d * (1.0 + c) + 3.0 * np.abs(rows[:, 1]).max() * (p["sigma0"] + p["sigma2"] * d * d))
    return 13.0 * U * m * abs(p["gain"])


def model_inst(raw, hit, envs, tick, p, rows):
    """y [len(envs), R] float32 and the dropped mask for the clean rows raw [len(envs), R] of `envs` under their `rows` [len(envs), 8]"""
    raw = np.asarray(raw, F)
    rows = np.asarray(rows, F)
    ng, ds, dq = (rows[:, k][:, None] for k in (1, 2, 3))
    u = SR.uniforms(p["seed"], p["rank"], envs, tick, p["stream_id"], raw.shape[1])
    g = SR.gauss(u)
    m = raw * (F(1.0) + (ds + dq * raw))
    noisy = m + (ng * (F(p["sigma0"]) + F(p["sigma2"]) * raw * raw)) * g
    v = np.where(hit, noisy, raw).astype(F)
    dropped = hit & (u[3] < F(p["p_drop"]))
    v = np.where(dropped, F(p["drop_value"]), v).astype(F)
    v = np.minimum(np.maximum(v, F(p["clip_lo"])), F(p["clip_hi"]))
    return ((v - F(p["offset"])) * F(p["gain"])).astype(F), dropped


def slots(lat, latency, frames, off_by=0):
    """Ke [N] of the header: clamp((int) lat, 0, latency) + frames.  `off_by`: the mutant that shifts through one slot more or fewer"""
    l = np.clip(np.trunc(np.asarray(lat, np.float64)).astype(np.int64), 0, latency)
    return l + frames + off_by


def advance_inst(hist, y, due, fill, ke):
    """the history after a launch: hist [N, K, R] before it, y [N, R] (rows of envs that are not due are ignored), ke [N] from slots()"""
    new = hist.copy()
    K = hist.shape[1]
    for e in np.nonzero(due)[0]:
        if fill[e]:
            new[e, :] = y[e][None, :]
        else:
            k = int(min(max(ke[e], 1), K))          # a mutant's count may leave 1 .. K; the header's never does
            new[e, :k - 1] = hist[e, 1:k]
            new[e, k - 1:] = y[e][None, :]
    return new
