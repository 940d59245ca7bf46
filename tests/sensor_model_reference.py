"""TEST INFRASTRUCTURE -- numpy reference of the sensor model, written from the comment of lsim_sensor_capture in include/lsim.h (not from
the kernel source): which envs are due, the per-ray model on a given clean frame, and the history state machine.

The ray cast itself is not repeated here: `raw` (the clean frame, rb.rc.out) and `hit` are taken from the launch under test and checked
elsewhere -- bit for bit against lsim_raycast / lsim_raycast_bodies by the identity tests.  `hit` is label != 0 of a launch that writes labels
(terrain-only form: exactly t < far; with bodies a body met at exactly t == far would be labelled without being a hit: no scene has one).

Everything is evaluated in float32, one rounding per operation, left to right.  The kernel may contract a product and a sum, so y is compared
with atol(...) below, the issue's bound: 8 * 2^-24 * M * |gain|, M = max(|clip_lo|, |clip_hi|, far + 3 (sigma0 + sigma2 far^2)) -- eight fp32
roundings of values no larger than M (|g| <= 3).  The dropout decision compares two values that both sides form exactly (u3 is an integer
times 2^-24, p_drop a given float), and a history shift copies: those are compared exactly."""
import numpy as np

import philox_np
from helpers import abi

TAG = abi.RNG_TAGS["sensor"]
FILL_ALL, RESETS_ONLY = abi.DEFINES["LSIM_SENSOR_FILL_ALL"], abi.DEFINES["LSIM_SENSOR_RESETS_ONLY"]
F = np.float32


def atol(p, far):
    m = max(abs(p["clip_lo"]), abs(p["clip_hi"]), far + 3.0 * (p["sigma0"] + p["sigma2"] * far * far))
    return 8.0 * 2.0 ** -24 * m * abs(p["gain"])


def due_sets(num_envs, env_stride, tick, period, stagger, flags, episode_length):
    """(due [N], fill [N]) bool"""
    e = np.arange(num_envs, dtype=np.int64)
    visited = e % env_stride == 0
    fill = visited & (bool(flags & FILL_ALL) | (np.asarray(episode_length) == 0))
    on_tick = (tick + (e if stagger else 0)) % period == 0
    due = fill | (visited & on_tick & (not (flags & RESETS_ONLY)))
    return due, fill


def uniforms(seed, rank, envs, tick, stream_id, num_rays):
    """u [4, len(envs), R] float32"""
    e = np.asarray(envs, np.uint32)[:, None]
    r = np.arange(num_rays, dtype=np.uint32)[None, :]
    x = philox_np.philox4x32_10(e, np.uint32(tick & 0xFFFFFFFF), np.uint32(TAG), np.uint32(stream_id << 16) | r, seed, rank)
    return np.stack([(w >> np.uint32(8)).astype(F) * F(2.0 ** -24) for w in x])


def gauss(u):
    return F(2.0) * ((u[0] + u[1] + u[2]) - F(1.5))


def model(raw, hit, envs, tick, p):
    """y [len(envs), R] float32 and the dropped mask for the clean rows raw [len(envs), R] of `envs`; p: dict of the struct's scalar fields"""
    raw = np.asarray(raw, F)
    u = uniforms(p["seed"], p["rank"], envs, tick, p["stream_id"], raw.shape[1])
    g = gauss(u)
    noisy = raw + (F(p["sigma0"]) + F(p["sigma2"]) * raw * raw) * g
    v = np.where(hit, noisy, raw).astype(F)
    dropped = hit & (u[3] < F(p["p_drop"]))
    v = np.where(dropped, F(p["drop_value"]), v).astype(F)
    v = np.minimum(np.maximum(v, F(p["clip_lo"])), F(p["clip_hi"]))
    return ((v - F(p["offset"])) * F(p["gain"])).astype(F), dropped


def advance(hist, y, due, fill):
    """the history after a launch: hist [N, K, R] before it, y [N, R] (rows of envs that are not due are ignored)"""
    new = hist.copy()
    for e in np.nonzero(due)[0]:
        if fill[e]:
            new[e, :] = y[e][None, :]
        else:
            new[e, :-1] = hist[e, 1:]
            new[e, -1] = y[e]
    return new
