"""TEST INFRASTRUCTURE -- numpy reference of the odometry launch, written from the comment of lsim_odometry_step in include/lsim.h (not from
the kernel source): which envs are visited and fresh, the draws, the drift integration and the estimated pose.  `step` works in the dtype it
is given: float64 is the reference, float32 (numpy: one rounding per operation, nothing fused, correctly rounded roots and quotients) is the
reference's own fp32 twin, whose distance from the float64 run says how much of a bound plain fp32 arithmetic uses up.

Exact parts.  s_k = 2 (x_k >> 8) 2^-24 - 1 is exact in fp32; so are the set of rows written, prev = p.xy, the three zero words, est[7:13], a
fresh env's zero drift and its est[0:7] = root_states[0:7] (up to -0 -> +0), everything under all-zero ranges, and a non-finite pose's copy.

Bound of the general scene (`bounds`), u = 2^-24, first order in u with every count rounded up.  The launch is fp32 with one rounding per
operation, a product and a sum possibly fused (fewer roundings, never more).  K launches, steps of at most L_max metres, R the sum of the six
ranges, q a unit quaternion.  The scene keeps K R <= 1 and K L_max <= 2 (asserted on its parameters), so that every accumulated quantity stays
small: |h| <= K L_max (yaw_range + yaw_noise) / 2 <= R, |dx|, |dy| <= K L_max (scale_range + pos_noise + 2 |h|) <= 2 L_max, |dz| <= K L_max
(z_range + z_noise) <= L_max.  Per step, L the true step length:
  D = p.xy - prev                      1 rounding                                                       -> u L
  L = sqrt(D.x^2 + D.y^2)              squares 2 u (from D) + u, sum u, root halves it and adds u         -> 3 u L
  Y = yaw_bias + yaw_noise s0          bias stored rounded u, product u, sum u                          -> 2 u (yaw_range + yaw_noise); likewise k, Z
  h += (L / 2) Y                       3 u + 2 u + u (product) on an increment <= L_max R / 2, the sum u |h| <= u R
                                       -> u (3 L_max R + R) per step
  c = 1 / sqrt(1 + h^2), d = (0, 0, h c, c):  c within 3 u, h c within err(h) + u
  r = R(d) (D, 0)                      u L (D) + 2 L err(h) <= 3 u L (K L_max <= 2) + two sums 2 u L + the |h|-sized terms <= u L            -> 7 u L
  k = 1 + (scale + pos_noise s1)       u (1 + 3 R)
  k r.x - D.x                          (1 + R) 7 u L + L u (1 + 3 R) + u L (1 + R) (product) + u L (D) + u L (difference)                -> 11 u L (1 + R)
  dx += ..                             u |dx| <= 2 u L_max                                                -> 13 u L_max (1 + R) per step:   a_xy = 13
  dz += L Z                            3 u + 2 u + u on <= L_max R, the sum u L_max                      -> u L_max (6 R + 1) per step:     a_z = 6
so  err(dx), err(dy) <= 13 u K L_max (1 + R);   err(dz) <= 6 u K L_max (1 + R);   err(h) <= u K R (3 L_max + 1)
     est[0:2] : err(d) + u (|p| + |d|), |d| <= 2 L_max <= K L_max  -> u (14 K L_max (1 + R) + |p|_inf)   (a = 14);  est[2]: a = 7.
                The sum's rounding is ONE rounding, which reaches u |p| when it is worst and which the reference's own fp32 twin makes too; a bound
                of which that twin may use only half (tests/odometry_scenes.py asserts it) therefore takes it twice: b = 2.
     est[3:7] : two non-zero products per component and their sums, 4 u |q|, plus |q| (err(h c) + err(c)) -> err(h) + 8 u |q|_inf
     biases   : one fp32 product each, which nothing can fuse: exact, like prev and the zero words (bound 0: compared as values).
No count has seen the kernel's output."""
import numpy as np

import philox_np
from helpers import abi

TAG = abi.RNG_TAGS["odometry"]
FILL_ALL, RESETS_ONLY = abi.DEFINES["LSIM_SENSOR_FILL_ALL"], abi.DEFINES["LSIM_SENSOR_RESETS_ONLY"]
F = np.float32
U = 2.0 ** -24
RANGE_NAMES = ("scale_range", "yaw_range", "z_range", "pos_noise", "yaw_noise", "z_noise")
A_XY, A_Z, B_POS, B_QUAT = 13.0, 6.0, 2.0, 8.0


def visited_set(num_envs, env_stride):
    return np.arange(num_envs) % env_stride == 0


def fresh_set(num_envs, env_stride, flags, episode_length):
    return visited_set(num_envs, env_stride) & (bool(flags & FILL_ALL) | (np.asarray(episode_length) == 0))


def draws(seed, rank, envs, tick, stream_id, block):
    """s [len(envs), 3] float32, exact: words 0..2 of block `block` (the fourth word is not used)"""
    x = philox_np.philox4x32_10(np.asarray(envs, np.uint32), np.uint32(tick & 0xFFFFFFFF), np.uint32(TAG), np.uint32((stream_id << 16) | block), seed, rank)
    u = np.stack([(w >> np.uint32(8)).astype(F) * F(U) for w in x[:3]], axis=1)
    return (F(2.0) * u - F(1.0)).astype(F)


def rot(q, v):
    """R(q) v = v + 2 w (u x v) + 2 u x (u x v), xyzw rows, in the dtype of the arguments"""
    u, w = q[:3], q[3]
    t = np.cross(u, v)
    t = t + t
    return v + w * t + np.cross(u, t)


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + bw * ax + (ay * bz - az * by), aw * by + bw * ay + (az * bx - ax * bz),
                     aw * bz + bw * az + (ax * by - ay * bx), aw * bw - (ax * bx + ay * by + az * bz)], dtype=a.dtype)


def step(root_states, odo, est, episode_length, tick, flags, env_stride, seed, rank, stream_id, ranges, T=np.float64, mutant=None):
    """(odo', est') of one launch over copies of `odo` [N, 12] and `est` [N, 13] (dtype T); `ranges` in the order of RANGE_NAMES, fp32 values.
    `mutant`: one of "true_yaw", "redraw_bias", "prev_fixed", "fresh_keeps", "whole_angle" -- wrong on purpose"""
    rs = np.asarray(root_states, F)
    N = rs.shape[0]
    odo, est = np.array(odo, dtype=T), np.array(est, dtype=T)
    sr, yr, zr, pn, yn, zn = (T(F(v)) for v in ranges)
    fresh = fresh_set(N, env_stride, flags, episode_length)
    half, one = T(0.5), T(1.0)
    for e in np.nonzero(visited_set(N, env_stride))[0]:
        p = rs[e].astype(T)
        finite = bool(np.isfinite(rs[e, :7]).all())
        o = odo[e].copy()
        s_step = draws(seed, rank, [e], tick, stream_id, 0)[0].astype(T)
        s_epi = draws(seed, rank, [e], tick, stream_id, 1)[0].astype(T)
        if fresh[e] or mutant == "redraw_bias":
            o[4], o[5], o[6] = (T(F(s_epi[k]) * F(ranges[k])) for k in range(3))     # one fp32 product, stored: exact in either dtype
        if fresh[e]:
            if mutant != "fresh_keeps":
                o[0:4] = 0
            o[8:10] = p[0:2]
        elif finite:
            have = bool(np.isfinite(o[8:10]).all())
            D = (p[0:2] - o[8:10]) if have else np.zeros(2, T)
            L = np.sqrt(D[0] * D[0] + D[1] * D[1])
            h = o[3] + (one if mutant == "whole_angle" else half) * L * (o[5] + yn * s_step[0])
            c = one / np.sqrt(one + h * h)
            d = np.array([0, 0, h * c, c], T)
            r = rot(p[3:7] if mutant == "true_yaw" else d, np.array([D[0], D[1], 0], T))
            k = one + (o[4] + pn * s_step[1])
            o[0] = o[0] + (k * r[0] - D[0])
            o[1] = o[1] + (k * r[1] - D[1])
            o[2] = o[2] + L * (o[6] + zn * s_step[2])
            o[3] = h
            if mutant != "prev_fixed":
                o[8:10] = p[0:2]
        else:
            o[0:4] = 0
            o[8:10] = np.nan
        o[7] = o[10] = o[11] = 0
        odo[e] = o
        if finite:
            c = one / np.sqrt(one + o[3] * o[3])
            est[e, 0:3] = p[0:3] + o[0:3]
            est[e, 3:7] = qmul(np.array([0, 0, o[3] * c, c], T), p[3:7])
        else:
            est[e, 0:7] = p[0:7]
        est[e, 7:13] = p[7:13]
    return odo, est


def bounds(K, L_max, ranges, root_states):
    """(odo_tol [N, 12], est_tol [N, 13]) after K launches (module docstring); `root_states` the poses of the launch compared"""
    r = np.asarray([F(v) for v in ranges], np.float64)
    R = float(r.sum())
    assert K * R <= 1.0 and K * L_max <= 2.0, "the scene leaves the regime the bound is derived for"
    rs = np.asarray(root_states, np.float64)
    N = rs.shape[0]
    walk = K * L_max * (1.0 + R)
    odo, est = np.zeros((N, 12)), np.zeros((N, 13))
    odo[:, 0:2] = U * A_XY * walk
    odo[:, 2] = U * A_Z * walk
    odo[:, 3] = U * K * R * (3.0 * L_max + 1.0)
    pinf = np.abs(rs[:, 0:3]).max(axis=1)
    est[:, 0:2] = U * ((A_XY + 1.0) * walk + B_POS * pinf)[:, None]
    est[:, 2] = U * ((A_Z + 1.0) * walk + B_POS * pinf)
    est[:, 3:7] = (odo[:, 3] + U * B_QUAT * np.abs(rs[:, 3:7]).max(axis=1))[:, None]
    return odo, est
