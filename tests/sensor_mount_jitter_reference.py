"""TEST INFRASTRUCTURE -- numpy reference of the mount-jitter launch, written from the comment of lsim_sensor_mount_jitter in include/lsim.h
(not from the kernel source): which envs are fresh, the six draws, the position and the Cayley rotation composed with the nominal pose.

Exact parts.  u_k = (x_k >> 8) * 2^-24 and s_k = 2 u_k - 1 are exact in fp32 (s_k is a multiple of 2^-23 in [-1, 1)), and so is the set of
rows written: those are compared exactly.  A launch shows its draws exactly when it is given nominal = (0, 0, 0, 0, 0, 0, 1) and all six
ranges 1 (`draws_of`):  m[k] = 0 + s_k * 1 = s_k, k < 3; and with n = identity the product leaves d itself, m[3 + k] = fl(h_k c), m[6] = c,
h_k = s_{3+k} / 2 exactly, so 2 m[3 + k] / m[6] = s_{3+k} (1 + e), |e| < 2^-24, off s_{3+k} by less than 2^-24 -- half the spacing 2^-23 of
the grid s_{3+k} lies on, which rounding to that grid therefore recovers exactly.

Bounds.  Position and quaternion are evaluated here in fp64 from the fp32 inputs; the launch is fp32 with one rounding per operation (u = 2^-24
relative), a product and a sum possibly fused (fewer roundings, never more):
  position   m = n + s r: the product errs by <= u r, the sum by <= u (|n| + r (1 + u))            ->  pos_bound = 3 u (|n| + r)
  rotation   a_k = s r_k: 1 rounding; h_k = a_k / 2 exact; h_k^2: 2 u from a_k and 1 more; the three sums of positive terms, 1 + (..): 3 more
             -> the radicand is within 6 u; its correctly rounded root within 3 u + u; the correctly rounded quotient c = 1 / root within 5 u;
             d_k = h_k c: u (a_k) + 5 u + u = 7 u, d_w = c: 5 u                                    -> every component of d within 7 u, relatively
             m_quat: four products of a component of d and one of n, three sums (fused or not): the usual dot-product bound 4 u on
             sum |d_i n_j|, plus the 7 u carried in by d                                           -> 11 u sum |d_i| |n_j|
             with |d_k| <= r_k / 2 (k < 3), |d_w| <= 1 and the pairing of the Hamilton product.  quat_bound uses 12 u: the twelfth covers every
             second-order term ((1 + u)^11 - 1 < 11.001 u).
Neither bound has seen the kernel's output."""
import numpy as np

import philox_np
from helpers import abi

TAG = abi.RNG_TAGS["sensor_mount"]
FILL_ALL, RESETS_ONLY = abi.DEFINES["LSIM_SENSOR_FILL_ALL"], abi.DEFINES["LSIM_SENSOR_RESETS_ONLY"]
F = np.float32
U = 2.0 ** -24
IDENTITY_ROW = np.array([0, 0, 0, 0, 0, 0, 1], F)


def fresh_set(num_envs, env_stride, flags, episode_length):
    """[N] bool: the rows the launch writes"""
    e = np.arange(num_envs, dtype=np.int64)
    return (e % env_stride == 0) & (bool(flags & FILL_ALL) | (np.asarray(episode_length) == 0))


def draws(seed, rank, envs, tick, stream_id, swap_blocks=False):
    """s [len(envs), 6] float32, exact.  `swap_blocks`: the mutant that reads block 1 where the header says block 0 and the reverse"""
    e = np.asarray(envs, np.uint32)
    blocks = []
    for b in ((1, 0) if swap_blocks else (0, 1)):
        x = philox_np.philox4x32_10(e, np.uint32(tick & 0xFFFFFFFF), np.uint32(TAG), np.uint32((stream_id << 16) | b), seed, rank)
        blocks.append(np.stack([(w >> np.uint32(8)).astype(F) * F(U) for w in x], axis=1))
    u = np.concatenate(blocks, axis=1)[:, :6]
    return (F(2.0) * u - F(1.0)).astype(F)


def qmul(a, b):
    """Hamilton product of xyzw rows, R(a b) = R(a) R(b)"""
    ax, ay, az, aw = (a[..., k] for k in range(4))
    bx, by, bz, bw = (b[..., k] for k in range(4))
    return np.stack((aw * bx + bw * ax + (ay * bz - az * by), aw * by + bw * ay + (az * bx - ax * bz),
                     aw * bz + bw * az + (ax * by - ay * bx), aw * bw - (ax * bx + ay * by + az * bz)), axis=-1)


def delta(s_rot, rot_range):
    """d [.., 4] fp64 of the header: the Cayley map of a = s * rot_range"""
    h = 0.5 * (np.asarray(s_rot, np.float64) * np.asarray(rot_range, F).astype(np.float64))
    c = 1.0 / np.sqrt(1.0 + (h * h).sum(axis=-1, keepdims=True))
    return np.concatenate((h * c, c), axis=-1)


def rows(nominal, s, pos_range, rot_range, swap_product=False):
    """fp64 [len(s), 7]: the mount rows of the envs whose nominal rows and draws are given.  `swap_product`: the mutant n (x) d"""
    n = np.asarray(nominal, F).astype(np.float64)
    pos = n[:, :3] + s[:, :3].astype(np.float64) * np.asarray(pos_range, F).astype(np.float64)
    d = delta(s[:, 3:], rot_range)
    return np.concatenate((pos, qmul(n[:, 3:], d) if swap_product else qmul(d, n[:, 3:])), axis=1)


def bound(nominal, pos_range, rot_range):
    """[len(nominal), 7]: per output, the distance the launch may be from rows() (module docstring)"""
    n = np.abs(np.asarray(nominal, F).astype(np.float64))
    pr, rr = np.asarray(pos_range, F).astype(np.float64), np.asarray(rot_range, F).astype(np.float64)
    dx, dy, dz = rr / 2.0
    x, y, z, w = (n[:, 3 + k] for k in range(4))
    quat = np.stack((x + w * dx + (dy * z + dz * y), y + w * dy + (dz * x + dx * z), z + w * dz + (dx * y + dy * x), w + (dx * x + dy * y + dz * z)), axis=1)
    return np.concatenate((3.0 * U * (n[:, :3] + pr), 12.0 * U * quat), axis=1)


def expected(nominal, before, fresh, seed, rank, tick, stream_id, pos_range, rot_range, **mutant):
    """(want fp64 [N, 7], tol [N, 7]) of a launch over `before`: rows that are not fresh keep what they held (tol 0, compared as bits elsewhere)"""
    want, tol = np.asarray(before, F).astype(np.float64), np.zeros(np.shape(before))
    envs = np.nonzero(fresh)[0]
    s = draws(seed, rank, envs, tick, stream_id, swap_blocks=mutant.get("swap_blocks", False))
    want[envs] = rows(np.asarray(nominal)[envs], s, pos_range, rot_range, swap_product=mutant.get("swap_product", False))
    tol[envs] = bound(np.asarray(nominal)[envs], pos_range, rot_range)
    return want, tol


def draws_of(mount_rows):
    """the six s_k of rows a launch wrote from IDENTITY_ROW with all ranges 1, exactly (module docstring)"""
    m = np.asarray(mount_rows, F).astype(np.float64)
    s_rot = np.round(2.0 * m[:, 3:6] / m[:, 6:7] * 2.0 ** 23) / 2.0 ** 23
    return np.concatenate((m[:, :3], s_rot), axis=1).astype(F)


def angle(q):
    """rotation angle of xyzw rows, fp64, in [0, pi]"""
    q = np.asarray(q, np.float64)
    return 2.0 * np.arctan2(np.linalg.norm(q[..., :3], axis=-1), np.abs(q[..., 3]))


def nominal_rows(num_envs, seed=5):
    """per-env distinct poses with non-trivial unit quaternions (fp32 [N, 7]); no component is zero"""
    g = np.random.RandomState(seed)
    pos = g.uniform(-0.4, 0.4, (num_envs, 3))
    q = g.normal(size=(num_envs, 4))
    q[np.abs(q) < 0.05] = 0.05
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.concatenate((pos, q), axis=1).astype(F)
