"""Statements, plan restatements, case tables, scenes and bounds for the second half of csrc/ls_amp.h -- lsim_relu_head_backward and lsim_masked_colsum
(lsim_k_relu_cols<0 / 1> + lsim_k_wgrad_reduce), lsim_running_moments_update (lsim_k_moments_partial / _merge) and lsim_amp_pair_rows -- written from
include/lsim.h.  Everything here is numpy on the CPU.

  column kernels   fp64 statements; fp32 twins that add the rows forward, reversed and in the kernel's own order (row lane, the lanes through LDS,
                   the slices in the reduce kernel's order); exact scenes in small integers
  running moments  the parallel-variance merge in numpy longdouble with a two-pass batch variance (more precise than the device's one-pass float64),
                   a DERIVED bound on the device's distance from it, and a float64 twin in the kernel's order that has to stay inside that bound
  pair rows        a numpy float32 twin of the same operations: the learner's translation unit keeps IEEE division and square root, so bit for bit
"""
import zlib

import numpy as np

from wgrad_shapes_reference import padded  # noqa: F401

U = 2.0 ** -53
COLK_SLICES, COLK_N = 1024, (4, 8, 16, 32, 64, 128, 256, 512, 1024)
MOM_SLICES, MOM_MAX_DIM = 256, 64


def _seed(*key):
    return zlib.crc32("/".join(str(k) for k in key).encode()) & 0x7FFFFFFF


# ---------------------------------------------------------------------------------------------------------------------------------------
# lsim_relu_head_backward / lsim_masked_colsum
def colk_plan(batch, n):
    """ls_colk_plan restated; None where the library answers LSIM_E_UNSUPPORTED"""
    if batch <= 0 or n <= 0 or n % 4 or n > 1024 or 256 % (n // 4):
        return None
    rl = 256 // (n // 4)
    rps = (batch + COLK_SLICES - 1) // COLK_SLICES
    rps = max((rps + rl - 1) // rl * rl, 4 * rl)
    slices = (batch + rps - 1) // rps
    return dict(rl=rl, rps=rps, slices=slices, bytes=slices * (2 * n + 4) * 4, floor=rps == 4 * rl)


COLK_BIG = {4: 1048577, 64: 70001, 1024: 4097}          # batches at which the rows per slice leave their floor of 4 row lanes' passes


def colk_cases():
    out = []
    for n in COLK_N:
        rl = 256 // (n // 4)
        rps = 4 * rl
        for b in sorted({1, rl - 1, rl, rl + 1, rps - 1, rps, rps + 1} - {0}) + ([COLK_BIG[n]] if n in COLK_BIG else []):
            i = len(out)
            out.append(dict(name="n%d-b%d" % (n, b), n=n, batch=b, ld=n + 4 * (i % 3 != 0), ldv=n + 8 if i % 2 else n + 4, ldm=n + 4 if i % 2 else n + 12))
            if b > 5000:                  # a million rows: one padding quad per row
                out[-1].update(ld=n + 4, ldv=n + 4, ldm=n + 4)
    return out


COLK_CASES = {c["name"]: c for c in colk_cases()}


def colk_classes(c):
    p = colk_plan(c["batch"], c["n"])
    out = {"n%d" % c["n"], "rl%d" % p["rl"]}
    out |= {k for k, v in (("batch1", c["batch"] == 1), ("below_one_pass", c["batch"] < p["rl"]), ("one_pass", c["batch"] == p["rl"]),
                           ("last_slice_one_row", p["slices"] > 1 and c["batch"] % p["rps"] == 1), ("one_full_slice", c["batch"] == p["rps"]),
                           ("above_floor", not p["floor"]), ("ld>n", c["ld"] > c["n"]), ("ld=n", c["ld"] == c["n"]), ("ldv!=ldm", c["ldv"] != c["ldm"]),
                           ("slices_gt64", p["slices"] > 64)) if v}
    return out


COLK_CLASSES = ({"n%d" % n for n in COLK_N} | {"rl%d" % (256 // (n // 4)) for n in COLK_N}
                | {"batch1", "below_one_pass", "one_pass", "last_slice_one_row", "one_full_slice", "above_floor", "ld>n", "ld=n", "ldv!=ldm", "slices_gt64"})

RELU_VALUES = np.array([0.0, -0.0, 1.0, 2.0, 3.0], dtype=np.float32)
MASK_VALUES = np.array([0.0, -0.0, np.finfo(np.float32).tiny, -1.0, 1.0, 2.5], dtype=np.float32)


def head_scene(c, exact):
    """(relu_out [B, n], grad_d [B], head_weight [n]) float32.  Exact: small integers, |sums| <= 9 B < 2^24; +0.0 and -0.0 in relu_out"""
    rs = np.random.RandomState(_seed("head", c["name"], exact))
    B, n = c["batch"], c["n"]
    if exact:
        assert 9 * B < 2 ** 24
        a = RELU_VALUES[rs.randint(0, 5, size=(B, n))]
        a.reshape(-1)[:4] = [0.0, -0.0, 2.0, 3.0]
        return a, rs.randint(-3, 4, size=B).astype(np.float32), rs.randint(-3, 4, size=n).astype(np.float32)
    a = np.maximum(rs.randn(B, n), 0).astype(np.float32)
    a.reshape(-1)[:2] = [0.0, -0.0]
    return a, rs.randn(B).astype(np.float32), rs.randn(n).astype(np.float32)


def colsum_scene(c, exact):
    """(v [B, n], mask_src [B, n]) float32; v is NaN exactly where the mask is not positive: the kernel selects, it does not multiply"""
    rs = np.random.RandomState(_seed("colsum", c["name"], exact))
    B, n = c["batch"], c["n"]
    m = MASK_VALUES[rs.randint(0, 6, size=(B, n))]
    m.reshape(-1)[:4] = MASK_VALUES[:4]
    v = rs.randint(-3, 4, size=(B, n)).astype(np.float32) if exact else rs.randn(B, n).astype(np.float32)
    v[~(m > 0)] = np.nan
    return v, m


def head_reference(a, gd, w3):
    """dict(g2 fp32 [B, n]: one product per element; db2 [n], dhead [n + 4] fp64)"""
    g2 = np.where(a > 0, gd[:, None] * w3[None, :], np.float32(0)).astype(np.float32)
    dhead = np.zeros(a.shape[1] + 4)
    dhead[:a.shape[1]] = (a.astype(np.float64) * gd.astype(np.float64)[:, None]).sum(0)
    dhead[a.shape[1]] = gd.astype(np.float64).sum()
    return dict(g2=g2, db2=g2.astype(np.float64).sum(0), dhead=dhead)


def colsum_reference(v, m):
    return np.where(m > 0, v, 0.0).astype(np.float64).sum(0)


def reduce_order(part):
    """lsim_k_wgrad_reduce on part [slices, count] in fp32: slice group sl = w % 16 adds w = sl, sl + 16, ... with four accumulators over rounds of 64
    and the rest into the first, (s0 + s1) + (s2 + s3), then the 16 groups in order"""
    W, count = part.shape
    red = np.zeros((16, count), dtype=np.float32)
    for sl in range(16):
        s = [np.zeros(count, dtype=np.float32) for _ in range(4)]
        w = sl
        while w + 48 < W:
            for j in range(4):
                s[j] = s[j] + part[w + 16 * j]
            w += 64
        while w < W:
            s[0] = s[0] + part[w]
            w += 16
        red[sl] = (s[0] + s[1]) + (s[2] + s[3])
    t = np.zeros(count, dtype=np.float32)
    for k in range(16):
        t = t + red[k]
    return t


def colsum_twins(vals, c):
    """fp32 column sums of vals [B, cols] (the addends, already selected / multiplied in fp32): forward, reversed, and in the kernel's order"""
    p = colk_plan(c["batch"], c["n"])
    B, cols = vals.shape
    fwd = np.cumsum(vals, axis=0, dtype=np.float32)[-1]
    rev = np.cumsum(vals[::-1], axis=0, dtype=np.float32)[-1]
    pad = np.zeros((p["slices"] * p["rps"], cols), dtype=np.float32)
    pad[:B] = vals
    pad = pad.reshape(p["slices"], p["rps"] // p["rl"], p["rl"], cols)
    lanes = np.zeros((p["slices"], p["rl"], cols), dtype=np.float32)
    for j in range(pad.shape[1]):
        lanes = lanes + pad[:, j]
    part = lanes[:, 0].copy()
    for l in range(1, p["rl"]):
        part = part + lanes[:, l]
    return {"forward": fwd, "reversed": rev, "kernel": reduce_order(part)}


def twin_tolerance(vals, ref, c, label=None):
    """(tolerance, twin distance): 4 x the twins' largest distance from the fp64 sums, floored at 4 ulp of the output's scale"""
    dist = 0.0
    for name, tw in colsum_twins(vals, c).items():
        d = float(np.abs(tw.astype(np.float64) - ref).max())
        if label:
            print(label, c["name"], "twin", name, "distance", d)
        dist = max(dist, d)
    return max(4.0 * dist, 4.0 * 2.0 ** -23 * float(np.abs(ref).max())), dist


def head_addends(a, gd, ref):
    """the fp32 addends of (db2, dhead[:n], dhead[n]) as the kernel forms them"""
    return ref["g2"], (a * gd[:, None]).astype(np.float32), gd[:, None]


COLK_REFUSALS = ([("n = %d" % n, e, dict(n=n), "E_UNSUPPORTED") for n in (12, 20, 1028, 2048, 30) for e in ("head", "colsum")]
                 + [("ld % 4", "head", dict(ld=-2), "E_UNSUPPORTED"), ("ldv % 4", "colsum", dict(ldv=-2), "E_UNSUPPORTED"), ("ldm % 4", "colsum", dict(ldm=-2), "E_UNSUPPORTED"),
                    ("ld < n", "head", dict(ld=-36), "E_INVALID"), ("ldv < n", "colsum", dict(ldv=-36), "E_INVALID"), ("ldm < n", "colsum", dict(ldm=-36), "E_INVALID"),
                    ("batch 0", "head", dict(batch=0), "E_UNSUPPORTED"), ("batch 0", "colsum", dict(batch=0), "E_UNSUPPORTED")]
                 + [("%s %d bytes off" % (k, o), "head", dict(off={k: o}), "E_UNSUPPORTED") for k in ("relu_out", "grad_pre", "head_weight") for o in (4, 8)]
                 + [("%s %d bytes off" % (k, o), "colsum", dict(off={k: o}), "E_UNSUPPORTED") for k in ("v", "mask_src") for o in (4, 8)]
                 + [("workspace one byte short", e, dict(ws_short=1), "E_INVALID") for e in ("head", "colsum")]
                 + [("workspace %d bytes off" % o, e, dict(off={"workspace": o}), "E_INVALID") for e in ("head", "colsum") for o in (4, 8)]
                 + [("%s NULL" % k, "head", dict(null=k), "E_INVALID") for k in ("relu_out", "grad_d", "head_weight", "grad_pre", "grad_bias", "grad_head", "workspace")]
                 + [("%s NULL" % k, "colsum", dict(null=k), "E_INVALID") for k in ("v", "mask_src", "out", "workspace")])


def colk_refusal_call(L, entry, edits, address):
    """one refused call on a shape that is accepted unedited (batch 5, n 32, pitches 40, or n + 8 for a wider n); address(floats) -> 16-byte aligned NaN buffer.  Every buffer is
    large enough for an accepted call of the edited pitches with the pointer moved by up to 8 bytes"""
    n, batch = edits.get("n", 32), edits.get("batch", 5)
    ld = {k: max(40, n + 8) + edits.get(k, 0) for k in ("ld", "ldv", "ldm")}
    ws = colk_plan(max(batch, 1), 32)["bytes"]
    ptr = {k: address(8 * 2100) for k in ("relu_out", "grad_pre", "v", "mask_src")}
    ptr.update({k: address(2100) for k in ("grad_d", "head_weight", "grad_bias", "grad_head", "out")})
    ptr["workspace"] = address(ws // 4 + 4)
    for k, o in edits.get("off", {}).items():
        ptr[k] += o
    if "null" in edits:
        ptr[edits["null"]] = None
    if entry == "head":
        return L.lsim_relu_head_backward(ptr["relu_out"], ld["ld"], ptr["grad_d"], ptr["head_weight"], batch, n, ptr["grad_pre"], ptr["grad_bias"], ptr["grad_head"],
                                         ptr["workspace"], ws - edits.get("ws_short", 0), None)
    return L.lsim_masked_colsum(ptr["v"], ld["ldv"], ptr["mask_src"], ld["ldm"], batch, n, ptr["out"], ptr["workspace"], ws - edits.get("ws_short", 0), None)


# ---------------------------------------------------------------------------------------------------------------------------------------
# lsim_running_moments_update
def mom_plan(batch):
    rps = (batch + MOM_SLICES - 1) // MOM_SLICES
    rps = max((rps + 3) & ~3, 16)
    slices = (batch + rps - 1) // rps
    # the longest chain of additions one input passes through: its row lane's loop, the four lanes, a merge group's loop, the four groups
    depth = (rps + 3) // 4 + 3 + (slices + 3) // 4 + 3
    return dict(rps=rps, slices=slices, depth=depth, floor=rps == 16)


MOM_DIMS, MOM_BATCHES = (1, 30, 63, 64), (1, 3, 15, 16, 17, 4096, 4097, 70001)
MOM_STARTS = {"count0": 0.0, "default": 1e-4, "large": 3.0e7}
COLUMN_KINDS = ("o1", "offset1000", "const0.1", "const1234.567", "const98765.43")
CONSTANTS = {"const0.1": 0.1, "const1234.567": 1234.567, "const98765.43": 98765.43}
NORMALIZER_EPS = 1e-4


def mom_cases():
    out = []
    for i, dim in enumerate(MOM_DIMS):
        for j, batch in enumerate(MOM_BATCHES):
            start = list(MOM_STARTS)[(i + j) % 3]
            out.append(dict(name="d%d-b%d-%s" % (dim, batch, start), dim=dim, batch=batch, ldx=dim + (3 if (i + j) % 4 else 0) + (1 if dim == 1 else 0), start=start))
    return out


MOM_CASES = {c["name"]: c for c in mom_cases()}


def mom_scene(c):
    """three batches x [batch, dim] float32 (three updates in a row on one state), the start state (mean, var, count) float64, the kind of each column"""
    rs = np.random.RandomState(_seed("mom", c["name"]))
    kinds = [COLUMN_KINDS[(j + c["batch"]) % 5] for j in range(c["dim"])]
    xs = []
    for _ in range(3):
        x = np.empty((c["batch"], c["dim"]), dtype=np.float32)
        for j, k in enumerate(kinds):
            x[:, j] = rs.randn(c["batch"]) if k == "o1" else 1000.0 + 0.01 * rs.randn(c["batch"]) if k == "offset1000" else CONSTANTS[k]
        xs.append(x)
    cnt = MOM_STARTS[c["start"]]
    if c["start"] == "large":
        mean, var = 0.3 * rs.randn(c["dim"]), 0.5 + rs.rand(c["dim"])
    else:
        mean, var = np.zeros(c["dim"]), np.ones(c["dim"])            # the Normalizer's initial state
    return xs, (mean, var, np.array([cnt])), kinds


LD = np.longdouble


def mom_reference(x, state, err=None):
    """one update in longdouble with a corrected two-pass batch variance -> (state', err'): err = (mean bound, var bound) [dim] on the distance of the
    device's float64 path from this reference, given the bounds `err` on the incoming state.

    The bound, with u = 2^-53, n rows, D = mom_plan(n)['depth'] the longest chain of additions an input passes through, and q = sum t^2 / n the
    column's mean square (t * t is exact in float64 for a float32 t):
        batch mean      |fl(a) - a| <= D u sum |t| <= D u n sqrt(q) (Cauchy-Schwarz), one more u for the division:      em = (D + 1) u sqrt(q)
        batch variance  b / n is off by (D + 1) u q; mean^2 by 2 sqrt(q) em + u q; the subtraction rounds a result <= q:    ev = (3 D + 5) u q
                        -- the one-pass form's cancellation: on a constant column the variance IS this noise, of either sign
        merge           the bounds above and the incoming ones pass through the formula's partial derivatives; every product, quotient and sum
                        of the merge rounds once (8 u on the non-negative terms of m2, 4 u on the mean's terms)
    times 1.01 for the terms of second order."""
    assert np.finfo(LD).nmant >= 63, "numpy longdouble is not wider than float64 here"
    mean, var, cnt = (np.asarray(s, dtype=LD) for s in state)
    n = LD(x.shape[0])
    t = x.astype(LD)
    bmean = t.sum(0) / n
    d = t - bmean
    bvar = (d * d).sum(0) / n - (d.sum(0) / n) ** 2
    tot = cnt[0] + n
    delta = bmean - mean
    m2 = var * cnt[0] + bvar * n + delta * delta * cnt[0] * n / tot
    new = (mean + delta * n / tot, np.maximum(m2 / tot, 0), np.array([tot]))
    q = np.asarray((t * t).sum(0) / n, dtype=np.float64)
    D = mom_plan(x.shape[0])["depth"]
    em0, ev0 = (np.zeros_like(q), np.zeros_like(q)) if err is None else err
    em = (D + 1) * U * np.sqrt(q)
    ev = (3 * D + 5) * U * q
    w, wc = float(n / tot), float(cnt[0] / tot)
    ad = np.abs(np.asarray(delta, dtype=np.float64))
    dm = em + em0 + U * (np.abs(np.asarray(bmean, dtype=np.float64)) + np.abs(np.asarray(mean, dtype=np.float64)))
    mean_b = wc * em0 + w * dm + 4 * U * (np.abs(np.asarray(mean, dtype=np.float64)) + ad)
    var_b = wc * ev0 + w * ev + 2 * ad * wc * w * dm + 8 * U * np.asarray(m2 / tot, dtype=np.float64)
    return new, (1.01 * mean_b, 1.01 * var_b)


def mom_twin(x, state):
    """the device's arithmetic in numpy float64, in the kernel's order (no fused multiply-add; the clamp included)"""
    p = mom_plan(x.shape[0])
    B, dim = x.shape
    pad = np.zeros((p["slices"] * p["rps"], dim))
    pad[:B] = x
    pad = pad.reshape(p["slices"], p["rps"] // 4, 4, dim)
    la, lb = np.zeros((p["slices"], 4, dim)), np.zeros((p["slices"], 4, dim))
    for j in range(pad.shape[1]):
        la, lb = la + pad[:, j], lb + pad[:, j] * pad[:, j]
    pa, pb = la[:, 0].copy(), lb[:, 0].copy()
    for l in range(1, 4):
        pa, pb = pa + la[:, l], pb + lb[:, l]
    ga, gb = np.zeros((4, dim)), np.zeros((4, dim))
    for s in range(p["slices"]):
        ga[s % 4], gb[s % 4] = ga[s % 4] + pa[s], gb[s % 4] + pb[s]
    a, b = ga[0].copy(), gb[0].copy()
    for l in range(1, 4):
        a, b = a + ga[l], b + gb[l]
    mean, var, cnt = (np.asarray(s, dtype=np.float64) for s in state)
    n = float(B)
    tot = cnt[0] + n
    bmean = a / n
    bvar = b / n - bmean * bmean
    delta = bmean - mean
    m2 = var * cnt[0] + bvar * n + delta * delta * cnt[0] * n / tot
    merged = m2 / tot
    return (mean + delta * n / tot, np.where(merged < 0, 0.0, merged), np.array([tot])), bvar


# ---------------------------------------------------------------------------------------------------------------------------------------
# lsim_amp_pair_rows
PAIR_CLIP, PAIR_EPS = 10.0, 1e-4
PAIR_CASES = {"d%d-b%d" % (d, b): dict(name="d%d-b%d" % (d, b), dim=d, batch=b, lds=d + 3, ldn=d + 5, ldo=2 * d + 7)
              for d, b in [(d, b) for d in (1, 30, 32, 64) for b in (1, 5, 1025)] + [(64, 65600)]}


def pair_blocks(batch, dim):
    """(blocks launched, trips of the grid-stride loop a thread of block 0 takes)"""
    total = batch * 2 * dim
    blocks = min(max((total + 1023) // 1024, 1), 8192)
    return blocks, (total + blocks * 256 - 1) // (blocks * 256)


def pair_scene(c):
    """(states, next_states float32 [B, D], mean, var float64 [D]).  Column 0 has var + eps = 4 (a deviation of exactly 2) and mean 0.5: rows hold values
    exactly at, one float inside and far beyond +-clip"""
    rs = np.random.RandomState(_seed("pair", c["name"]))
    B, D = c["batch"], c["dim"]
    s, ns = (3.0 * rs.randn(B, D)).astype(np.float32), (3.0 * rs.randn(B, D)).astype(np.float32)
    mean, var = 0.3 * rs.randn(D), 0.5 + rs.rand(D)
    mean[0], var[0] = 0.5, 4.0 - PAIR_EPS
    hi = np.float32(0.5 + 2 * PAIR_CLIP)
    lo = np.float32(0.5 - 2 * PAIR_CLIP)
    edge = np.array([hi, np.nextafter(hi, np.float32(0)), 30.5, lo, np.nextafter(lo, np.float32(0)), -29.5], dtype=np.float32)
    r = np.arange(min(B, 6))
    s[r, 0], ns[r, 0] = edge[r % 6], edge[(r + 3) % 6]
    return s, ns, mean, var


def pair_sd(var, eps, sum_in_float32=False):
    return np.sqrt((var.astype(np.float32) + np.float32(eps)) if sum_in_float32 else (var + eps).astype(np.float32))


def pair_twin(s, ns, mean, var, eps=PAIR_EPS, clip=PAIR_CLIP, sum_in_float32=False):
    """[B, 2 D] float32: clamp((x - float32(mean)) / sqrt(float32(var + eps)), +-clip), the sum var + eps formed in float64 as the kernel does
    (sum_in_float32: the other reading, for the test that the choice shows)"""
    m = mean.astype(np.float32)
    sd = pair_sd(var, eps, sum_in_float32)
    assert sd.dtype == np.float32
    cl = np.float32(clip)
    f = lambda x: np.minimum(np.maximum((x - m) / sd, -cl), cl)
    out = np.concatenate([f(s), f(ns)], axis=1)
    assert out.dtype == np.float32
    return out
