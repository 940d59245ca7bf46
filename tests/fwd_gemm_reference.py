"""fp64 numpy statement of lsim_linear_elu_forward and lsim_linear_masked_forward (csrc/ls_gemm.h, lsim_k_linear_fwd<TM, TN, BK, VX, VW, ACT>), written
from include/lsim.h; a restatement of ls_linear_fwd_launch (tile config, tile counts, persistent blocks, the XCD partition and the list of tiles each
block walks, the vector class of the operand loads and what it was demoted from); a case table built FROM that plan as a function of the device's CU
count, so that its classes hold on any device; scene builders; the bound of the ELU epilogue's hardware exponential; and the mutants a test of this
kernel has to see.

Everything here is numpy on the CPU.  A case fixes the entry, the shape and HOW the operands lie in memory: x is a view `xo` floats into a 16-byte
aligned buffer with row pitch ldx > k_in, W starts `wo` floats into one, out and mask_src have pitches ldo / ldm >= n_out.
"""
import functools
import math
import zlib

import numpy as np

from wgrad_shapes_reference import EXTRA_ROWS, padded  # noqa: F401  (padded: the NaN-padded flat buffer of an operand view)

ENTRY = {"elu": "lsim_linear_elu_forward", "mask": "lsim_linear_masked_forward"}
BM, BK = 160, 32                                # TM = 5: 160 samples per tile; both configs stage K in chunks of 32 (LS_FWD_NARROW_BK = 32)
BN = {"narrow": 64, "wide": 128}                # TN = 2 for n_out <= 128, TN = 4 above


# ---------------------------------------------------------------------------------------------------------------------------------------
# the launch plan, restated
def vec_source(k_in, ldx, x_off, w_off):
    """(vx, vw): the widest loads each operand allows; offsets in floats from a 16-byte boundary"""
    vx = 2 if (ldx % 4 == 0 and k_in % 4 == 0 and x_off % 4 == 0) else 1 if (ldx % 2 == 0 and k_in % 2 == 0 and x_off % 2 == 0) else 0
    vw = 2 if (k_in % 4 == 0 and w_off % 4 == 0) else 1 if (k_in % 2 == 0 and w_off % 2 == 0) else 0
    return vx, vw


def grid_blocks(total, cus):
    blocks = max(8, (2 * cus) & ~7)
    return min(blocks, (total + 7) & ~7)


def plan(batch, k_in, n_out, ldx, x_off, w_off, cus):
    """None where the library refuses the shape"""
    if batch <= 0 or k_in <= 0 or n_out <= 0 or n_out % 4:
        return None
    config = "wide" if n_out > 128 else "narrow"
    n_tiles, m_tiles = (n_out + BN[config] - 1) // BN[config], (batch + BM - 1) // BM
    total = n_tiles * m_tiles
    blocks = grid_blocks(total, cus)
    per_xcd, stride = (total + 7) >> 3, blocks >> 3
    vx, vw = vec_source(k_in, ldx, x_off, w_off)
    launched = 2 if (vx == 2 and vw == 2) else 1 if (vx >= 1 and vw >= 1) else 0
    walks = []
    for b in range(blocks):
        xcd = b & 7
        last = min((xcd + 1) * per_xcd, total)
        walks.append(list(range(xcd * per_xcd + (b >> 3), last, stride)))
    return dict(config=config, bn=BN[config], n_tiles=n_tiles, m_tiles=m_tiles, total=total, blocks=blocks, per_xcd=per_xcd, stride=stride,
                chunks=(k_in + BK - 1) // BK, source=(vx, vw), launched=launched, walks=walks)


def case_plan(c, cus):
    return plan(c["batch"], c["k_in"], c["n_out"], c["ldx"], c["xo"], c["wo"], cus)


# ---------------------------------------------------------------------------------------------------------------------------------------
# cases
# how the operands lie: name -> (x offset, ldx as a function of k_in, W offset, the k_in residue it needs)
def _up4(v):
    return (v // 4 + 1) * 4


LAYOUTS = {
    "22":  dict(xo=4, ldx=_up4, wo=0, k="k % 4 == 0"),                                  # both operands in 16-byte loads
    "21":  dict(xo=4, ldx=_up4, wo=2, k="k % 4 == 0"),                                  # W 8 bytes off: LS_F(1, 1)
    "12":  dict(xo=0, ldx=lambda k: next(v for v in range(k + 1, k + 5) if v % 4 == 2), wo=0, k="k % 4 == 0"),
    "11":  dict(xo=0, ldx=lambda k: k + 2, wo=0, k="k % 4 == 2"),
    "x4":  dict(xo=1, ldx=_up4, wo=0, k="k % 4 == 0"),                                  # x 4 bytes off, W 16-byte aligned: LS_F(0, 0)
    "w4":  dict(xo=0, ldx=_up4, wo=1, k="k % 4 == 0"),                                  # W 4 bytes off, x 16-byte aligned: LS_F(0, 0)
    "odd": dict(xo=0, ldx=lambda k: k + 1, wo=0, k="k % 2 == 1"),
}
SOURCE_OF = {"22": (2, 2), "21": (2, 1), "12": (1, 2), "11": (1, 1), "x4": (0, 2), "w4": (2, 0), "odd": (0, 0)}
LAUNCHED_OF = {"22": 2, "21": 1, "12": 1, "11": 1, "x4": 0, "w4": 0, "odd": 0}

K_LIST = (1, 3, 4, 15, 16, 31, 32, 33, 34, 64, 65, 100)             # 33: the second chunk holds one k; 100: four chunks
N_LIST = {"narrow": (4, 12, 60, 64, 68, 128), "wide": (132, 256, 260, 388)}
BATCH_LIST = (1, 15, 16, 17, 159, 160, 161, 321)
SMALL_TOTALS = (1, 2, 3, 4, 5, 6, 7, 9, 12)
_K4_LAYOUTS = ("22", "21", "12", "x4", "w4")


def _case(act, k_in, n_out, batch, layout, bias=True, ldo_pad=4, ldm_pad=8, general=False, tag=""):
    lay = LAYOUTS[layout]
    assert eval(lay["k"], {"k": k_in}), (layout, k_in)
    c = dict(act=act, k_in=k_in, n_out=n_out, batch=batch, layout=layout, xo=lay["xo"], ldx=lay["ldx"](k_in), wo=lay["wo"], bias=bool(bias and act == "elu"),
             ldo=n_out + ldo_pad, ldm=(n_out + ldm_pad) if act == "mask" else 0, general=general)
    c["name"] = "%s-%dx%d-b%d-%s%s-o%d%s%s" % (act, k_in, n_out, batch, layout, "" if c["bias"] or act == "mask" else "-nobias", ldo_pad,
                                               "-m%d" % ldm_pad if act == "mask" else "", "-" + tag if tag else "")
    c["key"] = c["name"].replace("-b%d-" % batch, "-")          # the same on every device: the batch of a tile-count case follows the CU count
    return c


def _layout_for(k, i):
    return _K4_LAYOUTS[i % 5] if k % 4 == 0 else "11" if k % 4 == 2 else "odd"


def _shape_cases():
    """every k_in, batch and n_out of the lists under both tile configs and both epilogues; the five layouts that need k_in % 4 == 0 rotate over the
    five such k_in, so each (config, epilogue) meets each source class once"""
    out = []
    for ci, config in enumerate(("narrow", "wide")):
        for ai, act in enumerate(("elu", "mask")):
            s, k4 = 2 * ci + ai, 0
            for i, k in enumerate(K_LIST):
                if k % 4 == 0:
                    lay, k4 = _layout_for(k, k4 + s), k4 + 1
                else:
                    lay = _layout_for(k, 0)
                ns = N_LIST[config]
                out.append(_case(act, k, ns[(i + s) % len(ns)], BATCH_LIST[(i + 3 * s) % 8], lay, bias=(i + ci) % 2 == 0, ldo_pad=4 * ((i + s) % 3),
                                 ldm_pad=4 * ((i + s + 1) % 3), general=k in (3, 31, 34, 64, 100)))
    return out


def _shape_for_total(config, total):
    """(n_out, m_tiles) with n_tiles * m_tiles == total.  The wide config has at least two feature tiles: a total of 1 is out of its reach, a prime
    total takes that many feature tiles"""
    if config == "narrow":
        nt = 2 if total % 2 == 0 else 1
        return (68 if nt == 2 else 60), total // nt
    assert total >= 2
    nt = next(d for d in range(2, total + 1) if total % d == 0)
    if nt == 2 and total % 3 == 0 and total > 6:
        nt = 3
    if total == 12:
        nt = 4
    return 128 * (nt - 1) + 4, total // nt


def _tile_cases(cus):
    out = []
    rows = (1, 77, 160, 33)
    for ci, config in enumerate(("narrow", "wide")):
        for j, total in enumerate(SMALL_TOTALS):
            if config == "wide" and total == 1:
                continue
            n_out, mt = _shape_for_total(config, total)
            for act in (("elu", "mask") if total in (1, 2, 9) else (("elu", "mask")[(j + ci) % 2],)):
                out.append(_case(act, 5 if j % 2 else 34, n_out, (mt - 1) * BM + rows[j % 4], "odd" if j % 2 else "11", bias=j % 3 != 0, tag="t%d" % total))
        # the persistent walk: as many tiles as blocks, a few more (some blocks walk two tiles, their neighbours one, the last XCD has idle blocks),
        # and more than twice as many (three tiles), each with one chunk of K and with two
        B = max(8, (2 * cus) & ~7)
        for k, lay in ((5, "odd"), (34, "11")):
            for j, extra in enumerate((0, 2, 5 if config == "narrow" else 4, 8, B + 8)):
                total = B + extra
                act = ("elu", "mask")[(j + ci + (k == 34)) % 2]
                if config == "narrow":
                    nt = 2 if (total % 2 == 0 and extra in (0, 8)) else 1
                    n_out = 68 if nt == 2 else 4
                else:
                    nt, n_out = 2, 132
                    if extra == B + 8:
                        act = "elu"                  # 98 000 rows x 136 floats: one such array, not two
                mt = total // nt
                assert nt * mt == total
                out.append(_case(act, k, n_out, (mt - 1) * BM + rows[j % 4], lay, bias=j % 2 == 0, tag="walk+%s" % ("B+8" if extra == B + 8 else extra)))
    return out


@functools.lru_cache(maxsize=None)
def cases(cus):
    cs = _shape_cases() + _tile_cases(cus)
    out = {c["name"]: c for c in cs}
    assert len(out) == len(cs) == len({c["key"] for c in cs})
    return out


def by_key(cus):
    return {c["key"]: c for c in cases(cus).values()}


SHAPE_NAMES = [c["name"] for c in _shape_cases()]                # the same on every device
GENERAL = [c["name"] for c in _shape_cases() if c["general"]]


def classes():
    """what the table must reach on every device"""
    out = set()
    for config in ("narrow", "wide"):
        for act in ("elu", "mask"):
            ca = "%s/%s" % (config, act)
            out |= {"source:%s/%s" % (lay, ca) for lay in LAYOUTS} | {"launched:%d%d/%s" % (v, v, ca) for v in (0, 1, 2)}
            out |= {"k:%d/%s" % (k, ca) for k in K_LIST} | {"batch:%d/%s" % (b, ca) for b in BATCH_LIST} | {"n:%d/%s" % (n, ca) for n in N_LIST[config]}
            out |= {"ldx>k/" + ca, "nan_rows/" + ca, "ldo>n/" + ca, "ldo=n/" + ca}
        out |= {"bias/" + config, "bias_null/" + config, "ldm>n/" + config, "ldm=n/" + config, "chunks:4/" + config, "second_chunk_one_k/" + config}
        out |= {"total:%d/%s" % (t, config) for t in SMALL_TOTALS if not (config == "wide" and t == 1)}
        out |= {"idle_xcds:7/narrow", "xcd_short/" + config, "xcd_empty/" + config, "total=blocks/" + config}
        for ch in (1, 2):
            out |= {"%s/chunks%d/%s" % (w, ch, config) for w in ("walk2_beside_walk1", "walk2_and_idle_blocks", "walk3", "every_block_busy")}
        out |= {"walk/%s/%s" % (act, config) for act in ("elu", "mask")}
    return out


def case_classes(c, cus):
    p = case_plan(c, cus)
    config, act = p["config"], c["act"]
    ca = "%s/%s" % (config, act)
    assert p["source"] == SOURCE_OF[c["layout"]] and p["launched"] == LAUNCHED_OF[c["layout"]], c["name"]
    out = {"source:%s/%s" % (c["layout"], ca), "launched:%d%d/%s" % (p["launched"], p["launched"], ca), "k:%d/%s" % (c["k_in"], ca), "batch:%d/%s" % (c["batch"], ca),
           "n:%d/%s" % (c["n_out"], ca), "ldo>n/" + ca if c["ldo"] > c["n_out"] else "ldo=n/" + ca}
    if c["ldx"] > c["k_in"]:
        out |= {"ldx>k/" + ca, "nan_rows/" + ca}            # padded(): NaN behind every row and EXTRA_ROWS NaN rows behind the last
    if act == "elu":
        out.add(("bias/" if c["bias"] else "bias_null/") + config)
    else:
        out.add(("ldm>n/" if c["ldm"] > c["n_out"] else "ldm=n/") + config)
    if p["chunks"] == 4:
        out.add("chunks:4/" + config)
    if c["k_in"] % BK == 1 and p["chunks"] == 2:
        out.add("second_chunk_one_k/" + config)
    out.add("total:%d/%s" % (p["total"], config))
    if p["total"] == 1:
        out.add("idle_xcds:7/narrow")
    owned = [sum(len(w) for b, w in enumerate(p["walks"]) if b & 7 == x) for x in range(8)]
    assert sum(owned) == p["total"] and sorted(t for w in p["walks"] for t in w) == list(range(p["total"])), c["name"]
    if p["total"] >= 8 and any(0 < o < p["per_xcd"] for o in owned):
        out.add("xcd_short/" + config)
    if p["total"] >= 8 and min(owned) == 0:
        out.add("xcd_empty/" + config)
    full = max(8, (2 * cus) & ~7)
    if p["total"] == full:
        out.add("total=blocks/" + config)
    lens = [len(w) for w in p["walks"]]
    if p["total"] >= full and p["chunks"] <= 2:
        ch = "chunks%d/%s" % (p["chunks"], config)
        if max(lens) >= 2:
            out.add("walk/%s/%s" % (act, config))
        if any(lens[b] == 2 and lens[b + 8] == 1 for b in range(len(lens) - 8)):
            out.add("walk2_beside_walk1/" + ch)
        if max(lens) == 2 and min(lens) == 0:
            out.add("walk2_and_idle_blocks/" + ch)
        if max(lens) >= 3:
            out.add("walk3/" + ch)
        if min(lens) >= 1:
            out.add("every_block_busy/" + ch)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the ELU epilogue's exponential.  For x <= 0 the kernel forms  fl(v_exp_f32(fl(x * log2e_f32)) - 1).  Three terms, absolute:
#   1. the hardware 2^y is good to one ulp, and for y <= 0 its result is at most 1: one ulp there is 2^-24;
#   2. the argument: fl(x * log2e_f32) is off from x log2(e) by at most |x| log2(e) (2^-24 + r), r = the relative error of log2(e) as a float
#      (1.34e-8); d(2^y) = 2^y ln2 dy, so the result is off by e^x |x| (2^-24 + r) -- at most (2^-24 + r) * sup |x| e^x over the scene's range,
#      which is xmax e^-xmax below xmax = 1 and 1 / e from there on;
#   3. the subtraction rounds a result of magnitude at most 1: half an ulp, 2^-25.
LOG2E_F32_RELERR = abs(float(np.float32(math.log2(math.e))) - math.log2(math.e)) / math.log2(math.e)


def elu_exp_bound(xmax=np.inf):
    """absolute error bound of the kernel's elu(x) for -xmax <= x <= 0 given an exact x"""
    sup = xmax * math.exp(-xmax) if xmax < 1.0 else 1.0 / math.e
    return 2.0 ** -24 + (2.0 ** -24 + LOG2E_F32_RELERR) * sup + 2.0 ** -25


ELU_BOUND = elu_exp_bound()                     # 1.17e-7: what csrc/ls_gemm.h and include/lsim.h state as "1.2e-7"


# ---------------------------------------------------------------------------------------------------------------------------------------
# the reference
def _elu(pre):
    return np.where(pre > 0, pre, np.expm1(np.minimum(pre, 0)))


def reference(c, x, W, b, mask):
    """dict(pre, out) fp64 [batch, n_out]: elu(x W^T + b), or mask > 0 ? x W^T : 0"""
    pre = np.asarray(x, dtype=np.float64) @ np.asarray(W, dtype=np.float64).T
    if c["act"] == "elu":
        if b is not None:
            pre = pre + np.asarray(b, dtype=np.float64)
        return dict(pre=pre, out=_elu(pre))
    return dict(pre=pre, out=np.where(np.asarray(mask) > 0, pre, 0.0))


# ---------------------------------------------------------------------------------------------------------------------------------------
# mutants: what a subtly wrong kernel would store, through the restated tiles and walks
MUTANTS = {
    "k_past_K_as_data":      "values",   # k >= K read as data: the NaN behind a row's last column reaches every sum of a ragged chunk
    "bias_at_n_minus_n0":    "values",   # the bias quad taken at the column's index inside its tile
    "mask_pitch_n_out":      "values",   # the mask read with pitch n_out instead of ldm
    "out_pitch_n_out":       "values",   # the output stored with pitch n_out instead of ldo
    "mask_ge_0":             "values",
    "elu_on_positives":      "values",
    "tile_by_m_tiles":       "values",   # tile -> (m0, n0) by m_tiles instead of n_tiles
    "xcd_last_tile_dropped": "values",   # last = min(...) - 1
    "walk_keeps_m0":         "values",   # the second walked tile computed and stored at the first one's sample rows
    "half_chunk_dropped":    "values",   # k = 16 .. 31 of every chunk left out
    "rows_past_batch_as_data": "nothing: sample row m of the MFMA's B operand feeds accumulator column m alone, and columns m >= batch are never stored; the "
                               "clamped address (row batch - 1) is what keeps the load inside the buffer, and the NaN rows behind the batch prove the store mask",
}


def _tile_values(c, p, x, W, b, mask_flat, rows0, rows_rest, cols, mask_rows, mutant):
    """one macro tile as the kernel forms it: chunk 0 from sample rows `rows0`, later chunks from `rows_rest` (they differ under walk_keeps_m0 only),
    feature columns `cols`, the mask read at `mask_rows`; rows and columns outside the problem are dropped by the caller"""
    K = c["k_in"]
    ks = np.arange(K)
    if mutant == "half_chunk_dropped":
        ks = ks[ks % BK < 16]
    k0 = ks[ks < BK]
    pre = x[rows0][:, k0] @ W[cols][:, k0].T
    k1 = ks[ks >= BK]
    if k1.size:
        pre = pre + x[rows_rest][:, k1] @ W[cols][:, k1].T
    if mutant == "k_past_K_as_data" and K % BK:
        pre = pre + np.nan
    if c["act"] == "elu":
        if b is not None:
            pre = pre + (b[cols - cols[0]] if mutant == "bias_at_n_minus_n0" else b[cols])
        if mutant == "elu_on_positives":
            with np.errstate(over="ignore"):
                return np.expm1(pre)
        return _elu(pre)
    pitch = c["n_out"] if mutant == "mask_pitch_n_out" else c["ldm"]
    mk = mask_flat[mask_rows[:, None] * pitch + cols[None, :]]
    with np.errstate(invalid="ignore"):
        keep = mk >= 0 if mutant == "mask_ge_0" else mk > 0
    return np.where(keep, pre, 0.0)


def structured(c, cus, x, W, b, mask, mutant=None):
    """the flat output buffer [batch * ldo] (fp64; NaN where nothing is stored) formed block by block and tile by tile from the restated plan.
    Without a mutant its columns < n_out equal reference() and the rest is NaN"""
    p = case_plan(c, cus)
    M, N, bn = c["batch"], c["n_out"], p["bn"]
    x, W = np.vstack([np.asarray(x, dtype=np.float64), np.zeros((1, c["k_in"]))]), np.asarray(W, dtype=np.float64)      # row M: what a row >= batch reads as
    b = None if b is None else np.asarray(b, dtype=np.float64)
    mask_flat = None if mask is None else padded(mask, 0, c["ldm"])
    out = np.full(M * c["ldo"], np.nan)
    opitch = N if mutant == "out_pitch_n_out" else c["ldo"]
    div = p["m_tiles"] if mutant == "tile_by_m_tiles" else p["n_tiles"]
    per_tile = mutant in ("tile_by_m_tiles", "walk_keeps_m0", "bias_at_n_minus_n0")
    if not per_tile:
        # every tile is formed from its own rows and columns: one product for the whole problem, stored tile by tile below
        rows, cols = np.arange(M), np.arange(N)
        full = _tile_values(c, p, x, W, b, mask_flat, rows, rows, cols, rows, mutant)
    for walk in p["walks"]:
        m_first = None
        for i, t in enumerate(walk):
            if mutant == "xcd_last_tile_dropped" and ((t + 1) % p["per_xcd"] == 0 or t == p["total"] - 1):
                continue
            m0, n0 = (t // div) * BM, (t % div) * bn
            if m_first is None:
                m_first = m0
            ms = m_first if (mutant == "walk_keeps_m0" and i > 0) else m0            # where the tile is stored and where later chunks are read
            rows_store = np.arange(ms, min(ms + BM, M))
            cols = np.arange(n0, min(n0 + bn, N))
            if rows_store.size == 0 or cols.size == 0:
                continue
            if per_tile:
                rows0 = np.minimum(np.arange(m0, m0 + rows_store.size), M)
                vals = _tile_values(c, p, x, W, b, mask_flat, rows0, rows_store, cols, rows_store, mutant)
            else:
                vals = full[rows_store[0]:rows_store[-1] + 1, n0:n0 + cols.size]
            out[rows_store[:, None] * opitch + cols[None, :]] = vals
    return out


def expected_flat(c, ref_out):
    out = np.full((c["batch"], c["ldo"]), np.nan)
    out[:, :c["n_out"]] = ref_out
    return out.reshape(-1)


def mutant_touches(mutant, c, cus):
    p = case_plan(c, cus)
    if mutant == "k_past_K_as_data":
        return c["k_in"] % BK != 0 and c["ldx"] > c["k_in"]
    if mutant == "bias_at_n_minus_n0":
        return c["bias"] and p["n_tiles"] > 1
    if mutant == "mask_pitch_n_out":
        return c["act"] == "mask" and c["ldm"] > c["n_out"] and c["batch"] > 1
    if mutant == "out_pitch_n_out":
        return c["ldo"] > c["n_out"] and c["batch"] > 1
    if mutant == "mask_ge_0":
        return c["act"] == "mask"
    if mutant == "elu_on_positives":
        return c["act"] == "elu"
    if mutant == "tile_by_m_tiles":
        return p["m_tiles"] != p["n_tiles"]
    if mutant == "walk_keeps_m0":
        return any(t // p["n_tiles"] != w[0] // p["n_tiles"] for w in p["walks"] for t in w[1:])
    if mutant == "half_chunk_dropped":
        return c["k_in"] > 16
    return mutant in ("xcd_last_tile_dropped", "rows_past_batch_as_data")


def differs(a, b, tol):
    """is flat output `a` farther than tol from `b` somewhere -- a NaN on one side only counts as far"""
    na, nb = np.isnan(a), np.isnan(b)
    if (na != nb).any():
        return True
    both = ~na
    return bool((np.abs(a[both] - b[both]) > tol).any())


# ---------------------------------------------------------------------------------------------------------------------------------------
# scenes
def _seed(c, salt):
    return zlib.crc32(("%s/%s" % (c["name"], salt)).encode()) & 0x7FFFFFFF


MASK_VALUES = np.array([0.0, -0.0, np.finfo(np.float32).tiny, -1.0, -np.finfo(np.float32).tiny, 1.0, 2.5], dtype=np.float32)


def exact_scene(c):
    """(x, W, b or None, mask or None) float32, all small integers, sum_k |W||x| + |b| < 2^24: every partial sum in any order is exact in fp32.
    Row 0 of x is -3 throughout; weight row 0 is all -1 (pre-activation 3 k_in + b >= 1: positive, and where the mask scene holds its +0.0); weight rows
    n % 8 == 1 are all 12 (row 0: -36 k_in <= -36, the ELU saturates to exactly -1); weight row 2 is all twos (where the mask scene holds the
    smallest positive normal: a kept, non-zero product in a scene of one row and four columns); weight rows n % 8 == 3 are zero, as is their bias
    (a pre-activation of exactly 0)"""
    rs = np.random.RandomState(_seed(c, "exact"))
    x = rs.randint(-3, 4, size=(c["batch"], c["k_in"])).astype(np.float32)
    W = rs.randint(-3, 4, size=(c["n_out"], c["k_in"])).astype(np.float32)
    x[0] = -3.0
    n = np.arange(c["n_out"])
    W[n % 8 == 1] = 12.0
    W[n % 8 == 3] = 0.0
    W[0], W[2] = -1.0, 2.0
    b = mask = None
    if c["bias"]:
        b = rs.randint(-2, 3, size=c["n_out"]).astype(np.float32)
        b[n % 8 == 3] = 0.0
    if c["act"] == "mask":
        mask = MASK_VALUES[rs.randint(0, len(MASK_VALUES), size=(c["batch"], c["n_out"]))]
        mask.reshape(-1)[:4] = MASK_VALUES[:4]            # +0.0 at [0, 0], -0.0, the smallest positive normal, a negative: in the smallest scene too
    bound = float((np.abs(x).astype(np.float64) @ np.abs(W).astype(np.float64).T).max() + (np.abs(b).max() if b is not None else 0.0))
    assert bound < 2 ** 24, (c["name"], bound)
    return x, W, b, mask


def general_scene(c):
    rs = np.random.RandomState(_seed(c, "general"))
    x = rs.randn(c["batch"], c["k_in"]).astype(np.float32)
    W = (rs.randn(c["n_out"], c["k_in"]) / math.sqrt(c["k_in"])).astype(np.float32)
    b = (0.1 * rs.randn(c["n_out"])).astype(np.float32) if c["bias"] else None
    mask = np.maximum(rs.randn(c["batch"], c["n_out"]), 0).astype(np.float32) if c["act"] == "mask" else None
    return x, W, b, mask


TWIN_ROWS = 256


def _k_orders(K):
    """the three orders in which the twins add the products of one output"""
    kernel = []
    for h0 in range(0, ((K + 15) // 16) * 16, 16):           # 16-wide sub-chunk; MFMA step s takes k = h0 + 4 q + s of the four lane groups q
        kernel += [h0 + 4 * q + s for s in range(4) for q in range(4)]
    return {"forward": list(range(K)), "reversed": list(range(K - 1, -1, -1)), "kernel16": [k for k in kernel if k < K]}


def twin(c, x, W, b, mask, order):
    """the entry in np.float32, one accumulator per output, the products added in `order`, exp(x) - 1 as the kernel (and torch) write the ELU"""
    acc = np.zeros((x.shape[0], W.shape[0]), dtype=np.float32)
    for k in order:
        acc += x[:, k, None] * W[None, :, k]
    if c["act"] == "mask":
        return np.where(mask > 0, acc, np.float32(0))
    if b is not None:
        acc = acc + b
    return np.where(acc > 0, acc, np.exp(np.minimum(acc, np.float32(0))) - np.float32(1))


def tolerance(c, x, W, b, mask, label=None):
    """dict(ref, tol [batch, n_out], twin_dist, base): 4 x the twins' largest distance from the fp64 statement (on the first TWIN_ROWS rows), floored
    at 4 ulp of the output's scale, plus the exponential's bound where the statement's pre-activation is <= 0 (ELU)"""
    ref = reference(c, x, W, b, mask)
    T = min(TWIN_ROWS, c["batch"])
    dist = 0.0
    for name, order in _k_orders(c["k_in"]).items():
        tw = twin(c, x[:T], W, b, None if mask is None else mask[:T], order)
        d = float(np.abs(tw.astype(np.float64) - ref["out"][:T]).max())
        if label:
            print(label, c["name"], "twin", name, "distance", d)
        dist = max(dist, d)
    scale = float(np.abs(ref["out"]).max())
    base = max(4.0 * dist, 4.0 * 2.0 ** -23 * scale)
    tol = np.full(ref["out"].shape, base)
    if c["act"] == "elu":
        tol = tol + np.where(ref["pre"] <= 0, ELU_BOUND, 0.0)
    return dict(ref=ref, tol=tol, twin_dist=dist, base=base, scale=scale)


@functools.lru_cache(maxsize=None)
def general_case(name):
    c = cases(256)[name]
    sc = general_scene(c)
    return dict(scene=sc, **tolerance(c, *sc, label="fwd"))


# ---------------------------------------------------------------------------------------------------------------------------------------
# refusals: (name, entry, edits of an accepted call, code)
REFUSAL_SHAPE = dict(batch=5, k_in=8, n_out=8)
REFUSALS = [
    ("x NULL", "elu", dict(null="x"), "E_INVALID"), ("weight NULL", "elu", dict(null="w"), "E_INVALID"), ("out NULL", "elu", dict(null="out"), "E_INVALID"),
    ("x NULL", "mask", dict(null="x"), "E_INVALID"), ("weight NULL", "mask", dict(null="w"), "E_INVALID"), ("out NULL", "mask", dict(null="out"), "E_INVALID"),
    ("mask_src NULL", "mask", dict(null="mask"), "E_INVALID"),
    ("ldx < k_in", "elu", dict(ldx=7), "E_INVALID"), ("ldx < k_in", "mask", dict(ldx=7), "E_INVALID"),
    ("ldo < n_out", "elu", dict(ldo=4), "E_INVALID"), ("ldo < n_out", "mask", dict(ldo=4), "E_INVALID"),
    ("ldm < n_out", "mask", dict(ldm=4), "E_INVALID"),
    ("n_out % 4", "elu", dict(n_out=6), "E_UNSUPPORTED"), ("n_out % 4", "mask", dict(n_out=6), "E_UNSUPPORTED"),
    ("ldo % 4", "elu", dict(ldo=10), "E_UNSUPPORTED"), ("ldo % 4", "mask", dict(ldo=10), "E_UNSUPPORTED"),
    ("ldm % 4", "mask", dict(ldm=10), "E_UNSUPPORTED"),
    ("out 4 bytes off", "elu", dict(out_off=4), "E_UNSUPPORTED"), ("out 8 bytes off", "mask", dict(out_off=8), "E_UNSUPPORTED"),
    ("mask_src 4 bytes off", "mask", dict(mask_off=4), "E_UNSUPPORTED"), ("mask_src 8 bytes off", "mask", dict(mask_off=8), "E_UNSUPPORTED"),
    ("batch 0", "elu", dict(batch=0), "E_UNSUPPORTED"), ("batch -1", "mask", dict(batch=-1), "E_UNSUPPORTED"),
    ("k_in 0", "elu", dict(k_in=0), "E_UNSUPPORTED"),
]


def refusal_call(L, entry, edits, address):
    """the return code of one refused call; address(floats) -> a 16-byte aligned NaN-filled buffer of that many floats"""
    s = dict(REFUSAL_SHAPE, ldx=12, ldo=12, ldm=12)
    s.update({k: v for k, v in edits.items() if k in s})
    rows = max(s["batch"], 1) + 1
    ptr = dict(x=address(rows * 16), w=address(16 * 16), bias=address(16), mask=address(rows * 16), out=address(rows * 16))
    ptr["out"] += edits.get("out_off", 0)
    ptr["mask"] += edits.get("mask_off", 0)
    if "null" in edits:
        ptr[edits["null"]] = None
    if entry == "elu":
        return L.lsim_linear_elu_forward(ptr["x"], s["ldx"], ptr["w"], ptr["bias"], s["batch"], s["k_in"], s["n_out"], ptr["out"], s["ldo"], None)
    return L.lsim_linear_masked_forward(ptr["x"], s["ldx"], ptr["w"], ptr["mask"], s["ldm"], s["batch"], s["k_in"], s["n_out"], ptr["out"], s["ldo"], None)
