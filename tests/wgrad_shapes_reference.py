"""fp64 numpy statement of the weight-gradient family of csrc/ls_learn.h -- lsim_linear_wgrad, lsim_linear_elu_wgrad, lsim_linear_relu_wgrad, their
_deferred forms and lsim_wgrad_reduce_batch -- written from include/lsim.h; a restatement of the launch plan (single-wave or tiled, rows per
partial, the four waves' quarters of a slice, the vector classes of the operand loads, what the steady loop hands to the guarded loop) so that a
CPU test can assert that the case table reaches every path; the case table; the scene builders; and the mutants a test of these kernels has to see.

Everything here is numpy on the CPU.  A case fixes the shape, the batch, the entry and HOW its operands lie in memory: the column offset of the
view into a 16-byte aligned buffer and the row pitch, which is what selects the kernel's <VX, VG> instantiation.
"""
import functools
import zlib

import numpy as np

import mlp_shapes_reference as M

ENTRY = {"plain": "lsim_linear_wgrad", "elu": "lsim_linear_elu_wgrad", "relu": "lsim_linear_relu_wgrad"}
ZOFF = {"elu": 1.0, "relu": 0.0}
EXTRA_ROWS = 3                    # NaN rows behind the batch's last row, inside the same buffer
MAX_WEIGHTS = 140000
REDUCE_BATCH = 24                 # LS_REDUCE_BATCH: items per launch of lsim_wgrad_reduce_batch


# ---------------------------------------------------------------------------------------------------------------------------------------
# the launch plan, restated (ls_wgrad_plan, ls_wgrad_workspace_bytes, the row split of both kernels, ls_wgrad_tile_loop3's loop bounds)
def plan(batch, k_in, n_out):
    """None where the library answers LSIM_E_UNSUPPORTED"""
    count = k_in * n_out
    if batch <= 0 or k_in <= 0 or n_out <= 0 or count > MAX_WEIGHTS:
        return None
    nt, kt = (n_out + 15) // 16, (k_in + 15) // 16
    if nt <= 8 and kt <= 8 and nt * kt <= 32 and count <= 4096:
        rows = max(16, ((batch + 1023) // 1024 + 3) & ~3)
        p = dict(small=True, nt=nt, kt=kt, kg=0, rows=rows, n_blocks=1, k_blocks=1)
    else:
        n_blocks = (n_out + 63) // 64
        k_blocks = 1 if k_in <= 64 else (k_in + 127) // 128
        slices = max(1, min(512 // (n_blocks * k_blocks), (32 << 20) // (count * 4)))
        rows = max(64, ((batch + slices - 1) // slices + 15) & ~15)
        p = dict(small=False, nt=nt, kt=kt, kg=1 if k_in <= 64 else 2, rows=rows, n_blocks=n_blocks, k_blocks=k_blocks)
    p["partials"] = (batch + p["rows"] - 1) // p["rows"]
    p["bytes"] = p["partials"] * (count + n_out) * 4
    p["tiles"] = p["n_blocks"] * p["k_blocks"]
    p["blocks"] = (p["partials"] + 3) // 4 if p["small"] else p["tiles"] * p["partials"]
    return p


def quarter(rows):
    """rows per wave of a slice of `rows` rows"""
    return ((rows + 3) // 4 + 3) & ~3


def waves(p, batch):
    """[(partial, b0, b1)]: the batch rows each wave owns.  Single-wave kernel: one wave per partial; tiled: four per partial"""
    out = []
    for s in range(p["partials"]):
        s0, s1 = s * p["rows"], min((s + 1) * p["rows"], batch)
        if p["small"]:
            out.append((s, s0, s1))
            continue
        q = quarter(s1 - s0)
        out.extend((s, min(s0 + w * q, s1), min(s0 + (w + 1) * q, s1)) for w in range(4))
    return out


def loop3(rows):
    """(rounds of the steady loop, rows it and its two trailing steps consume); the rest goes to the guarded loop"""
    if rows < 20:
        return 0, 0
    rounds = (rows - 20) // 12 + 1
    return rounds, 12 * rounds + 8


def xcd_order(total):
    """the tiled kernel's block renumbering: block id -> v"""
    return [(b & 7) * (total >> 3) + min(b & 7, total & 7) + (b >> 3) for b in range(total)]


def vec_class(off, ld, pairs=True):
    """2: 16-byte loads, 1: 8-byte loads (x only), 0: scalars -- for a view `off` floats into a 16-byte aligned buffer with row pitch ld"""
    if ld % 4 == 0 and off % 4 == 0:
        return 2
    return 1 if pairs and ld % 2 == 0 and off % 2 == 0 else 0


def layout(code, width):
    """(column offset, row pitch) of a view: the pitch is always wider than the width"""
    r4 = (width // 4 + 1) * 4
    odd = width + 1 if width % 2 == 0 else width + 2
    r2 = next(v for v in range(width + 1, width + 5) if v % 4 == 2)
    return {"2": (4, r4), "1": (2, r2), "1p": (2, r4), "0": (3, odd), "0p": (1, r4), "0h": (2, r2)}[code]


# ---------------------------------------------------------------------------------------------------------------------------------------
# cases
def _case(entry, k_in, n_out, batch, x="2", g="2", z="2", gy=True, db=True, dw_off=0, general=False):
    fz = entry != "plain"
    c = dict(entry=entry, k_in=k_in, n_out=n_out, batch=batch, fz=fz, gy=bool(fz and gy), db=db, dw_off=dw_off, general=general)
    (c["xo"], c["ldx"]), (c["go"], c["ldg"]) = layout(x, k_in), layout(g, n_out)
    c["zo"], c["ldz"] = layout(z, n_out) if fz else (0, 0)
    c["name"] = "%s-%dx%d-b%d-x%s-g%s%s%s%s%s" % (entry, k_in, n_out, batch, x, g, "-z" + z if fz else "", "" if c["gy"] or not fz else "-nogy",
                                                "" if db else "-nodb", "-dw+%d" % dw_off if dw_off else "")
    return c


def sw_pairs():
    """the (NT, KT) the single-wave plan can reach: at most 8 each, 32 together, and the narrowest widths of the pair within 4096 weights"""
    return [(nt, kt) for nt in range(1, 9) for kt in range(1, 9) if nt * kt <= 32 and (16 * (nt - 1) + 1) * (16 * (kt - 1) + 1) <= 4096]


_SW_RN = (1, 16, 5, 11, 8, 13, 3, 16, 1, 7)
_SW_RK = (16, 1, 9, 4, 14, 1, 16, 6, 12, 2)
_SW_BATCH = (1, 7, 19, 1100, 37, 16, 150, 4099)      # 1100: 69 partials; 37: three partials, one padding wave; 4099: 16-row waves and a 3-row one
_SW_X = ("2", "1", "0", "0p", "1p")


def _sw_cases():
    out = []
    for i, (nt, kt) in enumerate(sw_pairs()):
        rn, rk = _SW_RN[i % 10], _SW_RK[(3 * i) % 10]
        while (16 * (nt - 1) + rn) * (16 * (kt - 1) + rk) > 4096:
            rn, rk = (rn, rk - 1) if rk > 1 else (rn - 1, rk)
        out.append(_case("plain", 16 * (kt - 1) + rk, 16 * (nt - 1) + rn, _SW_BATCH[i % 8], x=_SW_X[i % 5], g=_SW_X[(i + 2) % 5],
                         db=i % 7 != 3, dw_off=1 if i % 6 == 2 else 0, general=i in (3, 30)))
    # a wave that runs a full 16-row round AND a ragged tail needs more than 16 rows per wave: more than 16 384 rows
    out.append(_case("plain", 19, 12, 16999, x="0", g="0"))
    return out


def _tiled_cases():
    P, E, Rl = "plain", "elu", "relu"
    return [
        # ---- 128-wide k tiles (KG = 2)
        _case(P, 512, 256, 2555),                                                   # interior tiles only; quarter 20
        _case(E, 512, 256, 4091, dw_off=1, general=True),                           # the update's shape; quarter 32: two rounds
        _case(Rl, 512, 256, 3067, x="1p"),                                          # quarter 24: four rows handed over
        _case(E, 512, 256, 3579, x="0p", g="0p"),                                   # quarter 28: eight rows handed over
        _case(P, 238, 512, 2555, x="1"),                                            # edge k tile with a live, partial second group
        _case(E, 238, 512, 4091, x="1", g="0", z="0", general=True),
        _case(Rl, 238, 512, 2555, x="0"),
        _case(P, 238, 512, 3067, x="0", g="0"),
        _case(P, 130, 260, 4075, g="0"),                                            # dead second k group; edge n tile of one vector
        _case(E, 130, 260, 6523, z="0p"),                                           # g aligned, z not: VG 0
        _case(Rl, 130, 260, 4891, gy=False),
        _case(P, 270, 128, 6795, x="1"),                                            # six tiles, 510 blocks: the renumbering's ragged XCDs
        _case(E, 270, 128, 10875, x="1p", general=True),
        _case(P, 270, 128, 3, x="1", g="0"),                                        # one slice of three rows: waves 1-3 own nothing
        _case(P, 700, 200, 1675, x="0", db=False),
        _case(Rl, 700, 200, 2683, x="1", g="0h"),
        _case(E, 130, 262, 4075),                                                   # n_out % 4 != 0: scalar grad_pre store, loop3 skipped where it is written
        _case(Rl, 130, 262, 6523, x="0", g="0", z="0", general=True),
        _case(E, 130, 262, 5707, gy=False),                                         # the same edge tiles through loop3
        _case(E, 238, 510, 3067, x="0"),
        _case(P, 238, 510, 2555, x="1", g="0"),
        _case(E, 66, 68, 777, x="1", g="0", z="0"),                                 # two tiles, 256 slices: quarter 16 at any test-sized batch
        _case(Rl, 66, 68, 1, x="2", z="0h", db=False),
        _case(P, 66, 68, 130, x="0", g="2", dw_off=1),
        # ---- 64-wide k tiles (KG = 1)
        _case(P, 64, 512, 5115),
        _case(E, 64, 512, 8187, general=True),
        _case(Rl, 64, 512, 6139, x="1p", g="0p"),
        _case(P, 64, 512, 7163, x="0p"),
        _case(P, 60, 1024, 2555, x="1", g="0"),                                     # every tile an edge k tile
        _case(E, 60, 1024, 4091, x="0"),
        _case(Rl, 60, 1024, 2555, db=False),
        _case(E, 60, 1022, 4091, g="0", general=True),
        _case(Rl, 60, 1022, 3067, x="1"),
        _case(P, 60, 1022, 2555, x="0", g="0"),
        _case(P, 3, 1400, 1835),                                                    # k_in < 4: the clamped vector start is column 0
        _case(E, 3, 1400, 2939, x="1"),
        _case(Rl, 3, 1400, 1835, x="0", g="0", z="0"),
        _case(P, 1, 4100, 555, x="1"),
        _case(E, 1, 4100, 891, x="0", z="0p"),
        _case(Rl, 1, 4100, 555, g="0", general=True),
        _case(P, 64, 80, 100, g="0"),
        _case(E, 64, 512, 3),
        _case(Rl, 3, 1400, 1, x="1"),
    ]


CASES = {c["name"]: c for c in _sw_cases() + _tiled_cases()}
GENERAL = [n for n, c in CASES.items() if c["general"]]

_KINDS = ("interior", "edge_n_vec", "edge_n_scalar", "edge_k", "edge_k_dead", "k_lt4")
CLASSES = (
    {"sw<%d,%d>" % p for p in sw_pairs()}
    | {"sw_rn1", "sw_rn16", "sw_rk1", "sw_rk16", "sw_batch1", "sw_batch_lt16", "sw_round_and_ragged_wave", "sw_round_then_tail_in_one_wave",
       "sw_partials_gt64", "sw_padding_waves", "sw_db_null"}
    | {"tiled<%d,%d,%d,%d>" % (vx, vg, kg, fz) for vx in (0, 1, 2) for vg in (0, 2) for kg in (1, 2) for fz in (0, 1)}
    | {"%s_kg%d" % (e, kg) for e in ("elu", "relu") for kg in (1, 2)}
    | {"%s_vx%d" % (k, v) for k in _KINDS for v in (0, 1, 2)} | {"%s_vg%d" % (k, v) for k in _KINDS for v in (0, 2)}
    | {"xcd_ragged", "quarter16", "quarter20", "quarter24", "quarter28", "quarter32", "loop3_rounds1", "loop3_rounds2", "handover0", "handover4",
       "handover8", "wave_ragged", "waves_without_rows", "gy_scalar_store", "gy_vector_store", "loop3_skipped_for_gy", "loop3<live1,gy>", "loop3<live1,nogy>",
       "loop3<dead1,nogy>", "gy_null", "tiled_db_null"}      # (no loop3<dead1,gy>: grad_pre is written by k block 0, whose second group is never dead)
    | {"reduce_partials1", "reduce_partials_lt16", "reduce_partials16_64", "reduce_partials_gt64", "reduce_vec4", "reduce_scalar",
       "reduce_vec4_unaligned_dw", "reduce_scalar_unaligned_dw"})


def case_vectors(c):
    """(VX, VG) the entry will choose"""
    vx = vec_class(c["xo"], c["ldx"])
    vg = vec_class(c["go"], c["ldg"], pairs=False)
    if c["fz"] and vec_class(c["zo"], c["ldz"], pairs=False) != 2:
        vg = 0
    return vx, vg


def tiles(c, p):
    """[(nb, kb, n0, n1, k0, k1, skip3)] of the tiled kernel; skip3: the tile's waves write grad_pre through the scalar store and skip loop3"""
    out = []
    for nb in range(p["n_blocks"]):
        for kb in range(p["k_blocks"]):
            n0, k0 = 64 * nb, 64 * p["kg"] * kb
            skip3 = c["gy"] and kb == 0 and not (c["n_out"] % 4 == 0 and n0 + 64 <= c["n_out"])
            out.append((nb, kb, n0, min(n0 + 64, c["n_out"]), k0, min(k0 + 64 * p["kg"], c["k_in"]), skip3))
    return out


def case_classes(c):
    """the classes of CLASSES a case reaches, from the restatement alone"""
    p = plan(c["batch"], c["k_in"], c["n_out"])
    count, parts = c["k_in"] * c["n_out"], p["partials"]
    out = {"reduce_partials1" if parts == 1 else "reduce_partials_lt16" if parts < 16 else "reduce_partials16_64" if parts <= 64 else "reduce_partials_gt64",
           "reduce_vec4" if count % 4 == 0 else "reduce_scalar"}
    if c["dw_off"] % 4:
        out.add("reduce_vec4_unaligned_dw" if count % 4 == 0 else "reduce_scalar_unaligned_dw")
    wv = waves(p, c["batch"])
    if p["small"]:
        out.add("sw<%d,%d>" % (p["nt"], p["kt"]))
        rn, rk = c["n_out"] - 16 * (p["nt"] - 1), c["k_in"] - 16 * (p["kt"] - 1)
        out |= {"sw_rn%d" % rn} & CLASSES | {"sw_rk%d" % rk} & CLASSES
        rows = [b1 - b0 for _, b0, b1 in wv]
        if c["batch"] == 1:
            out.add("sw_batch1")
        if c["batch"] < 16:
            out.add("sw_batch_lt16")
        if any(r >= 16 for r in rows) and any(r % 4 for r in rows):
            out.add("sw_round_and_ragged_wave")
        if any(r > 16 and r % 16 for r in rows):
            out.add("sw_round_then_tail_in_one_wave")
        if parts > 64:
            out.add("sw_partials_gt64")
        if parts % 4:
            out.add("sw_padding_waves")
        if not c["db"]:
            out.add("sw_db_null")
        return out
    vx, vg = case_vectors(c)
    kg = p["kg"]
    out.add("tiled<%d,%d,%d,%d>" % (vx, vg, kg, int(c["fz"])))
    if c["fz"]:
        out.add("%s_kg%d" % (c["entry"], kg))
        out.add("gy_null" if not c["gy"] else "gy_scalar_store" if c["n_out"] % 4 else "gy_vector_store")
    if not c["db"]:
        out.add("tiled_db_null")
    if p["tiles"] < 8 and p["blocks"] % 8:
        out.add("xcd_ragged")
    tl = tiles(c, p)
    for nb, kb, n0, n1, k0, k1, skip3 in tl:
        kinds = []
        if n0 + 64 <= c["n_out"] and k0 + 64 * kg <= c["k_in"]:
            kinds.append("interior")
        if n0 + 64 > c["n_out"]:
            kinds.append("edge_n_scalar" if c["n_out"] % 4 else "edge_n_vec")
        if k0 + 64 * kg > c["k_in"]:
            kinds.append("edge_k")
            if kg == 2 and k0 + 64 >= c["k_in"]:
                kinds.append("edge_k_dead")
        if c["k_in"] < 4:
            kinds.append("k_lt4")
        for k in kinds:
            out |= {"%s_vx%d" % (k, vx), "%s_vg%d" % (k, vg)}
    full = quarter(min(p["rows"], c["batch"]))
    if "quarter%d" % full in CLASSES:
        out.add("quarter%d" % full)
    rows = [b1 - b0 for _, b0, b1 in wv]
    if any(r % 4 for r in rows):
        out.add("wave_ragged")
    if any(r == 0 for r in rows):
        out.add("waves_without_rows")
    long_rows = [r for r in rows if r >= 20]
    if long_rows:
        if any(t[6] for t in tl):
            out.add("loop3_skipped_for_gy")
        for nb, kb, n0, n1, k0, k1, skip3 in tl:
            if skip3:
                continue
            live = kg == 1 or k0 + 64 < c["k_in"]
            out.add("loop3<%s,%s>" % ("live1" if live else "dead1", "gy" if c["gy"] and kb == 0 else "nogy"))
        if any(not t[6] for t in tl):
            for r in long_rows:
                rounds, used = loop3(r)
                out |= {"loop3_rounds%d" % rounds, "handover%d" % (r - used)} & CLASSES
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the reference
def _factor(z, zoff, dtype, mutant=None):
    pos = z >= 0 if (mutant == "relu_zero_positive" and zoff == 0.0) else z > 0
    if mutant == "factor_on_positive":
        pos = np.zeros_like(pos)
    return np.where(pos, dtype(1), z + dtype(zoff))


def grad_pre(c, g, z, dtype=np.float64, mutant=None):
    """g * (z > 0 ? 1 : z + zoff) -- in np.float32 the device's own two operations, one add and one multiply per element"""
    g = np.asarray(g, dtype=dtype)
    if not c["fz"]:
        return g
    return g * _factor(np.asarray(z, dtype=dtype), ZOFF[c["entry"]], dtype, mutant)


def reference(c, x, g, z):
    """dict(dw [n_out, k_in], db [n_out]) in fp64 and gy [batch, n_out] in fp32 (None for the plain entry)"""
    gy = grad_pre(c, g, z)
    return dict(dw=gy.T @ np.asarray(x, dtype=np.float64), db=gy.sum(0), gy=grad_pre(c, g, z, np.float32) if c["fz"] else None)


# ---------------------------------------------------------------------------------------------------------------------------------------
# mutants: what a subtly wrong kernel would compute, through the restated ownership of rows and tiles.  `sees`: which check of the GPU file sees it
MUTANTS = {
    "drop_ragged_rows":      "values",      # a wave whose row count is no multiple of 4 drops the last 1-3 rows
    "handover_skipped":      "values",      # the rows loop3 leaves to the guarded loop are skipped
    "handover_twice":        "values",      # ... or counted by both
    "live_k_dead":           "values",      # a partial second k group judged dead: its columns stay zero
    "last_partial_unsummed": "values",
    "relu_zero_positive":    "values",      # z == 0 on the `1` side under ReLU
    "factor_on_positive":    "values",      # z + zoff applied to positive z as well
    "db_without_factor":     "values",      # db summed over grad_out, not grad_pre
    "tile_n_origin_off4":    "values",      # the last n tile reads g (and z) four columns to the right, clamped into the row
    "wave3_rows_unowned":    "values",      # the slice's last wave takes no rows (what a quarter rounded DOWN to 4 rows would lose)
    # the two below cannot change a value by construction; the CPU test asserts exactly that
    "dead_k_live":           "nothing: the dead group's accumulators belong to columns >= k_in, which are never stored (the NaN padding the clamped loads "
                             "read proves the store mask); only a load past the row's pitch would differ, and that shows as a fault, not a value",
    "gy_from_kb1":           "nothing: the k-block-1 tiles would store the same bits to the same addresses; the guard bands and NaN prefills stay as "
                             "they are.  It costs bandwidth and shows in the benchmark alone",
}


def _row_weights(c, p, mutant, runs3):
    w = np.ones(c["batch"])
    for i, (part, b0, b1) in enumerate(waves(p, c["batch"])):
        r = b1 - b0
        if mutant == "last_partial_unsummed" and part == p["partials"] - 1:
            w[b0:b1] = 0
        elif mutant == "drop_ragged_rows" and r % 4:
            w[b1 - r % 4:b1] = 0
        elif mutant == "wave3_rows_unowned" and not p["small"] and i % 4 == 3:
            w[b0:b1] = 0
        elif mutant in ("handover_skipped", "handover_twice") and runs3 and not p["small"] and r >= 20:
            w[b0 + loop3(r)[1]:b1] = 0 if mutant == "handover_skipped" else 2
    return w


def structured(c, x, g, z, mutant=None):
    """the reference's sums, formed tile by tile from the rows each wave owns -> dict(dw, db fp64, gy fp32 or None, gy_stores: how often an
    element of grad_pre is stored).  Without a mutant it equals reference(): every row is owned once"""
    p = plan(c["batch"], c["k_in"], c["n_out"])
    x = np.asarray(x, dtype=np.float64)
    gy = grad_pre(c, g, z, mutant=mutant)
    gb = np.asarray(g, dtype=np.float64) if mutant == "db_without_factor" else gy
    dw, db = np.zeros((c["n_out"], c["k_in"])), np.zeros(c["n_out"])
    if p["small"]:
        tl = [(nt, 0, 16 * nt, min(16 * nt + 16, c["n_out"]), 0, c["k_in"], False) for nt in range(p["nt"])]
    else:
        tl = tiles(c, p)
    weights = {flag: _row_weights(c, p, mutant, runs3=not flag) for flag in (False, True)}
    if mutant not in ("tile_n_origin_off4", "live_k_dead", "dead_k_live") and (not any(t[6] for t in tl) or np.array_equal(weights[False], weights[True])):
        # every tile counts every row alike: the tile-by-tile sums below are one product
        w = weights[False][:, None]
        return dict(dw=(gy * w).T @ x, db=(gb * w).sum(0), gy=grad_pre(c, g, z, np.float32, mutant) if c["fz"] else None,
                    gy_stores=(p["k_blocks"] if mutant == "gy_from_kb1" else 1) if c["gy"] else 0)
    last_nb = max(t[0] for t in tl)
    for nb, kb, n0, n1, k0, k1, skip3 in tl:
        w = weights[skip3][:, None]
        cols = np.arange(n0, n1)
        if mutant == "tile_n_origin_off4" and nb == last_nb:
            cols = np.minimum(cols + 4, c["n_out"] - 1)
        # the tile as the kernel forms it: 64-column groups read from columns clamped into the row, a dead group (no column below k_in) left
        # at zero, and the store mask k < k_in behind it
        groups = 1 if p["small"] else p["kg"]
        width = c["k_in"] if p["small"] else 64 * groups
        kcols = np.minimum(np.arange(k0, k0 + width), c["k_in"] - 1)
        tile = (gy[:, cols] * w).T @ x[:, kcols]
        for q in range(1, groups):
            dead = k0 + 64 * q >= c["k_in"]
            judged_dead = dead or (mutant == "live_k_dead" and c["k_in"] < k0 + 64 * (q + 1))
            if judged_dead and not (dead and mutant == "dead_k_live"):
                tile[:, 64 * q:64 * (q + 1)] = 0
        dw[n0:n1, k0:k1] = tile[:, :k1 - k0]
        if kb == 0:
            db[n0:n1] = (gb[:, cols] * w).sum(0)
    out = dict(dw=dw, db=db, gy=grad_pre(c, g, z, np.float32, mutant) if c["fz"] else None, gy_stores=1 if c["gy"] else 0)
    if out["gy"] is not None and mutant == "tile_n_origin_off4":
        n0 = 64 * last_nb
        out["gy"][:, n0:] = out["gy"][:, np.minimum(np.arange(n0, c["n_out"]) + 4, c["n_out"] - 1)]
    return out


def mutant_touches(mutant, c):
    """can `mutant` change an output of this case's scenes at all -- for the two that change no value: does the case run the code they are about?"""
    p = plan(c["batch"], c["k_in"], c["n_out"])
    wv = waves(p, c["batch"])
    if mutant == "drop_ragged_rows":
        return any((b1 - b0) % 4 for _, b0, b1 in wv)
    if mutant in ("handover_skipped", "handover_twice"):
        return not p["small"] and any(not t[6] for t in tiles(c, p)) and any(b1 - b0 >= 20 and b1 - b0 > loop3(b1 - b0)[1] for _, b0, b1 in wv)
    if mutant == "wave3_rows_unowned":
        return not p["small"] and any(b1 > b0 for i, (_, b0, b1) in enumerate(wv) if i % 4 == 3)
    if mutant == "live_k_dead":
        return p["kg"] == 2 and any(t[4] + 64 < c["k_in"] < t[4] + 128 for t in tiles(c, p))
    if mutant == "dead_k_live":
        return p["kg"] == 2 and any(t[4] + 64 >= c["k_in"] for t in tiles(c, p))
    if mutant == "gy_from_kb1":
        return c["gy"] and p["k_blocks"] > 1
    if mutant == "relu_zero_positive":
        return c["entry"] == "relu"
    if mutant in ("factor_on_positive", "db_without_factor"):
        return c["fz"]
    if mutant == "tile_n_origin_off4":
        tw = 16 if p["small"] else 64
        return c["n_out"] - (c["n_out"] - 1) // tw * tw > 1
    return mutant == "last_partial_unsummed"


# ---------------------------------------------------------------------------------------------------------------------------------------
# scenes
def _seed(c, salt):
    return zlib.crc32(("%s/%s" % (c["name"], salt)).encode()) & 0x7FFFFFFF


def exact_scene(c):
    """(x, g, z or None) as float32: integers in [-3, 3] and activation outputs whose factors are multiples of 1/4, so that every product and
    every partial sum, in any order, is a multiple of 1/4 below 2^24 in size: fp32 adds them without rounding"""
    assert 9 * 4 * c["batch"] < 2 ** 24, c["name"]
    rs = np.random.RandomState(_seed(c, "exact"))
    x = rs.randint(-3, 4, size=(c["batch"], c["k_in"])).astype(np.float32)
    g = rs.randint(-3, 4, size=(c["batch"], c["n_out"])).astype(np.float32)
    z = None
    if c["entry"] == "elu":          # factors 1, 1, 1 (z = +0: the z + 1 side), 1 (-0), 0.75, 0.5, 0 (z = -1)
        z = np.array([2.0, 0.5, 0.0, -0.0, -0.25, -0.5, -1.0], dtype=np.float32)[rs.randint(0, 7, size=g.shape)]
    elif c["entry"] == "relu":
        z = rs.randint(0, 3, size=g.shape).astype(np.float32)
    return x, g, z


def general_scene(c):
    rs = np.random.RandomState(_seed(c, "general"))
    x = rs.randn(c["batch"], c["k_in"]).astype(np.float32)
    g = rs.randn(c["batch"], c["n_out"]).astype(np.float32)
    z = None
    if c["fz"]:
        pre = rs.randn(c["batch"], c["n_out"]).astype(np.float32)
        z = np.where(pre > 0, pre, np.expm1(np.minimum(pre, 0))).astype(np.float32) if c["entry"] == "elu" else np.maximum(pre, np.float32(0))
    return x, g, z


def padded(a, off, ld):
    """the flat buffer a case's operand lives in -- NaN before the view, between a row's width and its pitch, and in EXTRA_ROWS rows behind the
    last -- and the dense values it holds: element [b, j] is flat[off + b * ld + j]"""
    rows, width = a.shape
    flat = np.full(off + (rows + EXTRA_ROWS) * ld, np.nan, dtype=np.float32)
    view = flat[off:off + rows * ld].reshape(rows, ld)
    view[:, :width] = a
    return flat


TWIN_N = 16                          # output rows the twins run on (every batch row)


def twin_rows(c):
    return np.unique(np.linspace(0, c["n_out"] - 1, TWIN_N).astype(np.int64))


@functools.lru_cache(maxsize=None)
def general_case(name):
    """dict(x, g, z, ref, tol (dw, db), twin_dist (dw, db)): the tolerance is 4 x the largest distance from the fp64 reference of fp32 twins that add
    the same products over the batch index forward, reversed and in chunks of 16 -- on twin_rows() of the output, over all batch rows"""
    c = CASES[name]
    x, g, z = general_scene(c)
    ref = reference(c, x, g, z)
    nn = twin_rows(c)
    gy32 = np.ascontiguousarray((ref["gy"] if c["fz"] else g)[:, nn])
    B = c["batch"]

    def seq(order):
        dw, db = np.zeros((nn.size, c["k_in"]), dtype=np.float32), np.zeros(nn.size, dtype=np.float32)
        for b in order:
            dw += gy32[b][:, None] * x[b][None, :]
            db += gy32[b]
        return dw, db

    def chunked():
        dw, db = np.zeros((nn.size, c["k_in"]), dtype=np.float32), np.zeros(nn.size, dtype=np.float32)
        for b0 in range(0, B, 16):
            pw, pb = seq(range(b0, min(b0 + 16, B)))
            dw += pw
            db += pb
        return dw, db

    dist = [0.0, 0.0]
    for twin, (dw, db) in zip([t[0] for t in M.TWINS], (seq(range(B)), seq(range(B - 1, -1, -1)), chunked())):
        d = (float(np.abs(dw.astype(np.float64) - ref["dw"][nn]).max()), float(np.abs(db.astype(np.float64) - ref["db"][nn]).max()))
        print("wgrad", name, "twin", twin, "distance dw", d[0], "db", d[1])
        dist = [max(dist[0], d[0]), max(dist[1], d[1])]
    return dict(x=x, g=g, z=z, ref=ref, tol=(4.0 * dist[0], 4.0 * dist[1]), twin_dist=tuple(dist))


# ---------------------------------------------------------------------------------------------------------------------------------------
# refusals: (name, entry, edits of an accepted call's arguments, expected code name).  The accepted call: args() of the GPU / CPU test
REFUSALS = [
    ("batch 0", "plain", dict(batch=0), "E_UNSUPPORTED"),
    ("batch -1", "elu", dict(batch=-1), "E_UNSUPPORTED"),
    ("k_in * n_out > 140000", "plain", dict(k_in=351, n_out=399), "E_UNSUPPORTED"),
    ("ldx < k_in", "plain", dict(short="ldx"), "E_INVALID"),
    ("ldg < n_out", "relu", dict(short="ldg"), "E_INVALID"),
    ("ldz < n_out", "elu", dict(short="ldz"), "E_INVALID"),
    ("workspace one byte short", "plain", dict(ws_short=1), "E_INVALID"),
    ("x NULL", "plain", dict(null="x"), "E_INVALID"),
    ("g NULL", "elu", dict(null="g"), "E_INVALID"),
    ("dw NULL", "relu", dict(null="dw"), "E_INVALID"),
    ("workspace NULL", "plain", dict(null="ws"), "E_INVALID"),
    ("elu_out NULL", "elu", dict(null="z"), "E_INVALID"),
    ("relu_out NULL", "relu", dict(null="z"), "E_INVALID"),
    ("ELU entry on a single-wave shape", "elu", dict(k_in=45, n_out=19), "E_UNSUPPORTED"),
    ("ReLU entry on a single-wave shape", "relu", dict(k_in=64, n_out=64), "E_UNSUPPORTED"),
    ("workspace 4 bytes off 16-byte alignment, k_in % 4 == 0", "plain", dict(ws_off=4), "E_INVALID"),
    ("workspace 8 bytes off 16-byte alignment, k_in % 4 == 0", "relu", dict(ws_off=8), "E_INVALID"),
    ("grad_pre 4 bytes off 16-byte alignment, n_out % 4 == 0", "elu", dict(gy_off=4), "E_INVALID"),
    ("grad_pre 8 bytes off 16-byte alignment, n_out % 4 == 0", "relu", dict(gy_off=8), "E_INVALID"),
]
REFUSAL_SHAPE = dict(batch=5, k_in=64, n_out=80)          # tiled, k_in % 4 == 0 and n_out % 4 == 0: both vector stores


def refusal_call(L, entry, edits, address, deferred=None):
    """the return code of one refused call.  address(floats) -> the 16-byte aligned address of a NaN-filled buffer of that many floats, valid for
    everything an ACCEPTED call of the edited shape could touch: an offset of 4 or 8 bytes stays inside it"""
    import ctypes
    s = dict(REFUSAL_SHAPE)
    s.update({k: v for k, v in edits.items() if k in s})
    shape = plan(max(s["batch"], 1), s["k_in"], s["n_out"])
    ws_bytes = shape["bytes"] if shape else 1 << 16
    b = max(s["batch"], 1)
    ldx, ldg, ldz = (w - 1 if edits.get("short") == name else w + 4 for name, w in (("ldx", s["k_in"]), ("ldg", s["n_out"]), ("ldz", s["n_out"])))
    ptr = dict(x=address((b + 1) * (s["k_in"] + 4)), g=address((b + 1) * (s["n_out"] + 4)), z=address((b + 1) * (s["n_out"] + 4)),
               dw=address(s["k_in"] * s["n_out"] + 4), db=address(s["n_out"] + 4), gy=address(b * s["n_out"] + 4), ws=address(ws_bytes // 4 + 4))
    ptr["ws"] += edits.get("ws_off", 0)
    ptr["gy"] += edits.get("gy_off", 0)
    if "null" in edits:
        ptr[edits["null"]] = None
    a = [ptr["x"], ldx, ptr["g"], ldg] + ([ptr["z"], ldz] if entry != "plain" else []) + [s["batch"], s["k_in"], s["n_out"], ptr["dw"], ptr["db"]]
    a += ([ptr["gy"]] if entry != "plain" else []) + [ptr["ws"], ws_bytes - edits.get("ws_short", 0), None]
    if deferred is not None:
        return getattr(L, ENTRY[entry] + "_deferred")(*a, ctypes.byref(deferred))
    return getattr(L, ENTRY[entry])(*a)
