"""TEST INFRASTRUCTURE -- builds and binds tests/emu/emu_eval_columns.cpp (the CPU shim of the evaluator-columns launch,
isaacgymloco_amd/csrc/ls_eval_columns.h compiled by g++ under LS_EMU), a numpy restatement of the semantics include/lsim.h states, the
value mix and grouping both test files (CPU and GPU) run, and Rig: one evaluator plus its columns over numpy arrays."""
import ctypes

import numpy as np

import emu_binding
import eval_emu_binding as EE
from emu_binding import aligned
from helpers import abi

MAX_COLS = abi.DEFINES["LSIM_EVAL_MAX_COLUMNS"]
COL_WORDS = abi.DEFINES["LSIM_EVAL_COL_WORDS"]
CLAMP = np.float32(2.0 ** 20)
# robot x type x level = 2 x 8 x 20 = 320 groups: more distinct groups than a block's 256 lanes map to distinct start slots
R_BIG, T_BIG, L_BIG = 2, 8, 20
SPECIALS = np.array([np.nan, np.inf, -np.inf, 3.0e6, -3.0e6, 1.0e-12, 0.0, -0.0, 1.0e30, -7.25, 1048576.0, 1023.9999], np.float32)


def lib():
    L = emu_binding.shim("eval_columns")
    L.emu_eval_columns_accumulate_ordered.argtypes = [ctypes.POINTER(abi.LsimEvalColumns), ctypes.c_void_p]       # test-only: the env order permutation
    return L


def EmuApi():
    """lsim_eval_* of the evaluator's shim and lsim_eval_columns_* of this one, for learn.evaluate.Evaluator(api=...)"""
    return emu_binding.api("eval", "eval_columns", count=("lsim_eval_accumulate", "lsim_eval_columns_accumulate", "lsim_eval_columns_clear"))


def start_slot(group):
    """ls_eval_slot's first probe (csrc/ls_eval.h) for a group index"""
    return int(((np.uint64(group) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(24)) & 255


def fix(v):
    """ls_eval_fix on an fp32 array: llrint(clamp(v, -2^20, 2^20) * 2^32), exact in float64 (24-bit significand times a power of two; the
    rounding of magnitudes below 2^-9 is round-half-even in both)"""
    v = np.minimum(np.maximum(np.asarray(v, np.float32), -CLAMP), CLAMP)
    return np.rint(v.astype(np.float64) * 4294967296.0).astype(np.int64)


def reference_add(table, group1, reset, values, num_groups, num_cols):
    """one lsim_eval_columns_accumulate launch restated: adds into `table` [num_groups, 1 + 3 num_cols] int64 in place"""
    for e in range(len(group1)):
        g1 = int(group1[e])
        if reset[e] != 0 or g1 == 0 or g1 - 1 >= num_groups:
            continue
        row = table[g1 - 1]
        row[0] += 1
        for k in range(num_cols):
            v = np.float32(values[e, k])
            if np.isfinite(v):
                with np.errstate(over="ignore"):
                    sq = np.float32(v * v)                      # one fp32 multiply; +inf when it overflows, and then the clamp
                row[1 + COL_WORDS * k] += fix(v)
                row[2 + COL_WORDS * k] += fix(sq)
            else:
                row[3 + COL_WORDS * k] += 1


def value_mix(rs, N, ld, step):
    """[N, ld] fp32: normal values of several magnitudes, negative ones included, with the SPECIALS scattered over rows and columns (other
    places each step); the columns past num_cols are read by nobody and hold NaN"""
    v = (rs.standard_normal((N, ld)) * rs.choice([1e-3, 1.0, 40.0, 900.0], size=(N, ld))).astype(np.float32)
    n_special = max(1, N // 3)
    rows = rs.randint(0, N, n_special)
    cols = rs.randint(0, ld, n_special)
    v[rows, cols] = SPECIALS[(np.arange(n_special) + step) % len(SPECIALS)]
    return v


def script(N, num_cols, ld, big_groups, steps=3, seed=0):
    """`steps` env-steps: per step the evaluator's reset_buf / terrain_levels (resets from step 2 on, each moving the env to another level,
    so its latched group changes) and the [N, ld] values.  Envs 0 and 1 (one block) start in two groups whose start slots collide."""
    rs = np.random.RandomState(seed + 17 * N + num_cols)
    robots = (np.arange(N) % R_BIG).astype(np.uint8) if big_groups else np.zeros(N, np.uint8)
    types = rs.randint(0, T_BIG, N).astype(np.int64)
    levels = rs.randint(0, L_BIG, N).astype(np.int64)
    pair = None
    if big_groups and N >= 2:
        pair = colliding_groups()
        for e, g in zip((0, 1), pair):
            robots[e], types[e], levels[e] = g // (T_BIG * L_BIG), (g // L_BIG) % T_BIG, g % L_BIG
    out = []
    for t in range(steps):
        reset = (rs.rand(N) < 0.3) if t >= 1 else np.zeros(N, bool)
        if pair is not None:
            reset[:2] = False
        levels = np.where(reset, rs.randint(0, L_BIG, N), levels).astype(np.int64)
        padded = value_mix(rs, N, ld, t)
        padded[:, num_cols:] = np.nan
        out.append(dict(reset_buf=reset.astype(np.uint8), terrain_levels=levels.copy(), terrain_types=types.copy(), robot_ids=robots.copy(), values=padded))
    return out, pair


def colliding_groups():
    """two groups of the 320 whose ls_eval_slot start slots are equal"""
    seen = {}
    for g in range(R_BIG * T_BIG * L_BIG):
        s = start_slot(g)
        if s in seen:
            return seen[s], g
        seen[s] = g
    raise AssertionError("no two of the 320 groups share a start slot")


class Rig:
    """the evaluator over numpy arrays (eval_emu_binding.EmuEval, whose other inputs stay zero apart from unit torque limits) and an
    lsim_eval_columns on its state"""

    def __init__(self, N, num_cols, ld, big_groups):
        self.N, self.num_cols, self.ld = N, num_cols, ld
        self.ev = EE.EmuEval(N, R_BIG, T_BIG, L_BIG, 7 if big_groups else 0)
        self.ev.bufs["torque_limits"][...] = 1.0
        self.groups = self.ev.table.shape[0]
        self.values = aligned((N, ld), np.float32)
        self.table = aligned((self.groups, 1 + COL_WORDS * num_cols), np.int64)
        c = abi.LsimEvalColumns()
        c.state, c.reset_buf = self.ev.state.ctypes.data, self.ev.bufs["reset_buf"].ctypes.data
        c.values, c.table = self.values.ctypes.data, self.table.ctypes.data
        c.num_envs, c.num_groups, c.num_cols, c.ld = N, self.groups, num_cols, ld
        self.c = c
        tb = ctypes.c_size_t()
        assert lib().emu_eval_columns_sizes(self.groups, num_cols, ctypes.byref(tb)) == 0 and tb.value == self.table.nbytes
        assert lib().emu_eval_columns_clear(ctypes.byref(c), None) == 0

    def feed(self, step):
        for k in ("reset_buf", "terrain_levels", "terrain_types", "robot_ids"):
            self.ev.bufs[k][...] = step[k]
        self.values[...] = step["values"]

    def group1(self):
        """the evaluator's latched groups, read out of its state with the layout of csrc/ls_eval.h"""
        N = self.N
        up16 = lambda n: (n + 15) & ~15
        off = 64 + up16(8 * N) + 16 * N
        return self.ev.state[off:off + 4 * N].view(np.int32).copy()

    def accumulate_columns(self, order=None):
        o = None if order is None else np.ascontiguousarray(order, np.int32)
        rc = lib().emu_eval_columns_accumulate_ordered(ctypes.byref(self.c), None if o is None else o.ctypes.data)
        assert rc == 0, rc
