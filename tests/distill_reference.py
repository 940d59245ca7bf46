"""TEST INFRASTRUCTURE -- numpy reference of lsim_distill_loss, written from the text of include/lsim.h: the gradient as the fp32 statement
(one subtraction, one product), the squared error as fp64 sums per workgroup chunk, and the cases the tests of both backends run."""
import numpy as np

PARTIALS = 256          # LSIM_DISTILL_PARTIALS (the binding asserts it)
BLOCK = 256             # lanes of a workgroup (csrc/ls_distill.h, LS_DL_BLOCK): with PARTIALS, what one pass of the grid covers
ACTIONS = (12, 13, 1)


def vector_path(actions, mu_stride, target_stride, g_stride):
    """the 128-bit path's condition on the widths (the rigs' arrays are 64-byte aligned)"""
    return all(v % 4 == 0 for v in (actions, mu_stride, target_stride, g_stride))


def batch_above_one_pass(actions, vector):
    """the smallest kind of minibatch in which a lane loops: every workgroup's chunk holds more items than it has lanes"""
    per_row = actions // 4 if vector else actions
    return PARTIALS * (BLOCK // per_row + 1) - 3         # the last workgroup's chunk is three rows short


def scale_of(batch, actions):
    return np.float32(2.0) / np.float32(batch * actions)


def cases():
    """(batch kind, actions, pad): pad 0 -- strides equal to actions; otherwise the three strides are actions + pad, + pad + 4 and + pad
    + 8 wide with NaN in the padding.  12 actions run padded by 4 (the vector path) and by 3 (the scalar one)"""
    out = []
    for actions in ACTIONS:
        for pad in ((0, 4, 3) if actions == 12 else (0, 3)):
            for kind in ("one", "seventy", "above one pass"):
                out.append((kind, actions, pad))
    return out


def make_case(kind, actions, pad, seed=0):
    """mu [B, mu_stride], target [2 B, target_stride], index [B] (a random injection, a few entries at -1 and at target_rows, their mu
    rows NaN), the strides, and whether the widths select the vector path"""
    strides = (actions + pad, actions + pad + (4 if pad else 0), actions + pad + (8 if pad else 0))
    vector = vector_path(actions, *strides)
    batch = {"one": 1, "seventy": 70, "above one pass": batch_above_one_pass(actions, vector)}[kind]
    rng = np.random.default_rng(seed + 1000 * actions + 10 * pad + batch)
    rows = 2 * batch
    mu = rng.standard_normal((batch, strides[0])).astype(np.float32)
    target = rng.standard_normal((rows, strides[1])).astype(np.float32)
    mu[:, actions:] = np.nan
    target[:, actions:] = np.nan
    index = rng.permutation(rows)[:batch].astype(np.int32)
    if batch > 1:
        skipped = rng.choice(batch, size=max(2, batch // 16), replace=False)
        index[skipped[0::2]] = -1
        index[skipped[1::2]] = rows
        mu[skipped] = np.nan
    return mu, target, index, strides, vector


def reference(mu, target, index, actions, scale, g_before):
    """(g as the call leaves it, fp64 sums of d * d per workgroup chunk [PARTIALS], the mask of rows that carry a loss)"""
    batch = mu.shape[0]
    ok = (index >= 0) & (index < target.shape[0])
    d = np.zeros((batch, actions), dtype=np.float32)
    d[ok] = mu[ok, :actions] - target[index[ok], :actions]
    g = g_before.copy()
    g[:, :actions] = np.float32(0.0)
    g[ok, :actions] = d[ok] * np.float32(scale)
    chunk = -(-batch // PARTIALS)
    sq = (d.astype(np.float64) ** 2).sum(axis=1)
    sums = np.array([sq[p * chunk:(p + 1) * chunk].sum() for p in range(PARTIALS)])
    return g, sums, ok
