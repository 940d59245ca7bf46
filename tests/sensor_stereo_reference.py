"""TEST INFRASTRUCTURE -- numpy reference of lsim_sensor_stereo, written from the comment of include/lsim.h (not from the kernel source):
which envs are visited, validity, disparity, the shadow, the minimum range, the edge with its foreground, the draw, the outcome and the
slots written, and the two counts.

Everything is float32 arrays under float32 operations (numpy rounds each one correctly, as the header demands of the quotients; no
product feeds a sum, so nothing can be fused), the draw is the integer Philox of philox_np, and the outcome is a function of the stored
bits of `depth`: every comparison with a launch is EXACT equality of hist and state.  No tolerance, no ambiguous share.

MUTANTS: `apply(..., mutant=name)` restates one line wrongly; tests/test_sensor_stereo.py asserts that each differs from the shim on at
least one scene of tests/sensor_stereo_scenes.py."""
import numpy as np

import philox_np
import sensor_model_reference as SR
from helpers import abi

TAG = abi.RNG_TAGS["sensor_stereo"]
FILL_ALL, RESETS_ONLY = SR.FILL_ALL, SR.RESETS_ONLY
F = np.float32
KEEP, HOLE, FATTEN = 0, 1, 2
MUTANTS = ("occluder_left", "strict_less", "u_plus_delta", "validity_ignored", "window_off_by_one", "tie_largest_index",
           "foreground_after_stores", "slot_ke_minus_2", "hole_without_clip", "tan_scale_ignored")


def y_hole(p, mutant=None):
    d = F(p["drop_value"])
    if mutant != "hole_without_clip":
        d = np.minimum(np.maximum(d, F(p["clip_lo"])), F(p["clip_hi"]))
    return F(F(d - F(p["offset"])) * F(p["gain"]))


def uniform0(p, env, tick):
    """u0 [R] float32 of env, exact"""
    R = p["width"] * p["height"]
    r = np.arange(R, dtype=np.uint32)
    x = philox_np.philox4x32_10(np.uint32(env), np.uint32(tick & 0xFFFFFFFF), np.uint32(TAG), np.uint32(p["stream_id"] << 16) | r, p["seed"], p["rank"])
    return (x[0] >> np.uint32(8)).astype(F) * F(2.0 ** -24)


def decide(Z, label, inv_scale, inst_row, p, env, tick, mutant=None):
    """(code [R] of KEEP / HOLE / FATTEN, fg [R] foreground index or -1) of one due env from its depth row Z [R], label row or None, and
    instrument row or None"""
    W, H = p["width"], p["height"]
    Z = np.asarray(Z, F).reshape(H, W)
    with np.errstate(all="ignore"):
        t = Z if inv_scale is None else (Z * np.asarray(inv_scale, F).reshape(H, W)).astype(F)
        valid = (np.abs(Z) <= np.finfo(F).max) & (F(p["t_lo"]) < t) & (t < F(p["t_hi"]))
        if label is not None:
            valid &= np.asarray(label).reshape(H, W) != 0
        if mutant == "validity_ignored":
            valid = np.ones((H, W), bool)
        fbe = F(p["fb"])
        if inst_row is not None and F(inst_row[4]) != F(1.0) and mutant != "tan_scale_ignored":
            fbe = F(fbe / F(inst_row[4]))
        delta = (fbe / Z).astype(F)
        col = np.broadcast_to(np.arange(W, dtype=F)[None, :], (H, W))
        u = (col + delta if mutant == "u_plus_delta" else col - delta).astype(F)
        window = p["window"] - (1 if mutant == "window_off_by_one" else 0)
        shadow = np.zeros((H, W), bool)
        for j in range(1, min(window, W - 1) + 1):
            if mutant == "occluder_left":
                shadow[:, j:] |= valid[:, :-j] & (u[:, :-j] <= u[:, j:])
            elif mutant == "strict_less":
                shadow[:, :-j] |= valid[:, j:] & (u[:, j:] < u[:, :-j])
            else:
                shadow[:, :-j] |= valid[:, j:] & (u[:, j:] <= u[:, :-j])
        shadow &= valid
        near = valid & (delta > F(p["max_disparity"]))
        thr = (Z * F(F(1.0) - F(p["edge_rel"]))).astype(F)
        rad = p["edge_radius"]
        fg = np.full((H, W), -1, np.int64)
        best = np.zeros((H, W), F)
        idx = np.arange(H * W).reshape(H, W)
        for dy in range(-rad, rad + 1):
            for dx in range(-rad, rad + 1):             # ascending index of the neighbour
                ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
                xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
                Zn, vn, cur = Z[ys, xs], valid[ys, xs], fg[yd, xd]
                closer = Zn <= best[yd, xd] if mutant == "tie_largest_index" else Zn < best[yd, xd]
                take = vn & (Zn < thr[yd, xd]) & ((cur < 0) | closer)
                fg[yd, xd] = np.where(take, idx[ys, xs], cur)
                best[yd, xd] = np.where(take, Zn, best[yd, xd])
    edge = valid & ~shadow & ~near & (fg >= 0)
    u0 = uniform0(p, env, tick).reshape(H, W)
    hole = shadow | near | (edge & (u0 < F(p["p_edge_hole"])))
    fat = edge & ~hole & (u0 < F(p["p_edge_cum"]))
    code = np.where(hole, HOLE, np.where(fat, FATTEN, KEEP)).reshape(-1)
    return code, np.where(fat, fg, -1).reshape(-1)


def first_slot(p, inst_row, fill, mutant=None):
    K = p["latency"] + p["frames"]
    if fill:
        return 0
    ke = K if inst_row is None else min(max(int(np.trunc(np.nan_to_num(float(inst_row[0])))), 0), p["latency"]) + p["frames"]
    return max(ke - (2 if mutant == "slot_ke_minus_2" else 1), 0)


def apply(hist, state, depth, labels, inv_scale, episode_length, inst, p, tick, flags, mutant=None):
    """(hist', state', codes [N, R]) after one launch: hist [N, K, R] (the rays' part of every slot), state [2], depth [N, R], labels [N, R]
    or None, inv_scale [R] or None, inst [N, 8] or None; p: the struct's by-value fields"""
    N, K = p["num_envs"], p["latency"] + p["frames"]
    due, fill = SR.due_sets(N, p["env_stride"], tick, p["period"], p["stagger"], flags, episode_length)
    new, st = np.array(hist, F, copy=True), np.array(state, np.int64, copy=True)
    codes = np.zeros((N, p["width"] * p["height"]), np.int64)
    for e in np.nonzero(due)[0]:
        row = None if inst is None else np.asarray(inst, F)[e]
        code, fg = decide(depth[e], None if labels is None else labels[e], inv_scale, row, p, int(e), tick, mutant)
        k0 = first_slot(p, row, bool(fill[e]), mutant)
        yh = y_hole(p, mutant)
        for r in np.nonzero(code)[0]:
            src = new if mutant == "foreground_after_stores" else hist
            new[e, k0:, r] = yh if code[r] == HOLE else src[e, K - 1, fg[r]]
        st[0] += int((code == HOLE).sum())
        st[1] += int((code == FATTEN).sum())
        codes[e] = code
    return new, st, codes
