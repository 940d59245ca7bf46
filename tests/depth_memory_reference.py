"""TEST INFRASTRUCTURE -- numpy fp64 reference of the depth memory (lsim_depth_memory_step, lsim_gru_sequence_forward / _backward), written from
the comment in include/lsim.h (not from the kernels), with a per-output ERROR BOUND for an fp32 implementation of the forward, propagated
step by step through h_prev.

The forward bound.  u = 2^-24.  A pre-activation is one sum of I + H products and two biases, formed in fp32 in any order with or without fused
multiply-adds: it differs from the exact one by at most (K + 2) u S with K = I + H + 1 terms and S the sum of the absolute values of its terms
(Higham, Accuracy and Stability of Numerical Algorithms, section 3.1), plus what the errors E of its inputs contribute through |W|:

    E_pre = (I + H + 3) u (|b_ih| + |b_hh| + |W_ih| (|x| + E_x) + |W_hh| (|h| + E_h)) + |W_ih| E_x + |W_hh| E_h

sigmoid is 1/4-Lipschitz and tanh 1-Lipschitz; their own evaluation adds SIG_ULPS / TANH_ULPS units of the result: expf to 1 ulp, one addition,
a division that the simulator's translation unit compiles without IEEE rounding (2.5 ulp), tanhf to 2 ulp -- 8 covers either with a margin
that does not come from any measurement.  Products and sums of the gate math carry their first-order terms and one u per operation.  The
translation unit also flushes denormals, which moves a result by less than TINY.

The backward has no propagated bound (products of five factors through T steps: the bound grows much faster than the error).  As DESIGN.md
section 7.12 states, its tolerance is 4 x the largest distance of a torch fp32 evaluation of the same formulas (`torch_backward_fp32`) from
this fp64 reference on the same case: both are fp32 evaluations of one formula that differ in summation order and in exp.  Never calibrated on
the kernel."""
import numpy as np

U = 2.0 ** -24
SIG_ULPS = 8
TANH_ULPS = 8
TINY = 1e-30


def sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def _f64(params):
    return tuple(np.asarray(p, np.float64) for p in params)


def cell(gi, e_gi, s_gi, h, e_h, w_hh, b_hh, mutant=None):
    """one step from the input projection gi [n, 3H] (error e_gi, sum of absolute terms s_gi; zeros / |gi| for a gi that is given exactly) and
    h_prev [n, H] (error e_h) -> dict of h', its bound, r, u, n, gh_n.  mutant "swap": the r and z blocks exchanged; "inside": W_hn (r * h)"""
    H = h.shape[1]
    K = w_hh.shape[1]
    gh = h @ w_hh.T + b_hh
    s_gh = np.abs(b_hh) + (np.abs(h) + e_h) @ np.abs(w_hh).T
    e_gh = (K + 2) * U * s_gh + e_h @ np.abs(w_hh).T
    sl = [slice(0, H), slice(H, 2 * H), slice(2 * H, 3 * H)]
    if mutant == "swap":
        sl = [sl[1], sl[0], sl[2]]
    R, Z, N = sl
    terms = K + 3                               # the rounding of joining the two sums: (terms of both) u (sum of absolute terms)
    pre_r, pre_u = gi[:, R] + gh[:, R], gi[:, Z] + gh[:, Z]
    e_pr = e_gi[:, R] + e_gh[:, R] + terms * U * (s_gi[:, R] + s_gh[:, R])
    e_pu = e_gi[:, Z] + e_gh[:, Z] + terms * U * (s_gi[:, Z] + s_gh[:, Z])
    r, u = sigmoid(pre_r), sigmoid(pre_u)
    e_r = 0.25 * e_pr + SIG_ULPS * U * r + TINY
    e_u = 0.25 * e_pu + SIG_ULPS * U * u + TINY
    ghn, e_ghn = gh[:, N], e_gh[:, N]
    if mutant == "inside":
        ghn = (r * h) @ w_hh[N].T + b_hh[N]
    pre_n = gi[:, N] + r * ghn
    e_pn = e_gi[:, N] + e_r * (np.abs(ghn) + e_ghn) + r * e_ghn + 3 * U * (np.abs(gi[:, N]) + np.abs(r * ghn)) + terms * U * s_gi[:, N]
    n = np.tanh(pre_n)
    e_n = e_pn + TANH_ULPS * U * np.abs(n) + TINY
    hn = (1.0 - u) * n + u * h
    e_hn = (e_u * (np.abs(n) + e_n) + (1.0 - u) * e_n + e_u * (np.abs(h) + e_h) + u * e_h
            + 4 * U * (np.abs((1.0 - u) * n) + np.abs(u * h)) + TINY)
    return {"h": hn, "e_h": e_hn, "r": r, "u": u, "n": n, "ghn": ghn, "e_r": e_r, "e_u": e_u, "e_n": e_n, "e_ghn": e_ghn}


def project(x, params):
    """gi = W_ih x + b_ih with its bound and its sum of absolute terms, x exact"""
    w_ih, _, b_ih, _ = _f64(params)
    x = np.asarray(x, np.float64)
    gi = x @ w_ih.T + b_ih
    s = np.abs(b_ih) + np.abs(x) @ np.abs(w_ih).T
    return gi, (x.shape[-1] + 2) * U * s, s


def step(z, p, h, fresh, params, mutant=None):
    """lsim_depth_memory_step for envs that step: z [N, L], p [N, P] or None, h [N, H], fresh [N] bool -> (h' [N, H], bound [N, H])"""
    _, w_hh, _, b_hh = _f64(params)
    x = np.asarray(z, np.float64) if p is None else np.concatenate((np.asarray(z, np.float64), np.asarray(p, np.float64)), axis=1)
    gi, e_gi, s_gi = project(x, params)
    h = np.where(np.asarray(fresh, bool)[:, None], 0.0, np.asarray(h, np.float64))
    c = cell(gi, e_gi, s_gi, h, np.zeros_like(h), w_hh, b_hh, mutant)
    return c["h"], c["e_h"]


def sequence(gi, h0, reset, params, e_gi=None, s_gi=None, mutant=None):
    """lsim_gru_sequence_forward: gi [T, n, 3H] (exact unless e_gi / s_gi of `project` are given), h0 [n, H], reset [T, n] ->
    dict hs [T, n, H], e_hs, save [T, n, 4H] = [r | u | n | gh_n], e_save"""
    _, w_hh, _, b_hh = _f64(params)
    gi = np.asarray(gi, np.float64)
    e_gi = np.zeros_like(gi) if e_gi is None else e_gi
    s_gi = np.abs(gi) if s_gi is None else s_gi
    h, e_h = np.asarray(h0, np.float64), np.zeros(np.shape(h0))
    out = {k: [] for k in ("hs", "e_hs", "save", "e_save")}
    for t in range(gi.shape[0]):
        keep = (np.asarray(reset[t]) == 0)[:, None]
        c = cell(gi[t], e_gi[t], s_gi[t], h * keep, e_h * keep, w_hh, b_hh, mutant)
        h, e_h = c["h"], c["e_h"]
        out["hs"].append(h)
        out["e_hs"].append(e_h)
        out["save"].append(np.concatenate((c["r"], c["u"], c["n"], c["ghn"]), axis=1))
        out["e_save"].append(np.concatenate((c["e_r"], c["e_u"], c["e_n"], c["e_ghn"]), axis=1))
    return {k: np.stack(v) for k, v in out.items()}


def backward(dhs, fwd, h0, reset, params):
    """the backward formulas of include/lsim.h on the fp64 forward `fwd` -> dict dgi [T, n, 3H], dghn [T, n, H], dh0 [n, H]"""
    _, w_hh, _, _ = _f64(params)
    dhs = np.asarray(dhs, np.float64)
    T, n, H = dhs.shape
    hs, save = fwd["hs"], fwd["save"]
    dgi, dghn = np.zeros((T, n, 3 * H)), np.zeros((T, n, H))
    dh = dhs[T - 1].copy()
    for t in range(T - 1, -1, -1):
        keep = (np.asarray(reset[t]) == 0)[:, None]
        hp = (hs[t - 1] if t > 0 else np.asarray(h0, np.float64)) * keep
        r, u, nn, ghn = (save[t][:, k * H:(k + 1) * H] for k in range(4))
        dn = dh * (1 - u) * (1 - nn * nn)
        du = dh * (hp - nn) * u * (1 - u)
        dr = dn * ghn * r * (1 - r)
        dgi[t] = np.concatenate((dr, du, dn), axis=1)
        dghn[t] = dn * r
        prev = (dh * u + np.concatenate((dr, du, dn * r), axis=1) @ w_hh) * keep
        dh = prev + dhs[t - 1] if t > 0 else prev
    return {"dgi": dgi, "dghn": dghn, "dh0": dh}


def param_grads(x, fwd, bwd, h0, reset):
    """(dW_ih, dW_hh, db_ih, db_hh) from the sequence backward's outputs, as include/lsim.h states them"""
    T, n, H = bwd["dghn"].shape
    x = np.asarray(x, np.float64)
    g = bwd["dgi"].reshape(T * n, 3 * H)
    gh = np.concatenate((g[:, :2 * H], bwd["dghn"].reshape(T * n, H)), axis=1)
    hp = np.concatenate((np.asarray(h0, np.float64)[None], fwd["hs"][:-1])) * (np.asarray(reset) == 0)[:, :, None]
    return g.T @ x.reshape(T * n, -1), gh.T @ hp.reshape(T * n, H), g.sum(0), gh.sum(0)


def torch_backward_fp32(gi, h0, reset, params, dhs):
    """the same formulas evaluated by torch in fp32 with autograd (gi and every step's gh as leaves / retained): dict dgi, dghn, dh0, hs.
    The yardstick of the backward tolerance; it never sees the kernel."""
    import torch
    H = np.shape(h0)[1]
    w_hh, b_hh = (torch.tensor(np.asarray(params[k], np.float32)) for k in (1, 3))
    g = torch.tensor(np.asarray(gi, np.float32), requires_grad=True)
    h_0 = torch.tensor(np.asarray(h0, np.float32), requires_grad=True)
    keep = torch.tensor((np.asarray(reset) == 0).astype(np.float32))
    h, hs, ghs = h_0, [], []
    for t in range(g.shape[0]):
        hp = h * keep[t][:, None]
        gh = hp @ w_hh.T + b_hh
        gh.retain_grad()
        r = torch.sigmoid(g[t, :, :H] + gh[:, :H])
        u = torch.sigmoid(g[t, :, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(g[t, :, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - u) * n + u * hp
        hs.append(h)
        ghs.append(gh)
    hs = torch.stack(hs)
    (hs * torch.tensor(np.asarray(dhs, np.float32))).sum().backward()
    return {"dgi": g.grad.numpy().astype(np.float64), "dghn": torch.stack([a.grad[:, 2 * H:] for a in ghs]).numpy().astype(np.float64),
            "dh0": h_0.grad.numpy().astype(np.float64), "hs": hs.detach().numpy().astype(np.float64)}


def backward_tolerance(gi, h0, reset, params, dhs, want):
    """{name: 4 x max |torch fp32 - fp64 reference|} for dgi, dghn, dh0 on this case, and the measured distances themselves"""
    got = torch_backward_fp32(gi, h0, reset, params, dhs)
    dist = {k: float(np.abs(got[k] - want[k]).max()) for k in ("dgi", "dghn", "dh0")}
    return {k: 4.0 * v for k, v in dist.items()}, dist
