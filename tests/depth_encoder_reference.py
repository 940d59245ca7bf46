"""TEST INFRASTRUCTURE -- numpy fp64 reference of lsim_depth_encode, written from the comment in include/lsim.h (not from the kernel), with a
per-output ERROR BOUND for an fp32 implementation, propagated layer by layer.

The bound.  u = 2^-24 (fp32 unit round-off).  A dot product of length K with a bias, summed in fp32 in any order with or without fused
multiply-adds, differs from the exact one by at most (K + 2) u (|b| + sum |w| |x|) to first order (K - 1 additions, K products, the bias
addition; Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).  When the inputs themselves carry an error bound E_in (0 for
hist, which both sides read exactly) the computed inputs are bounded by |x| + E_in and their error passes through the weights:

    E_pre = (K + 2) u (|b| + sum |w| (|x| + E_in)) + sum |w| E_in

ELU is 1-Lipschitz, so the error of its argument passes at most unchanged; its own evaluation (expm1f, a few ulp of the result) adds

    E = E_pre + 4 u max(|y|, E_pre)

The bound is derived, not tuned: tests never widen it."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

U = 2.0 ** -24


def elu(v):
    return np.where(v > 0, v, np.expm1(np.minimum(v, 0)))


def conv(x, w, s):
    """x [N, C, H, W], w [O, C, k, k] -> [N, O, h, w]: no padding, no dilation, stride s"""
    k = w.shape[2]
    win = sliding_window_view(x, (k, k), axis=(2, 3))[:, :, ::s, ::s]          # [N, C, h, w, k, k]
    return np.einsum("nchwij,ocij->nohw", win, w, optimize=True)


def _act(pre, e_pre, act):
    if not act:
        return pre, e_pre
    y = elu(pre)
    return y, e_pre + 4 * U * np.maximum(np.abs(y), e_pre)


def encode(x, params, s1, s2, final_act, transpose_w2=False):
    """x [N, frames, H, W] (the values of hist), params = (w1, b1, w2, b2, w3, b3) in torch's layout -> (latent [N, L], bound [N, L]), fp64.
    `transpose_w2`: the WRONG network with ky / kx of w2 swapped (the sensitivity test)"""
    w1, b1, w2, b2, w3, b3 = (np.asarray(p, np.float64) for p in params)
    if transpose_w2:
        w2 = w2.transpose(0, 1, 3, 2)
    x = np.asarray(x, np.float64)
    e = np.zeros_like(x)
    for w, b, s in ((w1, b1, s1), (w2, b2, s2)):
        K = w.shape[1] * w.shape[2] * w.shape[3]
        bb = b[None, :, None, None]
        pre = conv(x, w, s) + bb
        e_pre = (K + 2) * U * (np.abs(bb) + conv(np.abs(x) + e, np.abs(w), s)) + conv(e, np.abs(w), s)
        x, e = _act(pre, e_pre, True)
    f, ef = x.reshape(x.shape[0], -1), e.reshape(e.shape[0], -1)           # (c, y, x): torch.flatten of NCHW
    K = f.shape[1]
    assert w3.shape[1] == K
    pre = f @ w3.T + b3
    e_pre = (K + 2) * U * (np.abs(b3) + (np.abs(f) + ef) @ np.abs(w3).T) + ef @ np.abs(w3).T
    return _act(pre, e_pre, final_act)


def due_sets(N, env_stride, tick, period, stagger, flags, episode_length, FILL_ALL=1, RESETS_ONLY=2):
    """(due [N], fill [N]) of one launch, from the rule in include/lsim.h"""
    e = np.arange(N)
    visited = e % env_stride == 0
    fill = visited & (bool(flags & FILL_ALL) | (np.asarray(episode_length) == 0))
    sched = np.zeros(N, bool) if flags & RESETS_ONLY else (tick + (e if stagger else 0)) % period == 0
    return visited & (fill | sched), fill
