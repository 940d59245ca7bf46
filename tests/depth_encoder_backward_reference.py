"""TEST INFRASTRUCTURE -- numpy fp64 reference of lsim_depth_encode_backward, written from the formulas in include/lsim.h (not from the kernel),
with a per-entry ERROR BOUND for an fp32 implementation, derived as depth_encoder_reference.py derives the forward's and never tuned.

The forward errors E_a1, E_a2, E_z are propagated exactly as in depth_encoder_reference.encode (the same statements, kept per layer here because
the backward needs the activations).  `latent` is an INPUT of the backward: any fp32 forward -- the fused launch, the CPU build, the reference
rounded to fp32 -- is within E_z of the exact z, so E_z is its bound.  g is exact (both sides read the same floats).

u = 2^-24.  Every sum of K products of computed factors p, r with bounds E_p, E_r, summed in fp32 in any order, fused or not, is within

    (K + 2) u sum (|p| + E_p)(|r| + E_r)  +  sum (|p| E_r + E_p |r| + E_p E_r)

of the exact sum of the exact products (Higham 3.1 on the computed factors, plus the factors' own errors).  A plain sum is the case r = 1,
E_r = 0, an elementwise product the case K = 1.  For the weight and bias gradients K = B * positions; for da2 K = latent_dim; for da1
K = c2 * k2 * k2 (the most taps that can reach one position).  ELU'(a) = a > 0 ? 1 : a + 1 is 1-Lipschitz in a and one addition: E = E_a + u."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import depth_encoder_reference as R

U = R.U
NAMES = ("gw1", "gb1", "gw2", "gb2", "gw3", "gb3")


def _sum(contract, K, p, Ep, r, Er):
    """(exact sum, bound) of sum p * r under `contract(p, r)`"""
    ap, ar = np.abs(p), np.abs(r)
    return contract(p, r), (K + 2) * U * contract(ap + Ep, ar + Er) + contract(ap, Er) + contract(Ep, ar) + contract(Ep, Er)


def _delu(a, Ea):
    return np.where(a > 0, 1.0, a + 1.0), Ea + U


def _windows(x, k, s):
    return sliding_window_view(x, (k, k), axis=(2, 3))[:, :, ::s, ::s]           # [N, C, h, w, k, k]


def forward(x, params, s1, s2, final_act):
    """((a1, E_a1), (a2, E_a2), (latent, E_z)), fp64: depth_encoder_reference.encode's statements, layer by layer"""
    w1, b1, w2, b2, w3, b3 = (np.asarray(p, np.float64) for p in params)
    x = np.asarray(x, np.float64)
    e = np.zeros_like(x)
    acts = []
    for w, b, s in ((w1, b1, s1), (w2, b2, s2)):
        K = w.shape[1] * w.shape[2] * w.shape[3]
        bb = b[None, :, None, None]
        pre = R.conv(x, w, s) + bb
        e_pre = (K + 2) * U * (np.abs(bb) + R.conv(np.abs(x) + e, np.abs(w), s)) + R.conv(e, np.abs(w), s)
        x, e = R._act(pre, e_pre, True)
        acts.append((x, e))
    f, ef = x.reshape(x.shape[0], -1), e.reshape(e.shape[0], -1)
    K = f.shape[1]
    pre = f @ w3.T + b3
    e_pre = (K + 2) * U * (np.abs(b3) + (np.abs(f) + ef) @ np.abs(w3).T) + ef @ np.abs(w3).T
    return acts[0], acts[1], R._act(pre, e_pre, final_act)


def backward(x, params, g, s1, s2, final_act, swap_w2_in_da1=False):
    """x [B, frames, H, W], params (w1, b1, w2, b2, w3, b3) in torch's layout, g [B, L] -> ({name: gradient}, {name: bound}, latent), fp64.
    `swap_w2_in_da1`: the WRONG backward with ky / kx of w2 swapped in the da1 step only (the sensitivity test)"""
    w1, b1, w2, b2, w3, b3 = (np.asarray(p, np.float64) for p in params)
    x = np.asarray(x, np.float64)
    g = np.asarray(g, np.float64)
    (a1, Ea1), (a2, Ea2), (lat, Ez) = forward(x, params, s1, s2, final_act)
    B = x.shape[0]
    zero = np.zeros(())
    mul = lambda p, r: p * r
    if final_act:
        dl, Edl = _delu(lat, Ez)
        dz, Edz = _sum(mul, 1, g, zero, dl, Edl)
    else:
        dz, Edz = g, np.zeros_like(g)
    one = np.ones(())
    grads, bounds = {}, {}
    grads["gb3"], bounds["gb3"] = _sum(lambda p, r: (p * r).sum(0), B, dz, Edz, one, zero)
    f, Ef = a2.reshape(B, -1), Ea2.reshape(B, -1)
    grads["gw3"], bounds["gw3"] = _sum(lambda p, r: p.T @ r, B, dz, Edz, f, Ef)
    da2, Eda2 = _sum(lambda p, r: p @ r, w3.shape[0], dz, Edz, w3, np.zeros_like(w3))
    da2, Eda2 = da2.reshape(a2.shape), Eda2.reshape(a2.shape)
    d2, Ed2 = _sum(mul, 1, da2, Eda2, *_delu(a2, Ea2))
    P2 = a2.shape[2] * a2.shape[3]
    grads["gb2"], bounds["gb2"] = _sum(lambda p, r: (p * r).sum((0, 2, 3)), B * P2, d2, Ed2, one, zero)
    k2 = w2.shape[2]
    wgrad2 = lambda p, r: np.einsum("nchw,ndhwij->cdij", p, _windows(r, k2, s2), optimize=True)
    grads["gw2"], bounds["gw2"] = _sum(wgrad2, B * P2, d2, Ed2, a1, Ea1)
    wt = w2.transpose(0, 1, 3, 2) if swap_w2_in_da1 else w2
    h2, w2e = a2.shape[2], a2.shape[3]

    def scatter(p, r):          # p: w2-like [c2, c1, k, k], r: d2-like [B, c2, h2, w2]
        out = np.zeros_like(a1)
        for i in range(k2):
            for j in range(k2):
                out[:, :, i:i + s2 * h2:s2, j:j + s2 * w2e:s2] += np.einsum("ncyx,cd->ndyx", r, p[:, :, i, j])
        return out

    da1, Eda1 = _sum(scatter, w2.shape[0] * k2 * k2, wt, np.zeros_like(wt), d2, Ed2)
    d1, Ed1 = _sum(mul, 1, da1, Eda1, *_delu(a1, Ea1))
    P1 = a1.shape[2] * a1.shape[3]
    grads["gb1"], bounds["gb1"] = _sum(lambda p, r: (p * r).sum((0, 2, 3)), B * P1, d1, Ed1, one, zero)
    k1 = w1.shape[2]
    wgrad1 = lambda p, r: np.einsum("nchw,ndhwij->cdij", p, _windows(r, k1, s1), optimize=True)
    grads["gw1"], bounds["gw1"] = _sum(wgrad1, B * P1, d1, Ed1, x, np.zeros_like(x))
    return grads, bounds, lat
