"""fp64 numpy statements of the loss heads and the optimiser step of csrc/ls_learn.h -- lsim_estimator_loss, lsim_sinkhorn, lsim_ppo_loss,
lsim_ppo_loss_std and lsim_adam_clip_step_ex -- written from include/lsim.h and the comment blocks above the kernels; fp32 twins of each (the same
arithmetic in np.float32, in forms that differ only in legitimate ways) from which the tolerances follow; a restatement of the launch plan (template
instantiation, vector flags, block counts, the trip counts of every multi-in-flight loop) so that a CPU test can prove what the case tables reach;
the case tables, the scene builders, the refusals of the C ABI, and the mutants a test of these kernels has to see.

Everything here is numpy on the CPU.  The tolerance of a general case, per output, is 4 x the largest twin distance from the fp64 statement,
floored at 4 * 2^-23 of the statement's largest magnitude over that output; it never comes from a device run.
"""
import functools
import zlib

import numpy as np

import wgrad_shapes_reference as W

F64, F32 = np.float64, np.float32
ULP = 2.0 ** -23
EST_ROWS, SK_ROWS, PPO_ROWS = 64, 256, 256         # LS_EST_ROWS, LS_SK_ROWS, rows per block of lsim_k_ppo_loss
PPO_MAX_A, ADAM_MAX_TENSORS, ADAM_SLICES = 60, 48, 32
TEMPERATURE, SK_EPS = 3.0, 0.05                    # HIMEstimator's defaults
ITERS = (1, 3)
EXTRA_ROWS = W.EXTRA_ROWS


def _seed(*key):
    return zlib.crc32("/".join(str(k) for k in key).encode()) & 0x7FFFFFFF


def ceil_div(a, b):
    return (a + b - 1) // b


# ---------------------------------------------------------------------------------------------------------------------------------------
# the launch plan, restated
def inflight(n, stride, depth):
    """a loop `for (i = sl; i + (depth - 1) * stride < n; i += depth * stride)` followed by `for (; i < n; i += stride)` on `stride` interleaved
    slices of n rows -> per slice (passes of the multi-in-flight loop, rows its tail takes), and the rows all tails own"""
    per, tail_rows = [], []
    for sl in range(stride):
        i, passes = sl, 0
        while i + (depth - 1) * stride < n:
            i, passes = i + depth * stride, passes + 1
        tail = list(range(i, n, stride))
        per.append((passes, len(tail)))
        tail_rows += tail
    return dict(per=per, tail_rows=tail_rows, any_pass=any(p for p, _ in per))


def loop_classes(tag, lp):
    out = set()
    for passes, tail in lp["per"]:
        out |= {tag + (":passes>0" if passes else ":passes=0"), tag + (":tail" if tail else ":notail")}
    return out


def scale_loop(blocks, K):
    """lsim_k_sinkhorn_scale over `blocks` partial rows: 1024 / kp interleaved slices, eight rows in flight"""
    kp = 32 if K <= 32 else 64
    return kp, inflight(blocks, 1024 // kp, 8)


def sinkhorn_plan(B, K):
    blocks = ceil_div(B, SK_ROWS)
    kp, lp = scale_loop(blocks, K)
    floats = ((B * K + 63) // 64) * 64 + blocks * K + 64
    return dict(kmax=kp, blocks=blocks, vec=K % 4 == 0, scale=lp, bytes=4 * floats)


def estimator_plan(B, D, K):
    """None where lsim_estimator_loss_workspace refuses"""
    if B <= 0 or not 0 < D <= 32 or not 0 < K <= 64:
        return None
    wp = W.plan(2 * B, D, K)
    blocks = ceil_div(B, EST_ROWS)
    kp, lp = scale_loop(blocks, K)
    fold = (D * K) % 4 == 0
    take = lambda floats: (floats + 63) & ~63
    floats = take(2 * B * D) + take(2 * B) + take(2 * B * K) + take(2 * blocks * K + 128) + take(blocks * 2) + take((wp["bytes"] + 3) // 4)
    return dict(inst=(kp, 16 if D <= 16 else 32), vec=K % 4 == 0, zvec=D % 4 == 0, blocks=blocks, sk_blocks=ceil_div(B, SK_ROWS), scale=lp,
                small=wp["small"], partials=wp["partials"], wrows=wp["rows"], fold=fold, tail=inflight(wp["partials"], 64, 8) if fold else None,
                bytes=4 * floats)


def ppo_plan(B, A, std_mode):
    blocks = ceil_div(B, PPO_ROWS)
    return dict(blocks=blocks, bytes=4 * blocks * (4 + A if std_mode else 4), finish=inflight(blocks, 3, 4) if std_mode else None)


def adam_plan(numel):
    """per tensor: (slices of the 32 that own an element, most trips of a thread's loop, the last owning slice is ragged)"""
    out = []
    for n in numel:
        out.append((min(ADAM_SLICES, ceil_div(n, 256)), ceil_div(n, ADAM_SLICES * 256), n % 256 != 0))
    return out


def adam_bytes(count):
    return 4 * (count * ADAM_SLICES + 4)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Sinkhorn and the estimator loss head
def _block_weights(B, rows, K, mutant):
    """weight of every sample row in the column sums lsim_k_sinkhorn_scale forms from per-block partial rows: 1 unless a mutant loses rows"""
    nb = ceil_div(B, rows)
    w = np.ones(nb)
    if mutant == "last_block_dropped":
        w[-1] = 0.0
    if mutant == "loop_tail_skipped":
        lp = scale_loop(nb, K)[1]
        if lp["any_pass"]:
            w[lp["tail_rows"]] = 0.0
    return np.repeat(w, rows)[:B]


def _sk_direct(S, eps, iters, f):
    """HIMEstimator.sinkhorn as written: Q [K, B], rows and columns normalised in turn"""
    B, K = S.shape
    Q = np.exp(S / f(eps)).T
    Q = Q / Q.sum()
    for _ in range(iters):
        Q = Q / Q.sum(1, keepdims=True)
        Q = Q / f(K)
        Q = Q / Q.sum(0, keepdims=True)
        Q = Q / f(B)
    return (Q * f(B)).T


def _sk_factors(S, eps, iters, f, rows, mutant):
    """E = exp(S * (1 / eps)), u [K] after the last column rescaling, v [B] of the round before it (None for one iteration)"""
    B, K = S.shape
    E = np.exp(S * (f(1) / f(eps)))
    w = _block_weights(B, rows, K, mutant).astype(f)[:, None]
    u = f(1) / (f(K) * (E * w).sum(0))
    v = None
    for _ in range(1, iters):
        v = f(1) / (f(B) * (E @ u))
        u = f(1) / (f(K) * (E * v[:, None] * w).sum(0))
    return E, u, v


def _sk_fold(E, u, v, f, mutant):
    """the last step, B E u v with v = 1 / (B sum_k E u), folded into the caller: E u / sum_k E u"""
    if mutant == "last_step_not_folded" and v is not None:
        return f(E.shape[0]) * E * u * v[:, None]          # the previous round's v
    Eu = E * u
    return Eu / Eu.sum(1, keepdims=True)


_FACTORED_MUTANTS = ("u_other", "last_block_dropped", "loop_tail_skipped", "last_step_not_folded")


def sinkhorn(scores, eps, iters, dtype=F64, form="direct", mutant=None):
    f = dtype
    S = np.asarray(scores, dtype=f)
    if form == "reversed":
        return sinkhorn(S[::-1], eps, iters, f, "direct", mutant)[::-1]
    if form == "direct" and mutant not in _FACTORED_MUTANTS:
        return _sk_direct(S, eps, iters, f)
    E, u, v = _sk_factors(S, eps, iters, f, SK_ROWS, mutant)
    return _sk_fold(E, u, v, f, mutant)


def _log_softmax(x):
    mx = x.max(1, keepdims=True)
    return x - (mx + np.log(np.exp(x - mx).sum(1, keepdims=True)))


def _swap_quarters(dz, dmax):
    """the two exchange steps leave lane q with latents [d0, d0 + DMAX / 4), d0 = (q & 1) DMAX / 2 + (q >> 1) DMAX / 4: a kernel that took
    d0 = q DMAX / 4 would pair the gradient of quarter 1 with the latents of quarter 2 and the other way round"""
    D, dq = dz.shape[1], dmax // 4
    full = np.zeros((dz.shape[0], dmax), dtype=dz.dtype)
    full[:, :D] = dz
    full[:, dq:3 * dq] = np.concatenate([full[:, 2 * dq:3 * dq], full[:, dq:2 * dq]], axis=1)
    return full[:, :D]


def estimator_loss(enc, tgt, proto, vel, T, eps, iters, dtype=F64, form="direct", mutant=None):
    """dict(est, swap, total, d_vel [B, 3], d_lat [B, D] (together d_enc), d_tgt [B, D], d_proto [K, D], clamped (2 x [B] bool))"""
    f = dtype
    enc, tgt, P, vel = (np.asarray(a, dtype=f) for a in (enc, tgt, proto, vel))
    if form == "reversed":          # every sum over the batch runs the other way
        o = estimator_loss(enc[::-1], tgt[::-1], P, vel[::-1], T, eps, iters, f, "direct", mutant)
        for k in ("d_vel", "d_lat", "d_tgt"):
            o[k] = o[k][::-1]
        o["clamped"] = [c[::-1] for c in o["clamped"]]
        return o
    B, D = tgt.shape
    K = P.shape[0]
    factored = form == "factored"
    z, inv, clamped = [], [], []
    for x in (enc[:, 3:], tgt):                       # F.normalize(x, dim=-1, eps=1e-12)
        n = np.sqrt((x * x).sum(1))
        i = f(1) / np.maximum(n, f(1e-12))
        z.append(x * i[:, None]); inv.append(i); clamped.append(n < f(1e-12))
    S = [z[0] @ P.T, z[1] @ P.T]
    if factored or mutant in _FACTORED_MUTANTS:
        Euv = [_sk_factors(S[m], eps, iters, f, EST_ROWS, mutant) for m in range(2)]
        q = [_sk_fold(Euv[m][0], Euv[1 - m][1] if mutant == "u_other" else Euv[m][1], Euv[m][2], f, mutant) for m in range(2)]
    else:
        q = [_sk_direct(S[m], eps, iters, f) for m in range(2)]
    lp = [_log_softmax(S[m] * (f(1) / f(T)) if factored else S[m] / f(T)) for m in range(2)]
    swap = f(-0.5) * (q[0] * lp[1] + q[1] * lp[0]).sum() / (f(B) * f(K))
    e = enc[:, :3] - vel
    est = (e * e).sum() / (f(3) * f(B))
    c = f(-0.5) / (f(B) if mutant == "c_with_B" else f(B) * f(K))
    dS, g = [], []
    for m in range(2):                                # the other matrix's assignment weights this one's log-softmax
        cq = c * q[1 - m]
        d = cq - np.exp(lp[m]) * cq.sum(1, keepdims=True)
        dS.append(d * (f(1) / f(T)) if factored else d / f(T))
        dz = dS[m] @ P
        if mutant == "d0_quarter":
            dz = _swap_quarters(dz, 16 if D <= 16 else 32)
        zd = (z[m] * dz).sum(1, keepdims=True)
        proj = (dz - z[m] * zd) * inv[m][:, None]
        g.append(proj if mutant == "clamp_missing" else np.where(clamped[m][:, None], dz * inv[m][:, None], proj))
    zz, dd = np.concatenate(z), np.concatenate(dS)    # the prototype gradient: a Linear weight gradient over the 2 B stacked rows
    if mutant == "loop_tail_skipped":
        p = estimator_plan(B, D, K)
        if p["fold"] and p["tail"]["any_pass"]:
            w = np.ones(p["partials"])
            w[p["tail"]["tail_rows"]] = 0.0
            dd = dd * np.repeat(w, p["wrows"])[:2 * B].astype(f)[:, None]
    return dict(est=est, swap=swap, total=est + swap, d_vel=f(2) / (f(3) * f(B)) * e, d_lat=g[0], d_tgt=g[1], d_proto=dd.T @ zz, clamped=clamped)


EST_TWINS = ("direct", "factored", "reversed")

# (B, D, K, rows with a latent whose norm is below 1e-12).  Every case runs with 1 and 3 Sinkhorn iterations
EST_CASES = {
    "b1-d1-k1": (1, 1, 1, False),
    "b63-d5-k3": (63, 5, 3, False),
    "b65-d16-k32": (65, 16, 32, True),
    "b130-d20-k28": (130, 20, 28, False),
    "b129-d17-k31": (129, 17, 31, True),
    "b777-d9-k50": (777, 9, 50, False),
    "b200-d32-k64": (200, 32, 64, False),
    "b3700-d32-k64": (3700, 32, 64, False),
    "b7300-d4-k36": (7300, 4, 36, False),
    "b14400-d4-k8": (14400, 4, 8, False),
    "b3585-d17-k33": (3585, 17, 33, False),
}


def clamped_rows(B):
    """(student rows, target rows): an all-zero latent and one of norm 3e-13 each.  The zero student row is the batch's last: in the 65-row case
    the only live row of the second block"""
    return (B - 1, 1), (B // 2, 2)


def estimator_scene(name):
    B, D, K, clamp = EST_CASES[name]
    rs = np.random.RandomState(_seed("est", name))
    enc, tgt, vel = rs.randn(B, 3 + D).astype(F32), rs.randn(B, D).astype(F32), rs.randn(B, 3).astype(F32)
    proto = rs.randn(K, D)
    proto = (proto / np.linalg.norm(proto, axis=1, keepdims=True)).astype(F32)
    if clamp:
        (zs, ts), (zt, tt) = clamped_rows(B)
        enc[zs, 3:], tgt[zt] = 0.0, 0.0
        for a, r, c0 in ((enc, ts, 3), (tgt, tt, 0)):
            d = rs.randn(D)
            a[r, c0:] = (3e-13 * d / np.linalg.norm(d)).astype(F32)
    return dict(enc=enc, tgt=tgt, proto=proto, vel=vel)


def est_split(name, o):
    """an output dict -> the arrays that are compared, each against its own scale: the clamped rows (about 1e12 x the others) one by one"""
    B, D, K, clamp = EST_CASES[name]
    out = {k: np.asarray(o[k]) for k in ("est", "swap", "total", "d_vel", "d_proto")}
    (rows_s, rows_t) = clamped_rows(B) if clamp else ((), ())
    for k, rows in (("d_lat", rows_s), ("d_tgt", rows_t)):
        out[k] = np.delete(np.asarray(o[k]), list(rows), axis=0)
        for r in rows:
            out["%s[%d]" % (k, r)] = np.asarray(o[k])[r]
    return out


def tolerances(ref, twins, tag):
    """{key: dict(ref, tol, dist, scale)} from split outputs: tol = max(4 x twin distance, 4 * 2^-23 x scale)"""
    out = {}
    for k, r in ref.items():
        r = np.asarray(r, dtype=F64)
        scale = float(np.abs(r).max()) if r.size else 0.0
        dist = max(float(np.abs(np.asarray(t[k], dtype=F64) - r).max()) if r.size else 0.0 for t in twins)
        out[k] = dict(ref=r, tol=max(4.0 * dist, 4.0 * ULP * scale), dist=dist, scale=scale)
        print(tag, k, "scale %.3e twin distance %.3e (%.2e of scale) tolerance %.3e" % (scale, dist, dist / scale if scale else 0.0, out[k]["tol"]))
    return out


@functools.lru_cache(maxsize=None)
def estimator_case(name, iters):
    """dict(scene, out: {key: ref, tol, dist, scale})"""
    sc = estimator_scene(name)
    run = lambda **kw: estimator_loss(sc["enc"], sc["tgt"], sc["proto"], sc["vel"], TEMPERATURE, SK_EPS, iters, **kw)
    ref = run()
    (rows_s, rows_t) = clamped_rows(EST_CASES[name][0]) if EST_CASES[name][3] else ((), ())
    assert sorted(np.flatnonzero(ref["clamped"][0])) == sorted(rows_s) and sorted(np.flatnonzero(ref["clamped"][1])) == sorted(rows_t)
    twins = [est_split(name, run(dtype=F32, form=form)) for form in EST_TWINS]
    return dict(scene=sc, raw=ref, out=tolerances(est_split(name, ref), twins, "estimator %s iters %d" % (name, iters)))


def estimator_classes(name):
    B, D, K, clamp = EST_CASES[name]
    p = estimator_plan(B, D, K)
    out = {"est<%d,%d>" % p["inst"], "est_vec%d" % p["vec"], "est_zvec%d" % p["zvec"], "est_fold%d" % p["fold"]}
    out |= loop_classes("scale%d" % p["inst"][0], p["scale"])
    if p["fold"]:
        out |= loop_classes("est_tail", p["tail"])
    if B % EST_ROWS:
        out.add("est_ragged_block")
    if B % EST_ROWS == 1 and B > 1:
        out.add("est_block_of_one_row")
    if K < 4:
        out.add("est_k_lt4")
    if clamp:
        out.add("est_clamped_rows")
    assert p["small"], "the prototype gradient left the single-wave plan"
    return out


# (B, K, layout of `scores`): "vec" a 16-byte aligned view with a pitch that is a multiple of 4 where K is, "odd": an odd pitch, "off4": the view
# starts 4 bytes behind a 16-byte boundary (pitch a multiple of 4)
SK_CASES = {"b%d-k%d-%s" % c: c for c in [(1, 1, "vec"), (5, 3, "vec"), (255, 4, "vec"), (256, 32, "vec"), (257, 33, "vec"), (513, 64, "vec"),
                                           (58000, 5, "vec"), (300, 8, "vec"), (300, 8, "odd"), (300, 8, "off4"), (513, 64, "odd"), (513, 64, "off4")]}


def sk_layout(K, layout):
    """(offset of the view in floats, row pitch): the pitch is always wider than the row"""
    if layout == "odd":
        return 0, K + 1 if K % 2 == 0 else K + 2
    return (1 if layout == "off4" else 0), (K // 4 + 1) * 4


def sk_vec_in(K, layout):
    off, lds = sk_layout(K, layout)
    return K % 4 == 0 and lds % 4 == 0 and off % 4 == 0


def sinkhorn_scene(name):
    """cosine similarities in [-1, 1], as the estimator produces them"""
    B, K, _ = SK_CASES[name]
    rs = np.random.RandomState(_seed("sk", B, K))
    a, b = rs.randn(B, 8), rs.randn(K, 8)
    s = (a / np.linalg.norm(a, axis=1, keepdims=True)) @ (b / np.linalg.norm(b, axis=1, keepdims=True)).T
    return np.clip(s, -1.0, 1.0).astype(F32)


@functools.lru_cache(maxsize=None)
def sinkhorn_case(name, iters):
    S = sinkhorn_scene(name)
    ref = {"q": sinkhorn(S, SK_EPS, iters)}
    twins = [{"q": sinkhorn(S, SK_EPS, iters, F32, form)} for form in EST_TWINS]
    return dict(scores=S, out=tolerances(ref, twins, "sinkhorn %s iters %d" % (name, iters)))


def sinkhorn_classes(name):
    B, K, layout = SK_CASES[name]
    p = sinkhorn_plan(B, K)
    out = {"sk<%d>" % p["kmax"], "sk_vec%d" % p["vec"], "sk_vec_in%d" % sk_vec_in(K, layout)} | loop_classes("scale%d" % p["kmax"], p["scale"])
    if K % 4 == 0 and not sk_vec_in(K, layout):
        out.add("sk_scalar_in_vector_out_" + layout)
    if K < 4:
        out.add("sk_k_lt4")
    if B < SK_ROWS:
        out.add("sk_batch_lt256")
    if B == 1:
        out.add("sk_batch1")
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the clipped-PPO loss
LOG_SQRT_2PI = 0.9189385332046727


def ppo_loss(s, clip, cv, ce, clipped, std_mode, dtype=F64, form="direct", mutant=None):
    """s: dict(mu, sigma ([B, A], or [A] in std mode), value, actions, old_logp, adv, returns, tv, old_mu, old_sigma) ->
    dict(stats [5]: surrogate, value, entropy, kl, total; g_mu [B, A]; g_sigma [B, A] or g_std [A]; g_value [B]).  torch's sub-gradients:
    maximum splits ties evenly, clamp passes the gradient on the closed interval"""
    f = dtype
    a = {k: np.asarray(v, dtype=f) for k, v in s.items()}
    if form == "reversed":
        o = ppo_loss({k: (v if (k == "sigma" and std_mode) else v[::-1]) for k, v in a.items()}, clip, cv, ce, clipped, std_mode, f, "direct", mutant)
        return {k: (v if k in ("stats", "g_std") else v[::-1]) for k, v in o.items()}
    mu, B, A = a["mu"], a["mu"].shape[0], a["mu"].shape[1]
    # "action_loop": a row's sums over the actions go term by term into ONE accumulator, as any one-thread-per-sample kernel forms them.  numpy's
    # own sum keeps eight accumulators and adds them pairwise, which is closer to fp64 than such a loop can be (A = 60: the log-prob reaches ~90,
    # where one fp32 addition rounds by up to 4e-6).  Sums over the batch stay numpy's: across threads they are trees on any device
    over_a = (lambda x: np.cumsum(x, axis=1, dtype=f)[:, -1]) if form == "action_loop" else (lambda x: x.sum(1))
    over_b = lambda x: x.sum(0)
    sg = np.broadcast_to(a["sigma"], mu.shape)
    d, ls, dm, osg = a["actions"] - mu, np.log(sg), a["old_mu"] - mu, a["old_sigma"]
    if form == "recip":
        r = f(1) / sg
        t = d * r
        logp = (f(-0.5) * t * t - ls - f(LOG_SQRT_2PI)).sum(1)
        kl = (np.log(sg * (f(1) / osg) + f(1e-5)) + f(0.5) * (osg * osg + dm * dm) * r * r - f(0.5)).sum(1)
        dl_dmu, dl_dsg = t * r, t * t * r - r
    else:
        logp = over_a(-(d * d) / (f(2) * sg * sg) - ls - f(LOG_SQRT_2PI))
        kl = over_a(np.log(sg / osg + f(1e-5)) + (osg * osg + dm * dm) / (f(2) * sg * sg) - f(0.5))
        dl_dmu, dl_dsg = d / (sg * sg), d * d / (sg * sg * sg) - f(1) / sg
    ent = over_a(f(0.5 + LOG_SQRT_2PI) + ls)
    adv, invB, clip = a["adv"], f(1) / f(B), f(F32(clip))
    ratio = np.exp(logp - a["old_logp"])
    lo, hi = f(1) - clip, f(1) + clip
    s1, s2 = -adv * ratio, -adv * np.clip(ratio, lo, hi)
    opened = mutant == "clamp_open"
    in_range = ((ratio > lo) & (ratio < hi)) if opened else ((ratio >= lo) & (ratio <= hi))
    half = f(1.0 if mutant == "tie_weights_10" else 0.5)
    w1 = np.where(s1 > s2, f(1), np.where(s1 == s2, half, f(0)))
    dS = invB * (-adv) * (w1 + (f(1) - w1) * in_range) * ratio
    v, R = a["value"], a["returns"]
    if clipped:
        tv = a["tv"]
        dv = v - tv
        vc = tv + np.clip(dv, -clip, clip)
        l1, l2 = (v - R) * (v - R), (vc - R) * (vc - R)
        val = np.maximum(l1, l2)
        pas = ((dv > -clip) & (dv < clip)) if opened else ((dv >= -clip) & (dv <= clip))
        u1 = np.where(l1 > l2, f(1), np.where(l1 == l2, half, f(0)))
        dV = invB * (u1 * f(2) * (v - R) + (f(1) - u1) * f(2) * (vc - R) * pas)
    else:
        val = (R - v) * (R - v)
        dV = invB * f(2) * (v - R)
    m = [over_b(np.maximum(s1, s2)) * invB, over_b(val) * invB, over_b(ent) * invB, over_b(kl) * invB]
    out = dict(stats=np.array(m + [m[0] + f(cv) * m[1] - f(ce) * m[2]], dtype=f), g_mu=dS[:, None] * dl_dmu, g_value=f(cv) * dV)
    gs = dS[:, None] * dl_dsg - f(ce) * invB / sg
    if std_mode:
        if mutant == "g_std_missing_block":
            gs = gs[:(ceil_div(B, PPO_ROWS) - 1) * PPO_ROWS]
        out["g_std"] = over_b(gs)
    else:
        out["g_sigma"] = gs
    return out


PPO_TWINS = ("direct", "recip", "reversed", "action_loop")
PPO_BLOCKS = (1, 2, 3, 4, 9, 10, 12, 13, 14, 25)
PPO_CLIP, PPO_CV, PPO_CE = 0.2, 1.0, 0.01
RATIO_MARGIN, DV_MARGIN, L_MARGIN = 2e-3, 1e-4, 1e-4      # a general scene keeps every row this far from a clip boundary, in fp64


def _ppo_batches():
    """blocks -> batch: 256 n - 255, 256 n - 1 and 256 n in turn"""
    return {n: 256 * n - (255, 1, 0)[i % 3] for i, n in enumerate(PPO_BLOCKS)}


def _ppo_cases():
    out = {}
    for i, (n, B) in enumerate(_ppo_batches().items()):
        out["std-a%d-b%d-c%d" % ((1, 12, 60)[i % 3], B, i % 2)] = dict(entry="std", A=(1, 12, 60)[i % 3], B=B, clipped=i % 2)
        j = i + 1
        out["sigma-a%d-b%d-c%d" % ((1, 12, 60)[j % 3], B, 1 - i % 2)] = dict(entry="sigma", A=(1, 12, 60)[j % 3], B=B, clipped=1 - i % 2)
    out["sigma-a61-b300-c1"] = dict(entry="sigma", A=61, B=300, clipped=1)
    return out


PPO_CASES = _ppo_cases()
PPO_FN = {"sigma": "lsim_ppo_loss", "std": "lsim_ppo_loss_std"}


def ppo_near(s, std_mode):
    """rows of a scene within the margins of a branch boundary, by the fp64 statement: (ratio vs 1 +- clip, |v - tv| vs clip, l1 vs l2 where clipped)"""
    a = {k: np.asarray(v, dtype=F64) for k, v in s.items()}
    sg = np.broadcast_to(a["sigma"], a["mu"].shape)
    d = a["actions"] - a["mu"]
    ratio = np.exp((-(d * d) / (2 * sg * sg) - np.log(sg) - LOG_SQRT_2PI).sum(1) - a["old_logp"])
    clip = float(F32(PPO_CLIP))
    near_r = (np.abs(ratio - (1 - clip)) < RATIO_MARGIN) | (np.abs(ratio - (1 + clip)) < RATIO_MARGIN)
    dv = a["value"] - a["tv"]
    vc = a["tv"] + np.clip(dv, -clip, clip)
    near_v = np.abs(np.abs(dv) - clip) < DV_MARGIN
    near_l = (np.abs(dv) > clip) & (np.abs((a["value"] - a["returns"]) ** 2 - (vc - a["returns"]) ** 2) < L_MARGIN)
    return near_r, near_v, near_l


def ppo_scene(name):
    """a general scene: offending rows are MOVED off the boundaries (old_logp, target value or return shifted), none is masked"""
    c = PPO_CASES[name]
    B, A, std_mode = c["B"], c["A"], c["entry"] == "std"
    rs = np.random.RandomState(_seed("ppo", name))
    n = lambda *sh: rs.randn(*sh)
    mu = 0.5 * n(B, A)
    std = 0.5 + rs.rand(A)
    sigma = std if std_mode else std * (1 + 0.1 * np.clip(n(B, A), -2, 2))
    old_mu = mu + 0.15 / np.sqrt(A) * n(B, A)
    old_sigma = std * (1 + 0.1 / np.sqrt(A) * np.clip(n(B, A), -2, 2))
    actions = old_mu + old_sigma * n(B, A)
    om, osg, ac = (x.astype(F32).astype(F64) for x in (old_mu, old_sigma, actions))
    old_logp = (-(ac - om) ** 2 / (2 * osg * osg) - np.log(osg) - LOG_SQRT_2PI).sum(1)
    value = n(B)
    s = dict(mu=mu, sigma=sigma, value=value, actions=actions, old_logp=old_logp, adv=n(B), returns=n(B), tv=value + 0.3 * n(B), old_mu=old_mu,
             old_sigma=old_sigma)
    s = {k: np.ascontiguousarray(v, dtype=F32) for k, v in s.items()}
    for _ in range(50):
        near_r, near_v, near_l = ppo_near(s, std_mode)
        if not (near_r.any() or near_v.any() or near_l.any()):
            break
        s["old_logp"][near_r] += F32(0.01)
        s["tv"][near_v] += F32(0.01)
        s["returns"][near_l] += F32(0.05)
    return s


def ppo_tie_scene(A=12, std_mode=True):
    """(scene, clip, rows): a deterministic scene of the ties and the closed ends, in dyadic numbers.  Rows, six of each kind:
      adv0      adv = 0: both surrogate branches are -0 whatever the ratio -> g_mu and the row's share of g_std are exactly zero
      same      mu = old_mu, equal sigmas, old_logp the fp32 log-prob: the ratio is 1 within rounding, inside the interval, both branches
                equal -> the weights sum to 1 under any tie rule and the gradient is the unclipped one
      v_eq_tv   v = tv: l1 == l2 and the clamp passes -> 2 (v - R) whatever the tie rule
      end       v = tv +- clip EXACTLY: l1 == l2, and the clamp passes only on the CLOSED interval -> 2 (v - R); an open clamp gives half
      mid       |v - tv| > clip with R midway between v and the clamped value: l1 == l2 with the clamp saturated -> (v - R): the 1/2 - 1/2
                split is the only thing that fixes it (weights 1 / 0 give 2 (v - R))"""
    clip = 0.25
    kinds = ("adv0", "same", "v_eq_tv", "end", "mid")
    B = 6 * len(kinds)
    rows = {k: np.arange(6 * i, 6 * i + 6) for i, k in enumerate(kinds)}
    rs = np.random.RandomState(_seed("ppo-ties", A))
    dy = lambda *sh: rs.randint(-8, 9, size=sh) / 8.0
    mu, std = dy(B, A), 0.5 + rs.randint(0, 5, size=A) / 4.0
    sigma = std if std_mode else np.broadcast_to(std, (B, A)).copy()
    old_mu, old_sigma = mu + rs.randint(-1, 2, size=(B, A)) / 8.0 / A, np.broadcast_to(std, (B, A)) * (1 + rs.randint(0, 2, size=(B, A)) / 16.0)
    actions = mu + rs.randint(-2, 3, size=(B, A)) / 4.0
    value, tv, returns, adv = dy(B), dy(B) + 3.0, dy(B), rs.randint(1, 5, size=B) / 4.0 * rs.choice([-1, 1], size=B)
    adv[rows["adv0"]] = 0.0
    r = rows["same"]
    old_mu[r], old_sigma[r] = mu[r], np.broadcast_to(std, (6, A))
    tv[rows["v_eq_tv"]] = value[rows["v_eq_tv"]]
    r = rows["end"]
    tv[r] = value[r] - clip * np.array([1, -1, 1, -1, 1, -1])
    returns[r] = value[r] + np.array([0.5, 0.5, -0.5, -0.5, 1.5, -1.5])      # v != R: the gradient the clamp passes is not zero
    r = rows["mid"]
    tv[r] = value[r] - np.array([1, -1, 2, -2, 0.5, -0.5])                 # |v - tv| >= 0.5 > clip
    vc = tv[r] + np.clip(value[r] - tv[r], -clip, clip)
    returns[r] = (value[r] + vc) / 2
    s = dict(mu=mu, sigma=sigma, value=value, actions=actions, adv=adv, returns=returns, tv=tv, old_mu=old_mu, old_sigma=old_sigma)
    s = {k: np.ascontiguousarray(v, dtype=F32) for k, v in s.items()}
    sg = np.broadcast_to(s["sigma"], s["mu"].shape)
    d = s["actions"] - s["mu"]
    s["old_logp"] = (-(d * d) / (F32(2) * sg * sg) - np.log(sg) - F32(LOG_SQRT_2PI)).sum(1).astype(F32)     # the fp32 log-prob under the NEW policy
    s["old_logp"][rows["mid"]] += F32(0.5)                                  # some rows outside the ratio interval as well
    return s, clip, rows


def ppo_outputs(o):
    out = {"stat%d" % i: o["stats"][i] for i in range(5)}
    out.update({k: o[k] for k in ("g_mu", "g_sigma", "g_std", "g_value") if k in o})
    return out


@functools.lru_cache(maxsize=None)
def ppo_case(name):
    c = PPO_CASES[name]
    s, std_mode = ppo_scene(name), c["entry"] == "std"
    run = lambda **kw: ppo_outputs(ppo_loss(s, PPO_CLIP, PPO_CV, PPO_CE, c["clipped"], std_mode, **kw))
    return dict(scene=s, near=[int(m.sum()) for m in ppo_near(s, std_mode)],
                out=tolerances(run(), [run(dtype=F32, form=form) for form in PPO_TWINS], "ppo " + name))


@functools.lru_cache(maxsize=None)
def ppo_tie_case(std_mode, clipped=1):
    s, clip, rows = ppo_tie_scene(std_mode=std_mode)
    run = lambda **kw: ppo_outputs(ppo_loss(s, clip, PPO_CV, PPO_CE, clipped, std_mode, **kw))
    return dict(scene=s, clip=clip, rows=rows, out=tolerances(run(), [run(dtype=F32, form=form) for form in PPO_TWINS], "ppo ties std=%d" % std_mode))


def ppo_classes(name):
    c = PPO_CASES[name]
    p = ppo_plan(c["B"], c["A"], c["entry"] == "std")
    out = {"ppo_%s_a%d_c%d" % (c["entry"], c["A"], c["clipped"]), "ppo_%s_blocks%d" % (c["entry"], p["blocks"])}
    if p["finish"]:
        out |= loop_classes("ppo_finish", p["finish"])
    out.add("ppo_last_block_%s" % {1: "one_row", 255: "short_one_row", 0: "full"}.get(c["B"] % 256, "ragged"))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# gradient clipping + Adam
def _sumsq(x, f, order):
    """sum of squares of one tensor in dtype f: fp64 exactly as numpy gives it; fp32 one element after the other, forward, reversed, or in chunks of 256"""
    x = np.asarray(x, dtype=f)
    if f is F64:
        return (x * x).sum()
    sq = x * x
    if order == "chunks":
        pad = np.zeros(ceil_div(sq.size, 256) * 256, dtype=f)
        pad[:sq.size] = sq
        return np.cumsum(np.cumsum(pad.reshape(-1, 256), axis=1, dtype=f)[:, -1], dtype=f)[-1]
    return np.cumsum(sq[::-1] if order == "reversed" else sq, dtype=f)[-1]


def adam_clip_step(p, g, m, v, steps, wd, clip_count, lr, b1, b2, eps, max_norm, dtype=F64, form="lerp", order="forward", mutant=None):
    """clip_grad_norm_(tensors [0, clip_count), max_norm) then torch.optim.Adam.step() with per-tensor step counters and L2 weight decay.
    lists of arrays in, dict(p, g (clipped, as written back), m, v: lists; step [count]; norm; coef) out"""
    f = dtype
    count = len(p)
    group = range(count if mutant == "norm_all_tensors" else clip_count)
    total = f(0)
    for i in group:
        total = total + _sumsq(g[i], f, order)
    norm = np.sqrt(total)
    coef = np.minimum(f(max_norm) / (norm + f(1e-6)), f(1)) if max_norm > 0 else f(1)
    out = dict(p=[], g=[], m=[], v=[], step=np.asarray(steps, dtype=f) + f(1), norm=norm, coef=coef)
    b1, b2, one = f(b1), f(b2), f(1)
    for i in range(count):
        pi, gi, mi, vi = (np.asarray(x[i], dtype=f) for x in (p, g, m, v))
        gc = gi * (coef if i < clip_count else one)
        gw = gc + f(wd[i]) * pi if wd[i] != 0 else gc
        step = out["step"][0 if mutant == "step0_for_all" else i]
        mn = mi + (gw - mi) * (one - b1) if form == "lerp" else b1 * mi + (one - b1) * gw
        vn = b2 * vi + (one - b2) * gw * gw
        bc1, bc2s = one - np.power(b1, step), np.sqrt(one - np.power(b2, step))
        out["p"].append(pi - (f(lr) / bc1) * mn / (np.sqrt(vn) / bc2s + f(eps)))
        out["g"].append(gw if mutant == "decay_written_back" else gc)
        out["m"].append(mn); out["v"].append(vn)
    return out


ADAM_SIZES = (1, 255, 256, 257, 8191, 8192, 8193, 20000)
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = 1e-2, 0.9, 0.999, 1e-8
ADAM_TWINS = (("lerp", "forward"), ("b1m", "reversed"), ("lerp", "chunks"), ("b1m", "forward"))


def _adam_case(count, clip_count, max_norm, lr_on_device, first=0, steps=(0, 4, 999), decay=True):
    sizes = [ADAM_SIZES[(first + i) % 8] for i in range(count)]
    return dict(sizes=sizes, count=count, clip_count=clip_count, max_norm=max_norm, lr_dev=lr_on_device,
                steps=[float(steps[i % len(steps)]) for i in range(count)], wd=[(0.0, 0.1, 0.0, 1e-3)[i % 4] if decay else 0.0 for i in range(count)])


ADAM_CASES = {
    "n1-clip1-active-host": _adam_case(1, 1, 0.5, False, decay=False),
    "n1-clip0-active-dev": _adam_case(1, 0, 0.5, True, first=6, steps=(4,)),
    "n7-clip3-active-dev": _adam_case(7, 3, 0.5, True),
    "n7-clip7-off0-host": _adam_case(7, 7, 0.0, False, first=1),
    "n7-clip0-idle-dev": _adam_case(7, 0, 1e9, True, first=3, steps=(999, 0, 4)),
    "n7-clip3-negative-host": _adam_case(7, 3, -1.0, False, first=5, decay=False),
    "n48-clip48-active-host": _adam_case(48, 48, 0.5, False),
    "n48-clip3-idle-dev": _adam_case(48, 3, 1e9, True, first=4),
    "n48-clip0-off0-host": _adam_case(48, 0, 0.0, False, first=7, steps=(7,), decay=False),
    "n48-clip3-active-dev": _adam_case(48, 3, 0.5, True, first=2),
}


def adam_scene(name, exact=False):
    """lists p, g, m, v.  Parameters of the size of the step (0.02 against lr 0.01), so that an error in the step is not lost in the parameter's
    own rounding; second moments random and non-negative.  exact: gradients in {-2 .. 2}, their squared sum exact in fp32"""
    c = ADAM_CASES[name]
    rs = np.random.RandomState(_seed("adam", name, exact))
    s = dict(p=[], g=[], m=[], v=[])
    for n in c["sizes"]:
        s["p"].append((0.02 * rs.randn(n)).astype(F32))
        s["g"].append(rs.randint(-2, 3, size=n).astype(F32) if exact else rs.randn(n).astype(F32))
        s["m"].append((0.5 * rs.randn(n)).astype(F32))
        s["v"].append((rs.rand(n) ** 2).astype(F32))
    if exact:
        assert 4 * sum(c["sizes"]) < 2 ** 24
        s["g"][0][0] = 1.0                      # g * coef == coef exactly: the clip coefficient can be read back from the clipped gradient
    return s


def adam_outputs(o):
    cat = lambda k: np.concatenate([np.ravel(x) for x in o[k]])
    return dict(p=cat("p"), g=cat("g"), m=cat("m"), v=cat("v"), step=o["step"], norm=o["norm"])


@functools.lru_cache(maxsize=None)
def adam_case(name):
    c, s = ADAM_CASES[name], adam_scene(name)
    run = lambda **kw: adam_outputs(adam_clip_step(s["p"], s["g"], s["m"], s["v"], c["steps"], c["wd"], c["clip_count"], F32(ADAM_LR), F32(ADAM_B1),
                                                   F32(ADAM_B2), F32(ADAM_EPS), c["max_norm"], **kw))
    twins = [run(dtype=F32, form=form, order=order) for form, order in ADAM_TWINS]
    return dict(scene=s, out=tolerances(run(), twins, "adam " + name))


def adam_classes(name):
    c = ADAM_CASES[name]
    out = {"adam_count%d" % c["count"], "adam_clip_%s" % ("none" if c["clip_count"] == 0 else "all" if c["clip_count"] == c["count"] else "part"),
           "adam_max_norm_%s" % ("off" if c["max_norm"] <= 0 else "active" if c["max_norm"] < 1 else "idle"), "adam_lr_%s" % ("dev" if c["lr_dev"] else "host")}
    if c["max_norm"] < 0:
        out.add("adam_max_norm_negative")
    if len(set(c["steps"])) > 1:
        out.add("adam_steps_differ")
    if 0 < sum(1 for w in c["wd"] if w) < c["count"]:
        out.add("adam_decay_on_a_subset")
    for n, (slices, trips, ragged) in zip(c["sizes"], adam_plan(c["sizes"])):
        out |= {"adam_n%d" % n, "adam_slices%d" % slices, "adam_trips%d" % trips, "adam_ragged%d" % ragged}
        if slices < ADAM_SLICES:
            out.add("adam_idle_slices")
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# what the case tables have to reach
_LOOPS = ("scale32", "scale64", "est_tail", "ppo_finish")
CLASSES = (
    {"est<%d,%d>" % (k, d) for k in (32, 64) for d in (16, 32)} | {"sk<32>", "sk<64>"}
    | {"%s%d" % (flag, b) for flag in ("est_vec", "est_zvec", "est_fold", "sk_vec", "sk_vec_in") for b in (0, 1)}
    | {"%s:%s" % (lp, c) for lp in _LOOPS for c in ("passes>0", "passes=0", "tail", "notail")}
    | {"est_ragged_block", "est_block_of_one_row", "est_k_lt4", "est_clamped_rows", "sk_k_lt4", "sk_batch_lt256", "sk_batch1",
       "sk_scalar_in_vector_out_odd", "sk_scalar_in_vector_out_off4"}
    | {"ppo_%s_a%d_c%d" % (e, a, c) for e in ("sigma", "std") for a in (1, 12, 60) for c in (0, 1)} | {"ppo_sigma_a61_c1"}
    | {"ppo_%s_blocks%d" % (e, n) for e in ("sigma", "std") for n in PPO_BLOCKS}
    | {"ppo_sigma_blocks2", "ppo_last_block_one_row", "ppo_last_block_short_one_row", "ppo_last_block_full", "ppo_last_block_ragged"}
    | {"adam_count%d" % n for n in (1, 7, 48)} | {"adam_clip_none", "adam_clip_part", "adam_clip_all", "adam_max_norm_off", "adam_max_norm_active",
                                                  "adam_max_norm_idle", "adam_max_norm_negative", "adam_lr_dev", "adam_lr_host", "adam_steps_differ",
                                                  "adam_decay_on_a_subset", "adam_idle_slices"}
    | {"adam_n%d" % n for n in ADAM_SIZES} | {"adam_slices%d" % n for n in (1, 2, 32)} | {"adam_trips%d" % n for n in (1, 2, 3)}
    | {"adam_ragged0", "adam_ragged1"})


def all_classes():
    """{class: [cases]} over the four tables"""
    where = {}
    for fam, table, fn in (("est", EST_CASES, estimator_classes), ("sk", SK_CASES, sinkhorn_classes), ("ppo", PPO_CASES, ppo_classes),
                           ("adam", ADAM_CASES, adam_classes)):
        for name in table:
            for cls in fn(name):
                where.setdefault(cls, []).append(fam + ":" + name)
    return where


# ---------------------------------------------------------------------------------------------------------------------------------------
# mutants: wrong-but-plausible variants of the statements -> (family, the cases it is meant to touch)
def _est_names(pred):
    return [n for n in EST_CASES if pred(n, *EST_CASES[n][:3], estimator_plan(*EST_CASES[n][:3]))]


MUTANTS = {
    "d0_quarter":           ("est", lambda: _est_names(lambda n, B, D, K, p: D > (16 if D <= 16 else 32) // 4 and K > 1)),
    "u_other":              ("est", lambda: _est_names(lambda n, B, D, K, p: K > 1 and B > 1)),
    "last_block_dropped":   ("est", lambda: _est_names(lambda n, B, D, K, p: K > 1 and p["blocks"] > 1)),
    "clamp_missing":        ("est", lambda: [n for n in EST_CASES if EST_CASES[n][3]]),
    "last_step_not_folded": ("est3", lambda: _est_names(lambda n, B, D, K, p: K > 1 and B > 1)),
    "c_with_B":             ("est", lambda: _est_names(lambda n, B, D, K, p: K > 1)),
    "loop_tail_skipped":    ("est", lambda: _est_names(lambda n, B, D, K, p: p["scale"]["any_pass"] or (p["fold"] and p["tail"]["any_pass"]))),
    "tie_weights_10":       ("ppo_ties", None),
    "clamp_open":           ("ppo_ties", None),
    "g_std_missing_block":  ("ppo", lambda: [n for n in PPO_CASES if PPO_CASES[n]["entry"] == "std"]),
    "step0_for_all":        ("adam", lambda: [n for n in ADAM_CASES if len(set(ADAM_CASES[n]["steps"])) > 1]),
    "norm_all_tensors":     ("adam", lambda: [n for n in ADAM_CASES if ADAM_CASES[n]["clip_count"] < ADAM_CASES[n]["count"] and 0 < ADAM_CASES[n]["max_norm"] < 1]),
    "decay_written_back":   ("adam", lambda: [n for n in ADAM_CASES if any(ADAM_CASES[n]["wd"])]),
}
SK_MUTANTS = {"last_block_dropped": lambda: [n for n in SK_CASES if SK_CASES[n][0] > SK_ROWS],
              "last_step_not_folded": lambda: [n for n in SK_CASES if SK_CASES[n][1] > 1 and SK_CASES[n][0] > 1],
              "loop_tail_skipped": lambda: [n for n in SK_CASES if sinkhorn_plan(*SK_CASES[n][:2])["scale"]["any_pass"]]}


def beyond(case_out, mutant_out):
    """outputs on which a mutant is farther from the statement than the case's tolerance (a NaN or Inf counts)"""
    bad = []
    for k, o in case_out.items():
        d = np.abs(np.asarray(mutant_out[k], dtype=F64) - o["ref"])
        if d.size and not (np.nanmax(d) <= o["tol"] and np.isfinite(d).all()):
            bad.append(k)
    return bad


# ---------------------------------------------------------------------------------------------------------------------------------------
# refusals: (label, family, edits of an accepted call's arguments, code).  Every one is answered by the entry's argument checks on the host, before
# any launch.  Edits: set (argument -> value), null (argument), off (argument -> bytes added to the pointer), short (bytes taken off workspace_bytes)
SIGNATURES = {
    "est": ("lsim_estimator_loss", ["enc", "ld_enc", "tgt", "ld_tgt", "proto", "vel", "ld_vel", "batch", "latent", "K", "T", "eps", "iters", "losses",
                                    "g_enc", "g_tgt", "g_proto", "ws", "ws_bytes", "stream"]),
    "sk": ("lsim_sinkhorn", ["scores", "lds", "batch", "K", "eps", "iters", "out", "ws", "ws_bytes", "stream"]),
    "ppo": ("lsim_ppo_loss", ["mu", "sigma", "value", "actions", "old_logp", "adv", "returns", "tv", "old_mu", "old_sigma", "batch", "A", "clip", "cv", "ce",
                              "clipped", "out5", "g_mu", "g_sigma", "g_value", "ws", "ws_bytes", "stream"]),
    "adam": ("lsim_adam_clip_step_ex", ["count", "numel", "p", "g", "m", "v", "step", "wd", "clip_count", "lr_dev", "lr_host", "b1", "b2", "eps", "max_norm",
                                        "norm_out", "ws", "ws_bytes", "stream"]),
}
SIGNATURES["ppo_std"] = ("lsim_ppo_loss_std", SIGNATURES["ppo"][1])
REFUSAL_SHAPE = {"est": dict(batch=5, latent=8, K=12), "sk": dict(batch=5, K=8), "ppo": dict(batch=5, A=3), "ppo_std": dict(batch=5, A=3),
                 "adam": dict(count=3, numel=(5, 1, 300))}
_INV = "E_INVALID"
REFUSALS = (
    [("est " + l, "est", e, _INV) for l, e in [
        ("latent 33", dict(set=dict(latent=33))), ("latent 0", dict(set=dict(latent=0))), ("K 65", dict(set=dict(K=65))), ("K 0", dict(set=dict(K=0))),
        ("batch 0", dict(set=dict(batch=0))), ("ld_enc < 3 + latent", dict(set=dict(ld_enc=10))), ("ld_tgt < latent", dict(set=dict(ld_tgt=7))),
        ("ld_vel < 3", dict(set=dict(ld_vel=2))), ("temperature 0", dict(set=dict(T=0.0))), ("eps 0", dict(set=dict(eps=0.0))),
        ("iters 0", dict(set=dict(iters=0))), ("workspace one byte short", dict(short=1)), ("workspace 4 bytes off 16-byte alignment", dict(off=dict(ws=4))),
        ("workspace 8 bytes off 16-byte alignment", dict(off=dict(ws=8)))]
        + [(a + " NULL", dict(null=a)) for a in ("enc", "tgt", "proto", "vel", "losses", "g_enc", "g_tgt", "g_proto", "ws")]]
    + [("sinkhorn " + l, "sk", e, _INV) for l, e in [
        ("K 65", dict(set=dict(K=65))), ("K 0", dict(set=dict(K=0))), ("batch 0", dict(set=dict(batch=0))), ("iters 0", dict(set=dict(iters=0))),
        ("lds < K", dict(set=dict(lds=7))), ("eps 0", dict(set=dict(eps=0.0))), ("eps negative", dict(set=dict(eps=-0.05))),
        ("workspace one byte short", dict(short=1)), ("workspace 4 bytes off 16-byte alignment", dict(off=dict(ws=4))),
        ("out 4 bytes off 16-byte alignment", dict(off=dict(out=4))), ("out 8 bytes off 16-byte alignment", dict(off=dict(out=8)))]
        + [(a + " NULL", dict(null=a)) for a in ("scores", "out", "ws")]]
    + [("%s %s" % (fam, l), fam, e, _INV) for fam in ("ppo", "ppo_std") for l, e in [
        ("batch 0", dict(set=dict(batch=0))), ("num_actions 0", dict(set=dict(A=0))), ("workspace one byte short", dict(short=1)),
        ("clipped value loss without target_values", dict(null="tv"))]
        + [(a + " NULL", dict(null=a)) for a in ("mu", "sigma", "value", "actions", "old_logp", "adv", "returns", "old_mu", "old_sigma", "out5", "g_mu",
                                                 "g_sigma", "g_value", "ws")]]
    + [("ppo_std num_actions 61", "ppo_std", dict(set=dict(A=61)), _INV)]
    + [("adam " + l, "adam", e, _INV) for l, e in [
        ("count 49", dict(set=dict(count=49))), ("count 0", dict(set=dict(count=0))), ("clip_count > count", dict(set=dict(clip_count=4))),
        ("clip_count negative", dict(set=dict(clip_count=-1))), ("beta1 1", dict(set=dict(b1=1.0))), ("beta2 negative", dict(set=dict(b2=-0.1))),
        ("eps 0", dict(set=dict(eps=0.0))), ("workspace one byte short", dict(short=1)), ("a tensor of 0 elements", dict(numel0=1)),
        ("a negative weight decay", dict(wd_neg=2)), ("a NULL entry in the gradient table", dict(null_entry=("g", 1)))]
        + [(a + " NULL", dict(null=a)) for a in ("numel", "p", "g", "m", "v", "step", "ws")]])


def refusal_call(L, fam, edits, address):
    """the return code of one refused call.  address(floats) -> the 16-byte aligned address of a NaN-filled buffer of that many floats (+ 4), valid for
    everything an ACCEPTED call of the shape could touch"""
    import ctypes
    fn, names = SIGNATURES[fam]
    sh = REFUSAL_SHAPE[fam]
    if fam == "est":
        B, D, K = sh["batch"], sh["latent"], sh["K"]
        nbytes = estimator_plan(B, D, K)["bytes"]
        a = dict(enc=address((B + 1) * (3 + D + 2)), ld_enc=3 + D + 2, tgt=address((B + 1) * (D + 1)), ld_tgt=D + 1, proto=address(K * D), vel=address((B + 1) * 4),
                 ld_vel=4, batch=B, latent=D, K=K, T=TEMPERATURE, eps=SK_EPS, iters=3, losses=address(3), g_enc=address(B * (3 + D)), g_tgt=address(B * D),
                 g_proto=address(K * D))
    elif fam == "sk":
        B, K = sh["batch"], sh["K"]
        nbytes = sinkhorn_plan(B, K)["bytes"]
        a = dict(scores=address((B + 1) * (K + 4)), lds=K + 4, batch=B, K=K, eps=SK_EPS, iters=3, out=address(B * K + 4))
    elif fam in ("ppo", "ppo_std"):
        B, A = sh["batch"], sh["A"]
        nbytes = ppo_plan(B, A, fam == "ppo_std")["bytes"]
        a = {k: address(B * A) for k in ("mu", "actions", "old_mu", "old_sigma", "g_mu")}
        a.update({k: address(B) for k in ("value", "old_logp", "adv", "returns", "tv", "g_value")})
        a.update(sigma=address(A if fam == "ppo_std" else B * A), g_sigma=address(A if fam == "ppo_std" else B * A), out5=address(5), batch=B, A=A, clip=PPO_CLIP,
                 cv=PPO_CV, ce=PPO_CE, clipped=1)
    else:
        n = sh["count"]
        numel = list(sh["numel"])
        if "numel0" in edits:
            numel[edits["numel0"]] = 0
        nbytes = adam_bytes(n)
        tabs = {k: [address(max(x, 1)) for x in sh["numel"]] for k in ("p", "g", "m", "v")}
        tabs["step"] = [address(1) for _ in range(n)]
        if "null_entry" in edits:
            tabs[edits["null_entry"][0]][edits["null_entry"][1]] = None
        wd = [0.0] * n
        if "wd_neg" in edits:
            wd[edits["wd_neg"]] = -0.5
        a = {k: (ctypes.c_void_p * n)(*v) for k, v in tabs.items()}
        a.update(count=n, numel=(ctypes.c_int64 * n)(*numel), wd=(ctypes.c_float * n)(*wd), clip_count=2, lr_dev=None, lr_host=ADAM_LR, b1=ADAM_B1, b2=ADAM_B2,
                 eps=ADAM_EPS, max_norm=0.5, norm_out=address(1))
    a.update(ws=address(nbytes // 4), ws_bytes=nbytes - edits.get("short", 0), stream=None)
    a.update(edits.get("set", {}))
    for k, off in edits.get("off", {}).items():
        a[k] += off
    if "null" in edits:
        a[edits["null"]] = None
    return getattr(L, fn)(*[a[k] for k in names])
