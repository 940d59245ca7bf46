"""fp64 numpy statement of the fused MLP launches -- lsim_policy_forward and its act / post / ext forms, lsim_amp_step, lsim_actor_input --
written from include/lsim.h, not from the kernels; their cases; an independent packer into the header's 16 x 16-block layout; a restatement of
the launch plan (which wave owns which output tiles, which template width, how the k loop splits) so that a CPU test can assert that the cases
reach every path; and the mutants a test of these launches has to see.

One set of formulas serves the reference (float64, numpy's matmul), the fp32 twins of DESIGN 7.12's tolerance rule (float32 with forward,
reversed and 16-chunked summation) and the mutants: `dtype` and `mm` are arguments.
"""
import numpy as np

# ---------------------------------------------------------------------------------------------------------------------------------------
# cases
POLICY_CASES = {
    #            O = hist x n1
    "shipped": dict(hist=6, n1=45, P=238, enc=(128, 64), latent=16, actor=(512, 256, 128), A=12, critic=(512, 256, 128), ext=None),
    "tiny":    dict(hist=2, n1=5, P=7, enc=(16, 16), latent=1, actor=(16, 16, 16), A=1, critic=(16, 16, 16), ext=None),
    "ragged":  dict(hist=3, n1=29, P=100, enc=(300, 40), latent=7, actor=(300, 200, 100), A=16, critic=(400, 272, 24), ext=None),
    "ext":     dict(hist=2, n1=32, P=80, enc=(80, 272), latent=13, actor=(336, 96, 64), A=5, critic=(512, 48, 80), ext=(23, 25)),
}
POLICY_ENVS = (1, 19, 2047, 2048, 2053)      # one row; a ragged second 16-row block; the last narrow and the first wide launch; a ragged 32-row block
AMP_CASES = {"shipped": (30, (1024, 512)), "small": (3, (40, 24)), "wide": (32, (1000, 520)), "odd": (17, (600, 300))}
AMP_ENVS = (37, 4096, 6150)                  # two blocks per row group (ragged, full) and one
ACTOR_INPUT_CASES = ((45, 16), (29, 7), (5, 1), (48, 16))
ACTOR_INPUT_BATCHES = (1, 37, 257)

POLICY_CLASSES_8 = {"full1", "full2", "full4", "part2_1", "part4_1", "part4_2", "part4_3", "idle"}
POLICY_CLASSES_16 = {"full1", "full2", "part2_1", "idle"}
POLICY_K_CLASSES = {"chunks1", "chunks2", "chunks3", "chunks4", "loop_tail2", "loop_tail3", "loop_tail4"}
AMP_CLASSES = {"t0_last_full2", "t0_last_part2_1", "t0_last_idle", "t1_per1_valid1", "t1_per1_valid0", "t1_per2_valid2", "t1_per2_valid1",
               "t1_per2_valid0", "t1_odd_split", "forced_nsplit2"}      # t1_per2_valid1: the predicated ls_amp_layer_head<2, RH, false>


def pad16(v):
    return (v + 15) // 16 * 16


def policy_dims(case):
    """{network: [(k_in, n_out), ...]} of a policy case"""
    c = POLICY_CASES[case]
    chain = lambda sizes: [(sizes[i], sizes[i + 1]) for i in range(len(sizes) - 1)]
    ext = c["ext"][0] if c["ext"] else 0
    return {"encoder": chain([c["hist"] * c["n1"], *c["enc"], c["latent"] + 3]),
            "actor": chain([c["n1"] + 3 + c["latent"] + ext, *c["actor"], c["A"]]),
            "critic": chain([c["P"], *c["critic"], 1])}


def amp_dims(case):
    D, (h1, h2) = AMP_CASES[case]
    return [(2 * D, h1), (h1, h2)]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the launch plan, restated (csrc/ls_policy.h: ls_pol_split, ls_pol_run_layer, the k loop of ls_pol_accumulate; csrc/ls_amp.h: the trunk
# passes, the split of trunk[1], ls_amp_nsplit)
def pol_split(n_pad, waves):
    """[(tile0, valid)] per wave and `per`, for a layer of n_pad outputs"""
    tiles = n_pad // 16
    per = (tiles + waves - 1) // waves
    return per, [(w * per, max(0, min(per, tiles - w * per))) for w in range(waves)]


def pol_ntw(per, waves):
    if 32 // waves > 2 and per > 2:
        return 4
    return 2 if per > 1 else 1


def _cls(ntw, valid):
    return "idle" if valid == 0 else ("full%d" % ntw if valid == ntw else "part%d_%d" % (ntw, valid))


def pol_layer_classes(n_pad, waves):
    per, split = pol_split(n_pad, waves)
    assert per <= (4 if waves == 8 else 2), "more tiles per wave than the widest template"
    return {_cls(pol_ntw(per, waves), v) for _, v in split}


def k_plan(k_pad):
    """(iterations of the unguarded three-chunk steady state, chunks of the guarded tail)"""
    kc = steady = 0
    while kc + 80 <= k_pad:
        kc += 48
        steady += 1
    tail = (k_pad - kc) // 16
    assert 1 <= tail <= 4
    return steady, tail


def k_class(k_pad):
    steady, tail = k_plan(k_pad)
    return ("chunks%d" if steady == 0 else "loop_tail%d") % tail


def policy_plan(case):
    """{"encoder0": {8: classes, 16: classes, "k": k class}, ...} for the eleven layers of a case"""
    out = {}
    for name, layers in policy_dims(case).items():
        for i, (k_in, n_out) in enumerate(layers):
            out["%s%d" % (name, i)] = {8: pol_layer_classes(pad16(n_out), 8), 16: pol_layer_classes(pad16(n_out), 16), "k": k_class(pad16(k_in))}
    return out


def policy_plan_union(case):
    """({8: classes, 16: classes}, k classes) over the layers of a case"""
    plan = policy_plan(case)
    return {w: set().union(*(p[w] for p in plan.values())) for w in (8, 16)}, {p["k"] for p in plan.values()}


AMP_ROWS, AMP_WAVES = 32, 16


def amp_nsplit(case, num_envs):
    """blocks per row group, without the A/B environment switch; 0: refused"""
    tiles = pad16(AMP_CASES[case][1][1]) // 16
    ns = 2 if (num_envs + AMP_ROWS - 1) // AMP_ROWS <= 192 else 1
    if (tiles + ns - 1) // ns > 2 * AMP_WAVES:
        ns = 2
    return 0 if (tiles + ns - 1) // ns > 2 * AMP_WAVES else ns


def amp_trunk0_last_pass(case):
    """the per-wave classes of trunk[0]'s last pass (two tiles per wave and pass)"""
    tiles = pad16(AMP_CASES[case][1][0]) // 16
    base = (tiles - 1) // (2 * AMP_WAVES) * (2 * AMP_WAVES)
    return {_cls(2, max(0, min(2, tiles - base - 2 * w))) for w in range(AMP_WAVES)}


def amp_trunk1(case, nsplit):
    """(share, per, [[valid per wave] per split], [tile range per split])"""
    tiles = pad16(AMP_CASES[case][1][1]) // 16
    share = (tiles + nsplit - 1) // nsplit
    per = (share + AMP_WAVES - 1) // AMP_WAVES
    valid, ranges = [], []
    for s in range(nsplit):
        first = s * share
        mine = min(share, tiles - first)
        valid.append([max(0, min(per, first + mine - (first + w * per))) for w in range(AMP_WAVES)])
        ranges.append((first, first + mine))
    return share, per, valid, ranges


def amp_plan(case, num_envs):
    ns = amp_nsplit(case, num_envs)
    tiles = pad16(AMP_CASES[case][1][1]) // 16
    out = set()
    last = amp_trunk0_last_pass(case)
    if last == {"full2"}:
        out.add("t0_last_full2")
    if "part2_1" in last:
        out.add("t0_last_part2_1")
    if "idle" in last:
        out.add("t0_last_idle")
    share, per, valid, _ = amp_trunk1(case, ns)
    for row in valid:
        for v in row:
            out.add("t1_per%d_valid%d" % (per, v))
    if ns == 2 and tiles % 2:
        out.add("t1_odd_split")
    if ns == 2 and (num_envs + AMP_ROWS - 1) // AMP_ROWS > 192:
        out.add("forced_nsplit2")
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the independent packer: include/lsim.h, weight[(n / 16) * (k_pad / 16) + k / 16][n % 16][k % 16], zero filled; bias [n_pad]
def pack_layer(W, b):
    W, b = np.asarray(W, dtype=np.float32), np.asarray(b, dtype=np.float32)
    n_out, k_in = W.shape
    n_pad, k_pad = pad16(n_out), pad16(k_in)
    flat = np.zeros(n_pad * k_pad, dtype=np.float32)
    n, k = np.arange(n_out)[:, None], np.arange(k_in)[None, :]
    flat[((n // 16) * (k_pad // 16) + k // 16) * 256 + (n % 16) * 16 + (k % 16)] = W
    bias = np.zeros(n_pad, dtype=np.float32)
    bias[:n_out] = b
    return {"weight": flat, "bias": bias, "k_pad": k_pad, "n_pad": n_pad, "k_in": k_in, "n_out": n_out}


def pack_policy(net):
    """{network: [packed layer]} from {network: [(W [n_out, k_in], b)]}"""
    return {name: [pack_layer(W, b) for W, b in layers] for name, layers in net.items()}


def pack_amp(disc):
    out = {"hidden": [pack_layer(W, b) for W, b in disc["hidden"]]}
    hw = np.zeros(out["hidden"][1]["n_pad"], dtype=np.float32)
    hw[:disc["head_w"].size] = disc["head_w"]
    out["head_w"], out["head_b"] = hw, np.asarray(disc["head_b"], dtype=np.float32).reshape(1)
    return out


def _fill_layer(dst, pl, address):
    dst.weight, dst.bias = address(pl["weight"]), address(pl["bias"])
    dst.k_pad, dst.n_pad, dst.k_in, dst.n_out = pl["k_pad"], pl["n_pad"], pl["k_in"], pl["n_out"]


def policy_struct(case, packed, address):
    """lsim_him_policy over the packed arrays; address(array) -> the address the library is to read it at"""
    from isaacgymloco_amd import abi
    c = POLICY_CASES[case]
    P = abi.LsimHimPolicy()
    for name in ("encoder", "actor", "critic"):
        for i, pl in enumerate(packed[name]):
            _fill_layer(getattr(P, name)[i], pl, address)
    P.num_obs, P.num_priv_obs, P.num_one_step_obs, P.num_actions = c["hist"] * c["n1"], c["P"], c["n1"], c["A"]
    return P


def amp_struct(case, packed, address, coef, lerp, norm=None):
    from isaacgymloco_amd import abi
    D = abi.LsimAmpDisc()
    for i, pl in enumerate(packed["hidden"]):
        _fill_layer(D.hidden[i], pl, address)
    D.head_weight, D.head_bias = address(packed["head_w"]), address(packed["head_b"])
    D.amp_dim = AMP_CASES[case][0]
    D.reward_coef, D.task_reward_lerp = float(coef), float(lerp)
    if norm is not None:
        D.norm_mean, D.norm_var, D.norm_eps, D.norm_clip = address(norm["mean"]), address(norm["var"]), float(norm["eps"]), float(norm["clip"])
    return D


# ---------------------------------------------------------------------------------------------------------------------------------------
# summation orders of the fp32 twins
def mm_blas(x, W):
    return x @ W.T


def _mm_seq(x, W, order):
    acc = np.zeros((x.shape[0], W.shape[0]), dtype=x.dtype)
    for k in order:
        acc += x[:, k:k + 1] * W[:, k][None, :]
    return acc


def mm_forward(x, W):
    return _mm_seq(x, W, range(W.shape[1]))


def mm_reversed(x, W):
    return _mm_seq(x, W, range(W.shape[1] - 1, -1, -1))


def mm_chunk16(x, W):
    acc = np.zeros((x.shape[0], W.shape[0]), dtype=x.dtype)
    for k0 in range(0, W.shape[1], 16):
        acc += _mm_seq(x[:, k0:k0 + 16], W[:, k0:k0 + 16], range(min(16, W.shape[1] - k0)))
    return acc


TWINS = (("forward", mm_forward), ("reversed", mm_reversed), ("chunk16", mm_chunk16))


def _elu(x):
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))


def _cast_net(layers, dtype):
    return [(np.asarray(W, dtype=dtype), np.asarray(b, dtype=dtype)) for W, b in layers]


# ---------------------------------------------------------------------------------------------------------------------------------------
# mutants: what a subtly wrong kernel would compute.  Each names the launch it belongs to and the general case on which a test must see it.
MUTANTS = {
    "drop_last_chunk": dict(launch="policy", case="ragged"),     # the last k chunk of one output tile (second actor and critic layer, last tile)
    "no_bias":         dict(launch="policy", case="ragged"),     # that tile's bias missing
    "swizzle_slip":    dict(launch="policy", case="tiny"),       # rows 4-7 of a 16-row block: 4-float groups 0 and 1 of the first chunk exchanged
    "latent_short":    dict(launch="policy", case="ragged"),     # the latent normalised over nl - 1 terms
    "extra_shift":     dict(launch="policy", case="ext"),        # the extra segment one column late
    "elu_last":        dict(launch="policy", case="shipped"),    # ELU behind the last layer
    "split1_twice":    dict(launch="amp", case="odd"),           # split 1's tiles of trunk[1] counted twice
    "patch_carry":     dict(launch="amp", case="small"),         # the terminal patch applied to the carry
}


def mutant_touches(mutant, case, num_envs, exact):
    """can `mutant` change an output of this scene at all?"""
    if mutant == "swizzle_slip":
        return num_envs > 4
    if mutant == "latent_short":
        return not exact                 # an exact scene's first actor layer is zero on the latent columns
    if mutant == "elu_last":
        return not exact                 # an exact scene's outputs are >= 0: ELU is the identity
    if mutant == "extra_shift":
        return POLICY_CASES[case]["ext"] is not None
    if mutant == "split1_twice":
        return amp_nsplit(case, num_envs) == 2
    return True


def _layer(x, W, b, tag, mm, mutant):
    if mutant == "swizzle_slip" and tag in ("actor1", "critic1"):
        x = x.copy()
        rows = np.nonzero((np.arange(x.shape[0]) % 16) // 4 == 1)[0]
        x[np.ix_(rows, np.arange(8))] = x[np.ix_(rows, np.r_[4:8, 0:4])]
    y = mm(x, W) + b
    if mutant in ("drop_last_chunk", "no_bias") and tag in ("actor1", "critic1"):
        t0 = (W.shape[0] - 1) // 16 * 16                       # the last output tile
        if mutant == "no_bias":
            y[:, t0:] = mm(x, W[t0:])
        else:
            kl = (W.shape[1] - 1) // 16 * 16                   # the last k chunk starts here
            y[:, t0:] = (mm(x[:, :kl], W[t0:, :kl]) if kl else 0) + b[t0:]
    return y


def _mlp(x, layers, name, mm, mutant):
    for i, (W, b) in enumerate(layers):
        x = _layer(x, W, b, "%s%d" % (name, i), mm, mutant)
        if i + 1 < len(layers):
            x = _elu(x)
    return x


def _sumsq(z, mm):
    if mm is mm_blas:
        return (z * z).sum(axis=1)
    order = range(z.shape[1] - 1, -1, -1) if mm is mm_reversed else range(z.shape[1])
    s = np.zeros(z.shape[0], dtype=z.dtype)
    for k in order:
        s += z[:, k] * z[:, k]
    return s


def actor_input(obs_now, enc_out, dtype=np.float64, mm=mm_blas, mutant=None):
    """lsim_actor_input: [obs_now | enc_out[:, :3] | enc_out[:, 3:] / max(||.||, 1e-12)]"""
    obs_now, enc_out = np.asarray(obs_now, dtype=dtype), np.asarray(enc_out, dtype=dtype)
    z = enc_out[:, 3:]
    zn = z[:, :-1] if mutant == "latent_short" else z
    norm = np.maximum(np.sqrt(_sumsq(zn, mm)), dtype(1e-12))
    return np.concatenate((obs_now, enc_out[:, :3], z / norm[:, None]), axis=1)


def policy_forward(case, net, obs, priv, extra=None, dtype=np.float64, mm=mm_blas, mutant=None):
    """HAC:136-163 as include/lsim.h states it -> (mean [N, A], values [N, 1]); extra: [N, dim] or None"""
    c = POLICY_CASES[case]
    enc, act, cri = (_cast_net(net[k], dtype) for k in ("encoder", "actor", "critic"))
    obs, priv = np.asarray(obs, dtype=dtype), np.asarray(priv, dtype=dtype)
    out = _mlp(obs, enc, "encoder", mm, mutant)
    x = actor_input(obs[:, :c["n1"]], out, dtype, mm, mutant)
    if c["ext"]:
        e = np.asarray(extra, dtype=dtype)
        assert e.shape == (obs.shape[0], c["ext"][0])
        if mutant == "extra_shift":
            e = np.concatenate((np.zeros((e.shape[0], 1), dtype=dtype), e[:, :-1]), axis=1)
        x = np.concatenate((x, e), axis=1)
    mean, val = _mlp(x, act, "actor", mm, mutant), _mlp(priv, cri, "critic", mm, mutant)
    if mutant == "elu_last":
        mean, val = _elu(mean), _elu(val)
    return mean, val


def amp_step(case, disc, prev, nxt, dones, term, task, coef, lerp, norm=None, replay=None, dtype=np.float64, mm=mm_blas, mutant=None, nsplit=1):
    """lsim_amp_step -> dict(d, reward, carry, replay_s, replay_ns).  replay: (states, next_states, cursor) or None; norm: dict(mean, var float64,
    eps, clip) or None.  nsplit only matters to the split1_twice mutant."""
    prev32, nxt32 = np.asarray(prev, dtype=np.float32), np.asarray(nxt, dtype=np.float32)
    patched = np.where(np.asarray(dones, dtype=bool)[:, None], np.asarray(term, dtype=np.float32), nxt32) if dones is not None else nxt32
    out = {"carry": (patched if mutant == "patch_carry" else nxt32).copy()}
    if replay is not None:
        rs, rns, cursor = replay[0].copy(), replay[1].copy(), replay[2]
        slots = (cursor + np.arange(prev32.shape[0])) % rs.shape[0]
        rs[slots], rns[slots] = prev32, patched
        out["replay_s"], out["replay_ns"] = rs, rns

    def normalise(x):
        x = x.astype(dtype)
        if norm is None:
            return x
        m = norm["mean"].astype(np.float32).astype(dtype)                         # UT:124-130: float32(mean), sqrt(float32(var + eps)), clamp
        sd = np.sqrt((norm["var"] + norm["eps"]).astype(np.float32)).astype(dtype)
        return np.clip((x - m) / sd, dtype(-norm["clip"]), dtype(norm["clip"]))
    x = np.concatenate((normalise(prev32), normalise(patched)), axis=1)
    (W0, b0), (W1, b1) = _cast_net(disc["hidden"], dtype)
    h1 = np.maximum(mm(x, W0) + b0, 0)
    h2 = np.maximum(mm(h1, W1) + b1, 0)
    hw = np.asarray(disc["head_w"], dtype=dtype).reshape(1, -1)
    d = mm(h2, hw)[:, 0]
    if mutant == "split1_twice" and nsplit == 2:
        lo, hi = amp_trunk1(case, 2)[3][1]
        lo, hi = 16 * lo, min(16 * hi, h2.shape[1])
        d = d + mm(h2[:, lo:hi], hw[:, lo:hi])[:, 0]
    d = d + dtype(np.asarray(disc["head_b"]).reshape(-1)[0])
    e = d - dtype(1)
    r = dtype(coef) * np.maximum(dtype(1) - dtype(0.25) * (e * e), 0)
    if lerp > 0:
        r = dtype(1.0 - lerp) * r + dtype(lerp) * np.asarray(task, dtype=dtype)
    out["d"], out["reward"] = d, r
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# exact scenes: small integers, every fp32 partial sum in any order exact
def _int_weight(n_out, k_in, zero_cols=(), signed=False):
    """one unit weight per row and k chunk at a drawn column of the chunk (a regular pattern makes later layers blind to a permutation inside
    a chunk); then repaired until every 16 x 16 block, every row and every (non-excluded) column holds a nonzero"""
    n, k = np.arange(n_out)[:, None], np.arange(k_in)[None, :]
    rs = np.random.RandomState(31 * n_out + k_in)
    W = np.zeros((n_out, k_in), dtype=np.int64)
    for ch in range(0, k_in, 16):
        W[np.arange(n_out), ch + rs.randint(0, min(16, k_in - ch), size=n_out)] = 1
    keep = np.ones(k_in, dtype=bool)
    keep[list(zero_cols)] = False
    W[:, ~keep] = 0
    cols = np.nonzero(keep)[0]
    for r in range(n_out):
        if not W[r].any():
            W[r, cols[r % cols.size]] = 1
    for col in cols:
        if not W[:, col].any():
            W[col % n_out, col] = 1
    for t in range(0, n_out, 16):
        for ch in range(0, k_in, 16):
            blk_cols = [q for q in range(ch, min(ch + 16, k_in)) if keep[q]]
            if blk_cols and not W[t:t + 16, ch:ch + 16].any():
                W[t, blk_cols[0]] = 1
    if signed:
        W = W * np.where((n + 2 * k) % 3 == 0, -1, 1)
    return W


def _int_bias(n_out, signed=False):
    b = 1 + np.arange(n_out) % 5
    return b - 3 if signed else b


def exact_policy_scene(case, num_envs):
    """(net, obs, priv, extra [N, ld] with NaN padding or None) of integers; the bound is asserted by check_exact_policy"""
    c = POLICY_CASES[case]
    dims = policy_dims(case)
    lat0 = c["n1"] + 3
    net = {}
    for name, layers in dims.items():
        net[name] = []
        for i, (k_in, n_out) in enumerate(layers):
            zero = range(lat0, lat0 + c["latent"]) if (name == "actor" and i == 0) else ()
            net[name].append((_int_weight(n_out, k_in, zero), _int_bias(n_out)))
    hi = 2 if case == "shipped" else 4
    rs = np.random.RandomState(1000 + num_envs)
    obs = rs.randint(0, hi, size=(num_envs, c["hist"] * c["n1"]))
    priv = rs.randint(0, hi, size=(num_envs, c["P"]))
    extra = None
    if c["ext"]:
        extra = np.full((num_envs, c["ext"][1]), np.nan)
        extra[:, :c["ext"][0]] = rs.randint(0, hi, size=(num_envs, c["ext"][0]))
    return net, obs, priv, extra


def _check_int_layers(x, layers, what, relu=False, stop_relu_last=True):
    """the int64 chain with sum |W| |x| + |b| < 2^24 asserted per layer; returns the last layer's output"""
    x = np.asarray(x, dtype=np.int64)
    for i, (W, b) in enumerate(layers):
        W, b = np.asarray(W, dtype=np.int64), np.asarray(b, dtype=np.int64)
        # the integer products through float64 BLAS: exact below 2^53, and numpy's own int64 matmul is a scalar loop
        bound = int((np.abs(x).astype(np.float64) @ np.abs(W).T.astype(np.float64) + np.abs(b)).max())
        assert bound < 2 ** 24, (what, i, bound)
        x = (x.astype(np.float64) @ W.T.astype(np.float64)).astype(np.int64) + b
        if relu:
            x = np.maximum(x, 0)
        else:
            assert (x >= 0).all(), (what, i, "a negative pre-activation: ELU would not be the identity")
    return x


def check_exact_policy(case, net, obs, priv, extra):
    """asserts what makes the scene exact and returns (mean, values) as int64"""
    c = POLICY_CASES[case]
    lat0 = c["n1"] + 3
    for name, layers in net.items():
        for i, (W, b) in enumerate(layers):
            excl = set(range(lat0, lat0 + c["latent"])) if (name == "actor" and i == 0) else set()
            assert all(W[r].any() for r in range(W.shape[0])), (name, i, "an output row without a weight")
            assert all(W[:, k].any() for k in range(W.shape[1]) if k not in excl) and not W[:, sorted(excl)].any(), (name, i, "columns")
            for t in range(0, W.shape[0], 16):
                for ch in range(0, W.shape[1], 16):
                    if not set(range(ch, min(ch + 16, W.shape[1]))) <= excl:
                        assert W[t:t + 16, ch:ch + 16].any(), (name, i, t, ch, "an all-zero block")
    obs, priv = np.asarray(obs, dtype=np.int64), np.asarray(priv, dtype=np.int64)
    enc = _check_int_layers(obs, net["encoder"], case + " encoder")
    x = np.concatenate((obs[:, :c["n1"]], enc[:, :3], np.zeros((obs.shape[0], c["latent"]), dtype=np.int64)), axis=1)     # zero weights there
    if c["ext"]:
        x = np.concatenate((x, extra[:, :c["ext"][0]].astype(np.int64)), axis=1)
    return _check_int_layers(x, net["actor"], case + " actor"), _check_int_layers(priv, net["critic"], case + " critic")


def exact_amp_scene(case, num_envs):
    """signed integers (ReLU is exact), no normaliser; head bias chosen so that some rows land on the reward's parabola"""
    D, _ = AMP_CASES[case]
    dims = amp_dims(case)
    disc = {"hidden": [(_int_weight(n, k, signed=True), _int_bias(n, signed=True)) for k, n in dims]}
    h2 = dims[1][1]
    disc["head_w"] = np.where(np.arange(h2) % 2 == 0, 1, -1).astype(np.int64)
    rs = np.random.RandomState(2000 + num_envs)
    prev, nxt, term = (rs.randint(-3, 4, size=(num_envs, D)) for _ in range(3))
    dones = rs.rand(num_envs) < 0.25
    task = rs.randint(-2, 3, size=num_envs)
    patched = np.where(dones[:, None], term, nxt)
    h = _check_int_layers(np.concatenate((prev, patched), axis=1), disc["hidden"], case + " trunk", relu=True)
    assert int((np.abs(h) @ np.abs(disc["head_w"])).max()) < 2 ** 24 - 2 ** 20
    raw = h @ disc["head_w"]
    disc["head_b"] = np.array([1 - int(np.median(raw))], dtype=np.int64)
    assert abs(int(disc["head_b"][0])) < 2 ** 20
    return disc, prev, nxt, dones, term, task, raw + disc["head_b"][0]
