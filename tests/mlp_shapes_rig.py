"""Scenes, tolerances and launches for the fused MLP shape tests (tests/mlp_shapes_reference.py holds the reference, the cases and the packer).

General scenes come from the project's own torch modules built at a case's widths and perturbed from their init; their tolerance is DESIGN
7.12's rule: per output tensor 4 x the largest distance from the fp64 reference of fp32 twins of the same formulas (numpy float32, forward,
reversed and 16-chunked summation) -- computed on the CPU for the case, never from what a kernel returns.  The twins run on the first TWIN_ROWS
rows of a case's inputs (their cost is a python loop over k); every env count of the case uses leading rows of the same inputs.
"""
import ctypes
import functools

import numpy as np
import torch

import mlp_shapes_reference as R

TWIN_ROWS = 256
MAX_ROWS = {"policy": max(R.POLICY_ENVS), "amp": max(R.AMP_ENVS)}
AMP_COEF, AMP_LERP = 0.01, 0.3
_SEEDS = {"shipped": 3, "tiny": 5, "ragged": 7, "ext": 11, "small": 13, "wide": 17, "odd": 19}


# ---- torch modules at a case's widths -------------------------------------------------------------------------------------------------
def policy_module(case, seed=None, perturb=0.05):
    """HIMActorCritic (VisionActorCritic for a case with an extra segment) with the case's encoder, actor and critic widths, on the CPU"""
    from isaacgymloco_amd.learn import modules as M
    from isaacgymloco_amd.learn.vision import VisionActorCritic
    c = R.POLICY_CASES[case]
    torch.manual_seed(_SEEDS[case] if seed is None else seed)
    O = c["hist"] * c["n1"]
    kw = dict(actor_hidden_dims=c["actor"], critic_hidden_dims=c["critic"])
    if c["ext"]:
        ac = VisionActorCritic(O, c["P"], c["n1"], c["A"], depth_latent_dim=c["ext"][0], **kw)
    else:
        ac = M.HIMActorCritic(O, c["P"], c["n1"], c["A"], **kw)
    ac.estimator = M.HIMEstimator(c["hist"], c["n1"], enc_hidden_dims=(*c["enc"], c["latent"]))
    k = c["n1"] + 3 + c["latent"]
    if c["ext"]:
        ac.num_him_actor_inputs = k
        k += c["ext"][0]
    ac.actor = M.mlp([k, *c["actor"], c["A"]], M.get_activation("elu"))
    with torch.no_grad():
        for p in ac.parameters():
            p.add_(perturb * torch.randn_like(p))
    return ac


def _pairs(seq):
    return [(m.weight.detach().cpu().numpy().copy(), m.bias.detach().cpu().numpy().copy()) for m in seq if isinstance(m, torch.nn.Linear)]


def net_of(ac):
    return {"encoder": _pairs(ac.estimator.encoder), "actor": _pairs(ac.actor), "critic": _pairs(ac.critic)}


def amp_module(case, seed=None, perturb=0.05):
    from isaacgymloco_amd.learn import amp
    D, hidden = R.AMP_CASES[case]
    torch.manual_seed(_SEEDS[case] if seed is None else seed)
    d = amp.AMPDiscriminator(2 * D, AMP_COEF, list(hidden), "cpu", AMP_LERP)
    with torch.no_grad():
        for p in d.parameters():
            p.add_(perturb * torch.randn_like(p))
    return d


def disc_of(d):
    return {"hidden": _pairs(d.trunk), "head_w": d.amp_linear.weight.detach().numpy().reshape(-1).copy(), "head_b": d.amp_linear.bias.detach().numpy().copy()}


# ---- general scenes and their tolerances ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def general_policy_scene(case, zero_latent=False):
    """dict(net, obs, priv, extra [N, ld] NaN padded or None, ref (mean, val) fp64, tol (mean, val), twin_dist) at MAX_ROWS rows"""
    c = R.POLICY_CASES[case]
    ac = policy_module(case)
    net = net_of(ac)
    if zero_latent:                       # the encoder's latent rows and biases zero: z = 0 exactly, the normalisation divides 0 by 1e-12
        W, b = net["encoder"][2]
        W[3:], b[3:] = 0.0, 0.0
    g = torch.Generator().manual_seed(100 + _SEEDS[case])
    N = MAX_ROWS["policy"]
    obs = (2.0 * torch.randn(N, c["hist"] * c["n1"], generator=g)).numpy()
    priv = (2.0 * torch.randn(N, c["P"], generator=g)).numpy()
    extra = None
    if c["ext"]:
        extra = np.full((N, c["ext"][1]), np.nan, dtype=np.float32)
        extra[:, :c["ext"][0]] = (2.0 * torch.randn(N, c["ext"][0], generator=g)).numpy()
    dense = None if extra is None else extra[:, :c["ext"][0]]
    ref = R.policy_forward(case, net, obs, priv, dense)
    T = TWIN_ROWS
    dist = [0.0, 0.0]
    for name, mm in R.TWINS:
        tw = R.policy_forward(case, net, obs[:T], priv[:T], None if dense is None else dense[:T], dtype=np.float32, mm=mm)
        for i in range(2):
            d = float(np.abs(tw[i].astype(np.float64) - ref[i][:T]).max())
            print("policy", case, "zero latent" if zero_latent else "plain", ("mean", "values")[i], "twin", name, "distance", d)
            dist[i] = max(dist[i], d)
    return dict(net=net, obs=obs, priv=priv, extra=extra, ref=ref, tol=(4.0 * dist[0], 4.0 * dist[1]), twin_dist=tuple(dist))


@functools.lru_cache(maxsize=None)
def general_amp_scene(case):
    D, _ = R.AMP_CASES[case]
    disc = disc_of(amp_module(case))
    g = torch.Generator().manual_seed(200 + _SEEDS[case])
    N = MAX_ROWS["amp"]
    prev, nxt, term = ((2.0 * torch.randn(N, D, generator=g)).numpy() for _ in range(3))
    prev[:, min(3, D - 1)] = 40.0                           # a column that hits the normaliser's clip
    task = torch.randn(N, generator=g).numpy()
    dones = (torch.rand(N, generator=g) < 0.2).numpy()
    norm = {"mean": (0.3 * torch.randn(D, generator=g, dtype=torch.float64)).numpy(), "var": (0.5 + torch.rand(D, generator=g, dtype=torch.float64)).numpy(),
            "eps": 1e-4, "clip": 10.0}
    ref = R.amp_step(case, disc, prev, nxt, dones, term, task, AMP_COEF, AMP_LERP, norm)
    T = TWIN_ROWS
    dist = {"d": 0.0, "reward": 0.0}
    for name, mm in R.TWINS:
        tw = R.amp_step(case, disc, prev[:T], nxt[:T], dones[:T], term[:T], task[:T], AMP_COEF, AMP_LERP, norm, dtype=np.float32, mm=mm)
        for k in dist:
            d = float(np.abs(tw[k].astype(np.float64) - ref[k][:T]).max())
            print("amp", case, k, "twin", name, "distance", d)
            dist[k] = max(dist[k], d)
    return dict(disc=disc, prev=prev, nxt=nxt, term=term, task=task, dones=dones, norm=norm, ref=ref, tol={k: 4.0 * v for k, v in dist.items()}, twin_dist=dist)


def actor_input_scene(n1, latent, batch):
    """(obs [B, ld] and enc [B, ld] with NaN in the unused columns, ref fp64, tolerance of the normalised columns); row B // 2 has a zero latent
    where there is more than one row.  A latent of one column normalises to +-1 exactly in every fp32 order: its twin distance is 0"""
    rs = np.random.RandomState(300 + 7 * n1 + latent + batch)
    obs = np.full((batch, n1 + 5), np.nan, dtype=np.float32)
    enc = np.full((batch, 3 + latent + 3), np.nan, dtype=np.float32)
    obs[:, :n1] = 2.0 * rs.randn(batch, n1)
    enc[:, :3 + latent] = 2.0 * rs.randn(batch, 3 + latent)
    if batch > 1:
        enc[batch // 2, 3:3 + latent] = 0.0
    ref = R.actor_input(obs[:, :n1], enc[:, :3 + latent])
    dist = 0.0
    for name, mm in R.TWINS:
        tw = R.actor_input(obs[:, :n1], enc[:, :3 + latent], dtype=np.float32, mm=mm)
        dist = max(dist, float(np.abs(tw.astype(np.float64) - ref)[:, n1 + 3:].max()))
    print("actor input", (n1, latent, batch), "twin distance", dist)
    return obs, enc, ref, 4.0 * dist


# ---- structs on host memory (refusal tests: the library answers before any HIP call) --------------------------------------------------------
class HostArrays:
    """keeps the arrays a struct points at alive; address() of a numpy array is its host address"""

    def __init__(self):
        self.keep = []

    def address(self, a):
        assert a.ctypes.data % 16 == 0
        self.keep.append(a)
        return a.ctypes.data


def host_policy(case, num_envs=4):
    """(struct, keep-alive, (obs, priv, mean, values) host arrays) of the case's exact scene: a struct the library would accept"""
    net, obs, priv, _ = R.exact_policy_scene(case, num_envs)
    h = HostArrays()
    P = R.policy_struct(case, R.pack_policy(net), h.address)
    c = R.POLICY_CASES[case]
    bufs = (obs.astype(np.float32), priv.astype(np.float32), np.full((num_envs, c["A"]), 7.25, dtype=np.float32), np.full((num_envs, 1), 7.25, dtype=np.float32))
    return P, h, bufs


# ---- launches on the device ----------------------------------------------------------------------------------------------------------
DEV = "cuda:0"


class DeviceArrays:
    """uploads each packed array once; address() is its device address; update() overwrites a device copy in place"""

    def __init__(self):
        self.t = {}

    def address(self, a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        self.t[id(a)] = (a, t)
        return t.data_ptr()

    def tensor(self, a):
        return self.t[id(a)][1]


def guarded(shape, dtype=torch.float32, fill=float("nan"), guard=64):
    """(view of `shape`, the flat buffer with `guard` elements in front and behind): everything starts as `fill`"""
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * guard,), fill, dtype=dtype, device=DEV)
    return flat[guard:guard + n].view(*shape), flat


def guards_intact(flat, n, guard=64):
    return bool(torch.isnan(flat[:guard]).all()) and bool(torch.isnan(flat[guard + n:]).all())


def bits(t):
    return t.contiguous().view(torch.int32)


class DevicePolicy:
    """a case's networks packed by the independent packer, on the device, behind an lsim_him_policy"""

    def __init__(self, case, net):
        from isaacgymloco_amd import lib
        self.case, self.c = case, R.POLICY_CASES[case]
        self.L = lib.load()
        self.arrays = DeviceArrays()
        self.packed = R.pack_policy(net)
        self.P = R.policy_struct(case, self.packed, self.arrays.address)

    def repack(self, net):
        """new parameters into the SAME device buffers"""
        new = R.pack_policy(net)
        for name in new:
            for old, pl in zip(self.packed[name], new[name]):
                for k in ("weight", "bias"):
                    self.arrays.tensor(old[k]).copy_(torch.from_numpy(pl[k]))

    def extra_struct(self, rows, store=None):
        from isaacgymloco_amd import abi
        x = abi.LsimPolicyExtra()
        x.rows, x.dim, x.ld = rows.data_ptr(), self.c["ext"][0], rows.shape[1]
        if store is not None:
            x.store = store.data_ptr()
        return x

    def forward_rc(self, obs, priv, mean, val, extra=None):
        s = torch.cuda.current_stream().cuda_stream
        if self.c["ext"]:
            return self.L.lsim_policy_forward_ext(ctypes.byref(self.P), ctypes.byref(self.extra_struct(extra)), obs.data_ptr(), priv.data_ptr(), obs.shape[0],
                                                  mean.data_ptr(), val.data_ptr(), s)
        return self.L.lsim_policy_forward(ctypes.byref(self.P), obs.data_ptr(), priv.data_ptr(), obs.shape[0], mean.data_ptr(), val.data_ptr(), s)

    def forward(self, obs, priv, extra=None):
        """numpy in, numpy out; NaN guard bands around mean_out and values_out and the NaN padding of the extra rows checked"""
        n = obs.shape[0]
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
        mean, mflat = guarded((n, self.c["A"]))
        val, vflat = guarded((n, 1))
        ext = to(extra) if extra is not None else None
        rc = self.forward_rc(to(obs), to(priv), mean, val, ext)
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert guards_intact(mflat, n * self.c["A"]) and guards_intact(vflat, n), "a write outside mean_out / values_out"
        if ext is not None:
            assert bool(torch.isnan(ext[:, self.c["ext"][0]:]).all()) and torch.equal(bits(ext[:, :self.c["ext"][0]]), bits(to(extra)[:, :self.c["ext"][0]]))
        return mean.cpu().numpy(), val.cpu().numpy()


STORAGE_FIELDS = ("observations", "privileged_observations", "next_privileged_observations", "actions", "values", "actions_log_prob", "mu", "sigma", "rewards")


def storage(T, N, O, P, A):
    """the ten storage tensors, zero, each with a NaN (0xff for the u8 one) guard row of its own behind it -> (tensors, guards, struct)"""
    from isaacgymloco_amd import abi
    widths = dict(zip(STORAGE_FIELDS, (O, P, P, A, 1, 1, A, A, 1)))
    st, guards = {}, {}
    for k, d in widths.items():
        flat = torch.full(((T + 1) * N * d,), float("nan"), device=DEV)
        st[k], guards[k] = flat[:T * N * d].view(T, N, d), flat[T * N * d:]
        st[k].zero_()
    flat = torch.full(((T + 1) * N,), 0xFF, device=DEV, dtype=torch.uint8)
    st["dones"], guards["dones"] = flat[:T * N].view(T, N, 1), flat[T * N:]
    st["dones"].zero_()
    S = abi.LsimRolloutStorage()
    for k, t in st.items():
        setattr(S, k, t.data_ptr())
    S.num_steps, S.num_envs, S.num_obs, S.num_priv_obs, S.num_actions = T, N, O, P, A
    return st, guards, S


def storage_guards_intact(guards):
    return all(bool((g == 0xFF).all()) if g.dtype == torch.uint8 else bool(torch.isnan(g).all()) for g in guards.values())


class DeviceAmp:
    def __init__(self, case, disc, num_envs, norm=None, coef=AMP_COEF, lerp=AMP_LERP):
        from isaacgymloco_amd import lib
        self.case, self.D = case, R.AMP_CASES[case][0]
        self.L = lib.load()
        self.arrays = DeviceArrays()
        self.packed = R.pack_amp(disc)
        self.S = R.amp_struct(case, self.packed, self.arrays.address, coef, lerp, norm)
        n = ctypes.c_size_t(0)
        assert self.L.lsim_amp_step_workspace(int(num_envs), ctypes.byref(n)) == 0
        self.workspace = torch.zeros((n.value + 3) // 4, dtype=torch.int32, device=DEV)

    def step(self, prev, nxt, dones, term, task, cap, cursor, launches=1):
        """numpy in; dict(d, reward, carry, replay_s, replay_ns) numpy out.  The ring starts as NaN, so untouched slots show"""
        n = prev.shape[0]
        to = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)
        rew, rflat = guarded((n,))
        d, dflat = guarded((n,))
        carry, cflat = guarded((n, self.D))
        rs, rsflat = guarded((cap, self.D))
        rns, rnsflat = guarded((cap, self.D))
        args = (to(prev), to(nxt), to(dones, np.uint8), to(term), to(task))
        for _ in range(launches):
            rc = self.L.lsim_amp_step(ctypes.byref(self.S), args[0].data_ptr(), args[1].data_ptr(), args[2].data_ptr(), args[3].data_ptr(), args[4].data_ptr(), n,
                                      rew.data_ptr(), d.data_ptr(), carry.data_ptr(), rs.data_ptr(), rns.data_ptr(), cap, cursor,
                                      self.workspace.data_ptr(), self.workspace.numel() * 4, torch.cuda.current_stream().cuda_stream)
            assert rc == 0, rc
        torch.cuda.synchronize()
        for flat, cnt in ((rflat, n), (dflat, n), (cflat, n * self.D), (rsflat, cap * self.D), (rnsflat, cap * self.D)):
            assert guards_intact(flat, cnt), "a write outside an output"
        return {"d": d.cpu().numpy(), "reward": rew.cpu().numpy(), "carry": carry.cpu().numpy(), "replay_s": rs.cpu().numpy(), "replay_ns": rns.cpu().numpy()}

    def counters(self, num_envs):
        return self.workspace[:(num_envs + 31) // 32]
