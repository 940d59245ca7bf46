"""GPU: the estimator loss head, the stand-alone Sinkhorn, the clipped-PPO loss (both entries) and the clip + Adam step of csrc/ls_learn.h through the
C ABI at the small shapes of tests/loss_heads_reference.py, against the fp64 numpy statements at the tolerance their fp32 twins give.  Every launch
reads operands whose unused columns and trailing rows are NaN, works in a NaN-filled workspace of exactly the queried size between NaN guard bands,
writes its outputs between NaN guard bands, leaves its operands bit-for-bit unchanged, and is run twice: the kernels claim a fixed summation order."""
import ctypes

import numpy as np
import pytest
import torch

import loss_heads_reference as R
import mlp_shapes_rig as G
from launch_rig import NanDevice as _Device, current_stream as _stream, device_lib as _lib
import wgrad_shapes_reference as W

pytestmark = pytest.mark.gpu
DEV = G.DEV


def _rows(a, width=None):
    """a [B, w] (or [B]) operand as the flat contiguous buffer it lives in, with NaN rows behind the batch"""
    a = np.asarray(a, dtype=np.float32)
    a = a.reshape(a.shape[0], -1) if a.ndim > 1 else a.reshape(-1, 1)
    return W.padded(a, 0, a.shape[1])


class Launch:
    """the buffers of one call: operands (kept on the host for the bit comparison), guarded outputs, a guarded workspace of the queried size"""

    def __init__(self):
        self.L, self.ops, self.outs = _lib(), {}, {}

    def operand(self, name, flat, off=0):
        t = torch.from_numpy(flat).to(DEV)
        assert t.data_ptr() % 16 == 0
        self.ops[name] = (flat, t)
        return t.data_ptr() + 4 * off

    def output(self, name, shape):
        view, flat = G.guarded(shape)
        assert view.data_ptr() % 16 == 0
        self.outs[name] = (view, flat, int(np.prod(shape)))
        return view.data_ptr()

    def workspace(self, nbytes, want):
        assert nbytes == want, ("the launch plan changed: re-derive the cases of tests/loss_heads_reference.py", nbytes, want)
        self.ws, self.ws_flat = G.guarded((nbytes // 4,))
        assert self.ws.data_ptr() % 16 == 0
        return self.ws.data_ptr()

    def refill(self):
        for view, _, _ in self.outs.values():
            view.fill_(float("nan"))
        self.ws.fill_(float("nan"))

    def check_memory(self):
        assert G.guards_intact(self.ws_flat, self.ws.numel()), "a write outside the workspace"
        for name, (view, flat, n) in self.outs.items():
            assert G.guards_intact(flat, n), "a write outside " + name
            assert bool(torch.isfinite(view).all()), "NaN or Inf in %s: an unwritten element, or an operand's NaN padding reached a sum" % name
        for name, (host, t) in self.ops.items():
            assert torch.equal(G.bits(t), G.bits(torch.from_numpy(host).to(DEV))), "operand %s changed" % name

    def run(self):
        """the call, twice, from NaN-filled outputs and workspace: memory checks, both results equal to the bit -> {output: numpy}"""
        assert self.call() == 0
        torch.cuda.synchronize()
        self.check_memory()
        first = {k: v[0].clone() for k, v in self.outs.items()}
        self.refill()
        assert self.call() == 0
        torch.cuda.synchronize()
        self.check_memory()
        for k, a in first.items():
            assert torch.equal(G.bits(a), G.bits(self.outs[k][0])), "two calls on the same inputs differ in " + k
        return {k: v[0].cpu().numpy() for k, v in self.outs.items()}


def _compare(tag, case_out, got):
    """every output within its tolerance of the fp64 statement (all figures printed first)"""
    bad = []
    for k, o in case_out.items():
        err = float(np.abs(np.asarray(got[k], dtype=np.float64) - o["ref"]).max()) if o["ref"].size else 0.0
        print(tag, k, "max |device - fp64| %.3e tolerance %.3e twin distance %.3e scale %.3e" % (err, o["tol"], o["dist"], o["scale"]))
        if not err <= o["tol"]:
            bad.append((k, err, o["tol"]))
    assert not bad, (tag, bad)


# ---- the estimator loss head -----------------------------------------------------------------------------------------------------------------
class EstLaunch(Launch):
    def __init__(self, name, iters):
        super().__init__()
        B, D, K, _ = R.EST_CASES[name]
        sc = R.estimator_case(name, iters)["scene"]
        self.shape, self.iters = (B, D, K), iters
        self.ld = (3 + D + 3, D + 1, 5)                               # pitches wider than the rows; the views start 1, 0 and 2 floats into their buffers
        enc = self.operand("enc", W.padded(sc["enc"], 1, self.ld[0]), 1)
        tgt = self.operand("tgt", W.padded(sc["tgt"], 0, self.ld[1]))
        vel = self.operand("vel", W.padded(sc["vel"], 2, self.ld[2]), 2)
        proto = self.operand("proto", W.padded(sc["proto"], 0, D))
        n = ctypes.c_size_t(0)
        assert self.L.lsim_estimator_loss_workspace(B, D, K, ctypes.byref(n)) == 0
        ws = self.workspace(n.value, R.estimator_plan(B, D, K)["bytes"])
        self.args = [enc, self.ld[0], tgt, self.ld[1], proto, vel, self.ld[2], B, D, K, R.TEMPERATURE, R.SK_EPS, iters, self.output("losses", (3,)),
                     self.output("g_enc", (B, 3 + D)), self.output("g_tgt", (B, D)), self.output("g_proto", (K, D)), ws, n.value]

    def call(self):
        return self.L.lsim_estimator_loss(*self.args, _stream())


def _est_outputs(got):
    return dict(est=got["losses"][0], swap=got["losses"][1], total=got["losses"][2], d_vel=got["g_enc"][:, :3], d_lat=got["g_enc"][:, 3:], d_tgt=got["g_tgt"],
                d_proto=got["g_proto"])


@pytest.mark.parametrize("iters", R.ITERS)
@pytest.mark.parametrize("name", list(R.EST_CASES))
def test_estimator_loss_against_the_statement(name, iters):
    """all four <KMAX, DMAX>, K < 4, ragged and one-row blocks, the scalar and vector forms, `fold` both ways, the eight-in-flight loops of
    lsim_k_sinkhorn_scale and lsim_k_est_tail with and without passes; two cases with rows F.normalize clamps, compared row by row on their own scale"""
    case = R.estimator_case(name, iters)
    got = EstLaunch(name, iters).run()
    _compare("estimator %s iters %d" % (name, iters), case["out"], R.est_split(name, _est_outputs(got)))


# ---- Sinkhorn --------------------------------------------------------------------------------------------------------------------------------
class SkLaunch(Launch):
    def __init__(self, name, iters):
        super().__init__()
        B, K, layout = R.SK_CASES[name]
        off, lds = R.sk_layout(K, layout)
        scores = self.operand("scores", W.padded(R.sinkhorn_case(name, iters)["scores"], off, lds), off)
        assert (scores % 16 == 0) == (layout != "off4")
        n = ctypes.c_size_t(0)
        assert self.L.lsim_sinkhorn_workspace(B, K, ctypes.byref(n)) == 0
        ws = self.workspace(n.value, R.sinkhorn_plan(B, K)["bytes"])
        self.args = [scores, lds, B, K, R.SK_EPS, iters, self.output("q", (B, K)), ws, n.value]

    def call(self):
        return self.L.lsim_sinkhorn(*self.args, _stream())


@pytest.mark.parametrize("iters", R.ITERS)
@pytest.mark.parametrize("name", list(R.SK_CASES))
def test_sinkhorn_against_the_statement(name, iters):
    case = R.sinkhorn_case(name, iters)
    got = SkLaunch(name, iters).run()
    _compare("sinkhorn %s iters %d" % (name, iters), case["out"], got)
    rows = np.abs(got["q"].astype(np.float64).sum(1) - 1.0).max()
    print("sinkhorn", name, iters, "max |row sum - 1| %.3e" % rows)
    assert rows <= case["out"]["q"]["tol"], (name, rows, case["out"]["q"]["tol"])


# ---- the clipped-PPO loss --------------------------------------------------------------------------------------------------------------------
class PpoLaunch(Launch):
    def __init__(self, scene, entry, clip, clipped):
        super().__init__()
        B, A = scene["mu"].shape
        std_mode = entry == "std"
        ptr = {k: self.operand(k, _rows(v) if not (k == "sigma" and std_mode) else W.padded(v.reshape(1, A), 0, A)) for k, v in scene.items()}
        n = ctypes.c_size_t(0)
        rc = self.L.lsim_ppo_loss_std_workspace(B, A, ctypes.byref(n)) if std_mode else self.L.lsim_ppo_loss_workspace(B, ctypes.byref(n))
        assert rc == 0
        ws = self.workspace(n.value, R.ppo_plan(B, A, std_mode)["bytes"])
        self.fn = getattr(self.L, R.PPO_FN[entry])
        self.args = [ptr[k] for k in ("mu", "sigma", "value", "actions", "old_logp", "adv", "returns", "tv", "old_mu", "old_sigma")]
        self.args += [B, A, clip, R.PPO_CV, R.PPO_CE, clipped, self.output("stats", (5,)), self.output("g_mu", (B, A)),
                      self.output("g_std", (A,)) if std_mode else self.output("g_sigma", (B, A)), self.output("g_value", (B,)), ws, n.value]

    def call(self):
        return self.fn(*self.args, _stream())


@pytest.mark.parametrize("name", list(R.PPO_CASES))
def test_ppo_loss_against_the_statement(name):
    """block counts 1 .. 25 through both finish kernels, A = 1, 12, 60 (61 on the broadcast entry), clipped and plain value loss.  No row of a scene
    lies within the margins of a clip boundary, so EVERY row and g_std are compared"""
    c, case = R.PPO_CASES[name], R.ppo_case(name)
    assert case["near"] == [0, 0, 0]
    got = PpoLaunch(case["scene"], c["entry"], R.PPO_CLIP, c["clipped"]).run()
    _compare("ppo " + name, case["out"], R.ppo_outputs(got))


@pytest.mark.parametrize("entry", ["std", "sigma"])
def test_ppo_ties_and_closed_ends(entry):
    """the deterministic scene: adv = 0, ratio 1 inside the interval, v = tv, v = tv +- clip exactly (the clamp passes on the CLOSED interval) and
    l1 == l2 with the clamp saturated (the 1/2 - 1/2 split): the statement's conventions fix every gradient"""
    case = R.ppo_tie_case(entry == "std")
    s, rows = case["scene"], case["rows"]
    got = PpoLaunch(s, entry, case["clip"], 1).run()
    _compare("ppo ties " + entry, case["out"], R.ppo_outputs(got))
    B = s["mu"].shape[0]
    assert not got["g_mu"][rows["adv0"]].any(), "adv = 0: both branches are zero"
    v, tv, Rt = (s[k].astype(np.float64) for k in ("value", "tv", "returns"))
    tol = case["out"]["g_value"]["tol"]
    for k, factor in (("v_eq_tv", 2.0), ("end", 2.0), ("mid", 1.0)):
        want = R.PPO_CV * factor * (v - Rt)[rows[k]] / B
        assert np.abs(got["g_value"][rows[k]] - want).max() <= tol, (k, got["g_value"][rows[k]], want)


# ---- clip + Adam -----------------------------------------------------------------------------------------------------------------------------
GAP = 64


class Arena:
    """tensors of one kind in one NaN-filled buffer, GAP NaN floats in front of, between and behind them (so most start off any alignment)"""

    def __init__(self, arrays):
        self.sizes = [int(a.size) for a in arrays]
        self.offs, o = [], GAP
        for n in self.sizes:
            self.offs.append(o)
            o += n + GAP
        host = np.full(o, np.nan, dtype=np.float32)
        for a, off in zip(arrays, self.offs):
            host[off:off + a.size] = np.ravel(a)
        self.mask = np.isnan(host)
        self.dev = torch.from_numpy(host).to(DEV)

    def pointers(self):
        return (ctypes.c_void_p * len(self.offs))(*[self.dev.data_ptr() + 4 * off for off in self.offs])

    def read(self):
        """the tensors; asserts that exactly the gaps are still NaN"""
        host = self.dev.cpu().numpy()
        assert np.array_equal(np.isnan(host), self.mask), "a write outside a tensor, or a NaN inside one"
        assert np.isfinite(host[~self.mask]).all()
        return host, [host[off:off + n] for off, n in zip(self.offs, self.sizes)]


class AdamLaunch(Launch):
    def __init__(self, name, scene, plain_entry=False):
        super().__init__()
        c = self.c = R.ADAM_CASES[name]
        self.arenas = {k: Arena(scene[k]) for k in ("p", "g", "m", "v")}
        self.arenas["step"] = Arena([np.float32([s]) for s in c["steps"]])
        n = ctypes.c_size_t(0)
        assert self.L.lsim_adam_clip_step_workspace(c["count"], ctypes.byref(n)) == 0
        ws = self.workspace(n.value, R.adam_bytes(c["count"]))
        lr = self.operand("lr", W.padded(np.float32([[R.ADAM_LR]]), 0, 1)) if c["lr_dev"] else None
        tabs = [self.arenas[k].pointers() for k in ("p", "g", "m", "v", "step")]
        self.keep = tabs + [(ctypes.c_int64 * c["count"])(*c["sizes"]), (ctypes.c_float * c["count"])(*c["wd"])]
        tail = [lr, 0.0 if c["lr_dev"] else R.ADAM_LR, R.ADAM_B1, R.ADAM_B2, R.ADAM_EPS, c["max_norm"], self.output("norm", (1,)), ws, n.value]
        if plain_entry:
            assert c["clip_count"] == c["count"] and not any(c["wd"])
            self.fn, self.args = self.L.lsim_adam_clip_step, [c["count"], self.keep[5]] + tabs + tail
        else:
            self.fn, self.args = self.L.lsim_adam_clip_step_ex, [c["count"], self.keep[5]] + tabs + [self.keep[6], c["clip_count"]] + tail

    def call(self):
        return self.fn(*self.args, _stream())

    def step(self):
        """ONE call (the tensors are updated in place) -> (dict like adam_outputs, raw arena bits)"""
        assert self.call() == 0
        torch.cuda.synchronize()
        self.check_memory()
        raw, out = {}, {}
        for k, a in self.arenas.items():
            raw[k], tensors = a.read()
            out[k] = np.concatenate(tensors)
        out["norm"] = self.outs["norm"][0].cpu().numpy()[0]
        return out, raw


def _adam_twice(name, scene, **kw):
    out, raw = AdamLaunch(name, scene, **kw).step()
    _, again = AdamLaunch(name, scene, **kw).step()
    for k in raw:
        assert np.array_equal(raw[k].view(np.int32), again[k].view(np.int32)), "two steps from the same state differ in " + k
    return out


@pytest.mark.parametrize("name", list(R.ADAM_CASES))
def test_adam_clip_step_against_the_formula(name):
    """ONE step from a given state: 1, 7 and 48 tensors of 1 .. 20000 elements, the clipped group empty, partial and full, max_norm active, idle, 0 and
    negative, the learning rate on the device and on the host, step counters that differ per tensor, weight decay on some tensors"""
    case = R.adam_case(name)
    _compare("adam " + name, case["out"], _adam_twice(name, case["scene"]))


def test_adam_plain_entry_equals_the_statement():
    case = R.adam_case("n1-clip1-active-host")
    _compare("adam plain entry", case["out"], _adam_twice("n1-clip1-active-host", case["scene"], plain_entry=True))


@pytest.mark.parametrize("name", ["n1-clip1-active-host", "n7-clip3-active-dev", "n48-clip48-active-host"])
def test_adam_norm_and_coefficient_of_integer_gradients(name):
    """gradients in {-2 .. 2}: the squared sum is exact in fp32 in any order, so grad_norm_out is sqrtf of an exact number -- within 1 ulp of the
    correctly rounded root (HIP's documented sqrtf accuracy) -- and the clip coefficient, read back from an element whose gradient was 1, is within
    1 ulp of max_norm / (norm + 1e-6) formed in fp32 from that norm"""
    c, scene = R.ADAM_CASES[name], R.adam_scene(name, exact=True)
    total = sum(float((g.astype(np.float64) ** 2).sum()) for g in scene["g"][:c["clip_count"]])
    assert total == int(total) < 2 ** 24
    root = np.float32(np.sqrt(total))
    out, _ = AdamLaunch(name, scene).step()
    norm, coef = np.float32(out["norm"]), np.float32(out["g"][0])
    print(name, "sum of squares", total, "norm", norm, "correctly rounded", root, "coefficient", coef)
    assert abs(float(norm) - float(root)) <= float(np.spacing(root)), (norm, root)
    want = np.float32(c["max_norm"]) / (norm + np.float32(1e-6))
    assert want < 1 and abs(float(coef) - float(want)) <= float(np.spacing(want)), (coef, want)
    ref = 0.5 / (np.sqrt(total) + 1e-6)
    assert abs(float(coef) - ref) <= 3 * float(np.spacing(np.float32(ref)))          # 1 ulp of the root, the sum's and the quotient's rounding


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_entries_refuse_before_any_launch():
    """the refusals of tests/test_loss_heads.py on device buffers: the tabulated code, nothing written, no HIP error left behind -- a valid call of
    every entry succeeds afterwards.  Every refused call is answered by the entry's argument checks on the host"""
    from isaacgymloco_amd import abi
    L = _lib()
    for label, fam, edits, code in R.REFUSALS:
        d = _Device()
        rc = R.refusal_call(L, fam, edits, d.address)
        assert rc == getattr(abi, code), (label, rc)
        assert d.untouched(), label
    _compare("estimator after the refusals", R.estimator_case("b63-d5-k3", 3)["out"], R.est_split("b63-d5-k3", _est_outputs(EstLaunch("b63-d5-k3", 3).run())))
    _compare("sinkhorn after the refusals", R.sinkhorn_case("b5-k3-vec", 3)["out"], SkLaunch("b5-k3-vec", 3).run())
    for name in ("std-a1-b1-c0", "sigma-a12-b1-c1"):
        c = R.PPO_CASES[name]
        _compare("ppo after the refusals", R.ppo_case(name)["out"], R.ppo_outputs(PpoLaunch(R.ppo_case(name)["scene"], c["entry"], R.PPO_CLIP, c["clipped"]).run()))
    _compare("adam after the refusals", R.adam_case("n1-clip1-active-host")["out"], _adam_twice("n1-clip1-active-host", R.adam_case("n1-clip1-active-host")["scene"]))
