"""TEST INFRASTRUCTURE -- builds and binds tests/emu/emu_depth_memory.cpp (the CPU shim of the depth-memory launches,
isaacgymloco_amd/csrc/ls_depth_memory.h compiled by g++ under LS_EMU), the shapes both depth-memory test files run, and the two rigs: the
arrays of one lsim_depth_memory_t / lsim_gru_sequence_t with guard words behind each (inputs included), in host memory for the shim or in device memory for
the HIP library, and the checks that run on either."""
import numpy as np

import emu_binding
import depth_memory_reference as R
from helpers import abi
from launch_rig import LaunchRig

FILL_ALL, RESETS_ONLY = abi.DEFINES["LSIM_SENSOR_FILL_ALL"], abi.DEFINES["LSIM_SENSOR_RESETS_ONLY"]
LsimDepthMemory, LsimGruSequence = abi.STRUCTS["lsim_depth_memory_t"], abi.STRUCTS["lsim_gru_sequence_t"]

# A: less than one tile; B: I = 17 (no multiple of 4), every stride larger than its width, a ragged last tile; C: the default cell, crossing
# tile 16; D: p == NULL, three hidden tiles; E: T = 1, the largest hidden size that must be accepted (two hidden tiles on waves 0 and 1)
SHAPES = {
    "A": dict(N=7, L=5, P=3, H=16, T=4),
    "B": dict(N=37, L=10, P=7, H=32, T=6, pad=(3, 2, 4, 5)),
    "C": dict(N=257, L=64, P=45, H=64, T=5),
    "D": dict(N=16, L=12, P=0, H=48, T=3),
    "E": dict(N=33, L=8, P=4, H=96, T=1),
}
PREFILL = 0x7FC00ABC          # a NaN: an output not written


def lib():
    return emu_binding.shim("depth_memory")


def EmuApi(*more, count=()):
    """the sensor and encoder shims plus this one (and the libraries `more`), for envs.sensors.RaySensor(api=...); counts the launches named in `count`"""
    return emu_binding.api("raycast", "raycast_bodies", "sensor_model", "depth_encoder", "depth_memory", *more, count=count)


def params(shape, seed=0):
    """(weight_ih, weight_hh, bias_ih, bias_hh) fp32 with nn.GRUCell's initialisation: uniform in +- 1 / sqrt(H)"""
    H, I = shape["H"], shape["L"] + shape["P"]
    g = np.random.default_rng(seed)
    k = 1.0 / np.sqrt(H)
    return tuple(g.uniform(-k, k, s).astype(np.float32) for s in ((3 * H, I), (3 * H, H), (3 * H,), (3 * H,)))


def resets(shape, seed=0):
    """[T, N] uint8: env 0 fresh at t = 0, env 1 reset mid-sequence, env 2 at two consecutive steps, env 3 never, the others at random"""
    T, N = shape["T"], shape["N"]
    r = (np.random.default_rng(seed).random((T, N)) < 0.2).astype(np.uint8)
    r[:, :4] = 0
    r[0, 0] = 1
    r[T // 2, 1] = 1
    r[max(T - 3, 0):max(T - 1, 1), 2] = 1
    return r


def nan_fill(shape):
    return np.full(shape, PREFILL, np.uint32).view(np.float32)


class StepRig(LaunchRig):
    """one lsim_depth_memory_t: z, p, h, rows with the row pitches of `shape` (width + pad), episode_length, the four parameters"""

    def __init__(self, shape, prm, z, p, h, episode_length, device=None, entry=None):
        super().__init__(device)
        s = self.shape = shape
        N, L, P, H = s["N"], s["L"], s["P"], s["H"]
        pz, pp, ph, pr = s.get("pad", (0, 0, 0, 0))
        self.ld = dict(z=L + pz, p=P + pp, h=H + ph, rows=L + H + pr)

        def padded(v, ld):
            out = nan_fill((N, ld))
            out[:, :v.shape[1]] = v
            return out
        self.add("z", padded(z, self.ld["z"]), guard=True)
        if P:
            self.add("p", padded(p, self.ld["p"]), guard=True)
        self.add("h", padded(h, self.ld["h"]), guard=True)
        self.add("rows", nan_fill((N, self.ld["rows"])), guard=True)
        self.add("episode_length", np.asarray(episode_length, np.int64), guard=True)
        for k, v in zip(("weight_ih", "weight_hh", "bias_ih", "bias_hh"), prm):
            self.add(k, v, guard=True)
        dm = LsimDepthMemory()
        self.point(dm, list(self.a))
        dm.num_envs, dm.latent_dim, dm.proprio_dim, dm.hidden = N, L, P, H
        dm.z_ld, dm.p_ld, dm.h_ld, dm.rows_ld = self.ld["z"], self.ld["p"], self.ld["h"], self.ld["rows"]
        self.dm = self.bind(dm, entry if device is not None else lib().emu_depth_memory_step)

    def launch(self, flags=0, edit=None, stream=None):
        return super().launch(None, flags, edit, stream)

    def h(self):
        return self.get("h")[:, :self.shape["H"]]

    def outputs_bits(self):
        return np.concatenate((self.get("h").view(np.uint32).reshape(-1), self.get("rows").view(np.uint32).reshape(-1)))


def step_case(shape, seed=0):
    """(params, z, p, h, episode_length): envs 0 and N - 1 (and every 5th) fresh"""
    g = np.random.default_rng(100 + seed)
    N, L, P, H = shape["N"], shape["L"], shape["P"], shape["H"]
    el = np.arange(N, dtype=np.int64) % 5
    el[N - 1] = 0
    return (params(shape, seed), g.standard_normal((N, L)).astype(np.float32), g.standard_normal((N, P)).astype(np.float32),
            (0.6 * g.uniform(-1, 1, (N, H))).astype(np.float32), el)


def check_step(name, make_rig, seed=0, weight_edit=None):
    """shape `name` through `make_rig(shape, params, z, p, h, episode_length)`: flags 0, FILL_ALL, RESETS_ONLY, rows == NULL, a repeat; every output
    within the reference's bound, everything else bit for bit as it was.  `weight_edit(rig)`: an in-place change of the parameters between two
    launches, returns the new parameters.  Returns the worst |difference| / bound."""
    s = SHAPES[name]
    prm, z, p, h, el = step_case(s, seed)
    L, H = s["L"], s["H"]
    fresh = el == 0
    pp = p if s["P"] else None
    worst = 0.0

    def verify(rig, prm, flags):
        nonlocal worst
        fr = np.ones_like(fresh) if flags & FILL_ALL else fresh
        stepped = fr if flags & RESETS_ONLY else np.ones_like(fresh)
        want, bound = R.step(z, pp, h, fr, prm)
        got_h, got_rows = rig.get("h"), rig.get("rows")
        assert rig.guards_intact(), "a word behind a buffer was written"
        assert (got_h.view(np.uint32)[:, H:] == PREFILL).all() and (got_rows.view(np.uint32)[:, L + H:] == PREFILL).all(), "padding columns were written"
        assert (got_rows.view(np.uint32)[~stepped] == PREFILL).all(), "the row of an env that does not step was written"
        np.testing.assert_array_equal(got_h[~stepped, :H].view(np.uint32), h[~stepped].view(np.uint32))
        assert np.isfinite(got_h[stepped, :H]).all()
        ratio = float((np.abs(got_h[stepped, :H] - want[stepped]) / bound[stepped]).max()) if stepped.any() else 0.0
        np.testing.assert_array_equal(got_rows[stepped, :L].view(np.uint32), z[stepped].view(np.uint32))
        np.testing.assert_array_equal(got_rows[stepped, L:L + H].view(np.uint32), got_h[stepped, :H].view(np.uint32))
        for k, v in (("z", z), ("p", p)) if s["P"] else (("z", z),):
            np.testing.assert_array_equal(rig.get(k)[:, :v.shape[1]], v)
        worst = max(worst, ratio)
        print(f"step {name} flags {flags}: worst |difference| / bound = {ratio:.2e} (bound max {bound.max():.3e})")
        assert ratio <= 1.0

    for flags in (0, FILL_ALL, RESETS_ONLY):
        rig = make_rig(s, prm, z, p, h, el)
        assert rig.launch(flags) == 0
        verify(rig, prm, flags)
        first = rig.outputs_bits()
        rig.put("h", _repad(h, rig.ld["h"]))
        rig.put("rows", nan_fill((s["N"], rig.ld["rows"])))
        assert rig.launch(flags) == 0
        np.testing.assert_array_equal(rig.outputs_bits(), first, "two identical calls wrote different bits")
    # rows == NULL: h is stepped, no row is written
    rig = make_rig(s, prm, z, p, h, el)
    assert rig.launch(0, lambda dm: setattr(dm, "rows", None)) == 0
    assert (rig.get("rows").view(np.uint32) == PREFILL).all() and rig.guards_intact()
    want, bound = R.step(z, pp, h, fresh, prm)
    assert (np.abs(rig.h() - want) <= bound).all()
    if weight_edit is not None:         # the launch reads the parameters where they are: no packing step
        rig.put("h", _repad(h, rig.ld["h"]))
        prm2 = weight_edit(rig)
        assert rig.launch(0) == 0
        verify(rig, prm2, 0)
        assert (np.abs(rig.h() - want) > bound).any(), "the changed parameters were not read"
    return worst


def _repad(v, ld):
    out = nan_fill((v.shape[0], ld))
    out[:, :v.shape[1]] = v
    return out


def scale_weights(rig):
    """multiply weight_hh and bias_ih in place by -1.5 / +2; returns the parameters the next launch must see"""
    prm = [rig.get(k) for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    prm[1], prm[2] = (prm[1] * np.float32(-1.5)).astype(np.float32), (prm[2] * np.float32(2.0)).astype(np.float32)
    for k, f in (("weight_hh", -1.5), ("bias_ih", 2.0)):
        rig.a[k][:int(np.prod(rig.n[k][0]))] *= f        # in place, on the host or on the device
    return tuple(prm)


class SeqRig(LaunchRig):
    """one lsim_gru_sequence_t with contiguous [T, n, .] arrays; outputs start as NaN with the bit pattern PREFILL"""

    def __init__(self, shape, prm, gi, h0, reset, dhs, device=None, entries=None):
        super().__init__(device)
        s = self.shape = shape
        T, n, H = s["T"], s["N"], s["H"]
        for k, v in (("gi", gi), ("h0", h0), ("reset", np.asarray(reset, np.uint8)), ("weight_hh", prm[1]), ("bias_hh", prm[3]), ("dhs", dhs)):
            self.add(k, v, guard=True)
        for k, w in (("hs", H), ("save", 4 * H), ("dgi", 3 * H), ("dghn", H)):
            self.add(k, nan_fill((T, n, w)), guard=True)
        self.add("dh0", nan_fill((n, H)), guard=True)
        gs = LsimGruSequence()
        self.point(gs, list(self.a))
        gs.steps, gs.num_envs, gs.hidden = T, n, H
        L = lib() if device is None else None
        self._fwd, self._bwd = entries if device is not None else (L.emu_gru_sequence_forward, L.emu_gru_sequence_backward)
        self.gs = self.bind(gs, self._fwd)

    def forward(self, edit=None, stream=None):
        return self.launch(edit=edit, stream=stream)

    def backward(self, edit=None, stream=None):
        return self.launch(edit=edit, stream=stream, entry=self._bwd)

    OUT = ("hs", "save", "dgi", "dghn", "dh0")

    def output_bits(self):
        return np.concatenate([self.get(k).view(np.uint32).reshape(-1) for k in self.OUT])

    def clear(self):
        for k in self.OUT:
            self.put(k, nan_fill(self.n[k][0]))


_seq_cases = {}


def sequence_case(name, seed=0):
    """the inputs of shape `name` and their fp64 reference, computed once and shared (never modified): dict prm, x, gi, h0, reset, dhs, fwd, bwd, tol, dist"""
    if (name, seed) not in _seq_cases:
        s = SHAPES[name]
        g = np.random.default_rng(200 + seed)
        T, n, H, I = s["T"], s["N"], s["H"], s["L"] + s["P"]
        prm = params(s, seed)
        x = g.standard_normal((T, n, I)).astype(np.float32)
        gi = R.project(x, prm)[0].astype(np.float32)                  # the kernel's input: taken as exact from here on
        h0 = (0.6 * g.uniform(-1, 1, (n, H))).astype(np.float32)
        reset = resets(s, seed)
        dhs = g.standard_normal((T, n, H)).astype(np.float32)
        fwd = R.sequence(gi, h0, reset, prm)
        bwd = R.backward(dhs, fwd, h0, reset, prm)
        tol, dist = R.backward_tolerance(gi, h0, reset, prm, dhs, bwd)
        c = dict(prm=prm, x=x, gi=gi, h0=h0, reset=reset, dhs=dhs, fwd=fwd, bwd=bwd, tol=tol, dist=dist)
        for v in list(c.values()) + list(fwd.values()) + list(bwd.values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _seq_cases[name, seed] = c
    return _seq_cases[name, seed]


def check_sequence(name, make_rig, seed=0):
    """shape `name` through `make_rig(shape, params, gi, h0, reset, dhs)`: forward within the propagated bound, backward within 4 x the distance of
    the torch fp32 evaluation, guards intact, dh0 == NULL and save == NULL accepted, a repeat bit for bit.  Returns the worst ratios."""
    s, c = SHAPES[name], sequence_case(name, seed)
    rig = make_rig(s, c["prm"], c["gi"], c["h0"], c["reset"], c["dhs"])
    assert rig.forward() == 0 and rig.backward() == 0
    assert rig.guards_intact(), "a word behind a buffer was written"
    out = {k: rig.get(k) for k in rig.OUT}
    ratios = {}
    for k, e in (("hs", "e_hs"), ("save", "e_save")):
        assert np.isfinite(out[k]).all(), k
        ratios[k] = float((np.abs(out[k] - c["fwd"][k]) / c["fwd"][e]).max())
    for k in ("dgi", "dghn", "dh0"):
        assert np.isfinite(out[k]).all(), k
        ratios[k] = float(np.abs(out[k] - c["bwd"][k]).max() / c["tol"][k])
    print(f"sequence {name}: |difference| / allowance " + ", ".join(f"{k} {v:.2e}" for k, v in ratios.items()) +
          "; torch fp32 distance " + ", ".join(f"{k} {v:.2e}" for k, v in c["dist"].items()))
    assert max(ratios.values()) <= 1.0, ratios
    for k in ("gi", "h0", "reset", "dhs"):
        np.testing.assert_array_equal(rig.get(k), c[k])
    first = rig.output_bits()
    rig.clear()
    assert rig.forward() == 0 and rig.backward() == 0
    np.testing.assert_array_equal(rig.output_bits(), first, "two identical calls wrote different bits")
    # the optional outputs left out: nothing is written there, the rest is the same
    rig.clear()
    assert rig.forward(lambda gs: setattr(gs, "save", None)) == 0
    assert (rig.get("save").view(np.uint32) == PREFILL).all()
    np.testing.assert_array_equal(rig.get("hs").view(np.uint32), out["hs"].view(np.uint32))
    rig.put("save", out["save"])
    assert rig.backward(lambda gs: setattr(gs, "dh0", None)) == 0
    assert (rig.get("dh0").view(np.uint32) == PREFILL).all() and rig.guards_intact()
    np.testing.assert_array_equal(rig.get("dgi").view(np.uint32), out["dgi"].view(np.uint32))
    return ratios
