"""TEST INFRASTRUCTURE -- builds and binds tests/emu/emu_depth_encoder.cpp (the CPU shim of the depth-encoder launch,
isaacgymloco_amd/csrc/ls_depth_encoder.h compiled by g++ under LS_EMU), the shapes both depth-encoder test files run, and Rig: one
lsim_depth_encoder with the arrays it points to, in host memory for the shim or in device memory for the HIP library."""
import numpy as np

import emu_binding
from helpers import abi
from launch_rig import LaunchRig

FILL_ALL, RESETS_ONLY = abi.DEFINES["LSIM_SENSOR_FILL_ALL"], abi.DEFINES["LSIM_SENSOR_RESETS_ONLY"]

# name -> extents.  A: nothing a multiple of a tile, hist_stride > R, fewer frames than slots, strided envs; B: one frame, one channel tile,
# a kernel larger than the stride; C: the default network on the 64 x 48 camera (LDS above 64 KB); D: a flattened length that is no multiple
# of 4 (the linear layer's single-float path), 3 channel tiles in conv 2, no final activation
SHAPES = {
    "A": dict(height=13, width=17, hist_stride=224, frames=2, slots=3, c1=5, k1=3, s1=2, c2=19, k2=3, s2=1, latent_dim=33, N=7, env_stride=2),
    "B": dict(height=12, width=16, frames=1, slots=1, c1=4, k1=5, s1=1, c2=8, k2=2, s2=2, latent_dim=8, N=2),
    "C": dict(height=48, width=64, frames=2, slots=2, c1=16, k1=5, s1=2, c2=32, k2=3, s2=2, latent_dim=64, N=3),
    "D": dict(height=9, width=11, frames=3, slots=4, c1=7, k1=2, s1=1, c2=35, k2=4, s2=3, latent_dim=5, N=2, final_act=False),
}


def lib():
    return emu_binding.shim("depth_encoder")


def EmuApi():
    """the range-sensor entry points of the three sensor shims and lsim_depth_encode of this one, for envs.sensors.RaySensor(api=...); counts the launches"""
    return emu_binding.api("raycast", "raycast_bodies", "sensor_model", "depth_encoder",
                           count=("lsim_raycast", "lsim_raycast_bodies", "lsim_sensor_capture", "lsim_depth_encode"))


def module(shape, seed=0):
    """the torch twin of `shape` with torch's default initialisation under `seed`"""
    import torch
    from isaacgymloco_amd.learn.depth_encoder import DepthEncoder
    torch.manual_seed(seed)
    s = shape
    return DepthEncoder(s["height"], s["width"], s["frames"], s["c1"], s["k1"], s["s1"], s["c2"], s["k2"], s["s2"], s["latent_dim"], s.get("final_act", True))


def params_of(mod):
    return tuple(p.detach().cpu().numpy().copy() for p in mod.device_params())


def images(shape, seed=1, scale=1.0):
    """[N, slots, hist_stride] fp32 uniform in [0, scale): the whole of hist, padding and the slots past `frames` included"""
    s = shape
    stride = s.get("hist_stride") or (s["height"] * s["width"] + 3) // 4 * 4
    return (np.random.default_rng(seed).random((s["N"], s["slots"], stride)) * scale).astype(np.float32)


def frames_of(shape, hist):
    """[N, frames, H, W]: what the encoder reads of hist"""
    s = shape
    return hist[:, :s["frames"], :s["height"] * s["width"]].reshape(s["N"], s["frames"], s["height"], s["width"])


class Rig(LaunchRig):
    """`shape`: an entry of SHAPES; `params`: (w1, b1, w2, b2, w3, b3) numpy; `hist`: images(shape).  `device`: None -- numpy arrays and the
    shim -- or a torch device and `entry` = the library's lsim_depth_encode.  `latent` starts as NaN with the bit pattern PREFILL, with a guard behind it;
    episode_length as 1.  period / stagger: keywords."""
    PREFILL = 0x7FC00ABC

    def __init__(self, shape, params, hist, device=None, entry=None, period=1, stagger=0):
        s = self.shape = shape
        super().__init__(device)
        self.N, self.L = s["N"], s["latent_dim"]
        self.lstride = (self.L + 3) // 4 * 4 + 4
        for k, v in zip(("w1", "b1", "w2", "b2", "w3", "b3"), params):
            self.add(k, np.asarray(v, np.float32))
        self.add("hist", np.asarray(hist, np.float32))
        self.add("episode_length", np.ones(self.N, np.int64))
        self.add("latent", np.full((self.N, self.lstride), self.PREFILL, np.uint32).view(np.float32), guard=True)
        de = abi.LsimDepthEncoder()
        self.point(de, ("hist", "episode_length", "latent", "w1", "b1", "w2", "b2", "w3", "b3"))
        de.hist_stride, de.hist_slots, de.num_envs, de.env_stride = hist.shape[2], hist.shape[1], self.N, s.get("env_stride", 1)
        for k in ("height", "width", "frames", "c1", "k1", "s1", "c2", "k2", "s2", "latent_dim"):
            setattr(de, k, s[k])
        de.final_act, de.latent_stride, de.period, de.stagger = int(s.get("final_act", True)), self.lstride, int(period), int(stagger)
        self.de = self.bind(de, entry if device is not None else lib().emu_depth_encode)

    def latent_bits(self):
        """[N, lstride] uint32: the whole buffer, padding included; asserts the guard behind it intact"""
        self.assert_guards()
        return self.get("latent").view(np.uint32)

    def latent(self):
        self.assert_guards()
        return self.get("latent")[:, :self.L]


def check_shape(name, make_rig, seed=0):
    """shape `name` through `make_rig(shape, params, hist)` against the reference within its bound; returns the worst |difference| / bound"""
    import depth_encoder_reference as R
    s = SHAPES[name]
    params, hist = params_of(module(s, seed)), images(s, seed + 1)
    rig = make_rig(s, params, hist)
    assert rig.launch(0, FILL_ALL) == 0
    want, bound = R.encode(frames_of(s, hist), params, s["s1"], s["s2"], s.get("final_act", True))
    got, bits = rig.latent(), rig.latent_bits()
    visited = np.arange(s["N"]) % s.get("env_stride", 1) == 0
    assert (bits[~visited] == Rig.PREFILL).all() and (bits[:, s["latent_dim"]:] == Rig.PREFILL).all(), "rows of envs not visited and the padding stay"
    assert np.isfinite(got[visited]).all()
    ratio = float((np.abs(got[visited] - want[visited]) / bound[visited]).max())
    print(f"shape {name}: worst |difference| / bound = {ratio:.2e}  (bound max {bound.max():.3e}, latent rms {np.sqrt((want ** 2).mean()):.3e})")
    assert ratio <= 1.0
    return ratio


def schedule(make_rig):
    """a staggered period-3 schedule on shape A with env_stride 1 and N = 7: plain ticks, a reset env, RESETS_ONLY, FILL_ALL, every launch on a
    fresh NaN pre-fill and fresh images.  Returns [(due set, latent)] per launch; rows not due keep the pre-fill bit for bit, due rows
    are within the bound of the reference."""
    import depth_encoder_reference as R
    s = dict(SHAPES["A"], env_stride=1)
    params = params_of(module(s, 3))
    rig = make_rig(s, params, images(s, 0), period=3, stagger=1)
    out = []
    steps = [(0, 0, None), (1, 0, None), (2, 0, 0), (5, RESETS_ONLY, 1), (7, RESETS_ONLY, None), (8, FILL_ALL, None), (9, 0, None)]
    for k, (tick, flags, reset) in enumerate(steps):
        hist = images(s, 10 + k)
        el = np.ones(s["N"], np.int64)
        if reset is not None:
            el[reset] = 0
        rig.put("hist", hist)
        rig.put("episode_length", el)
        rig.put("latent", np.array([Rig.PREFILL], np.uint32).view(np.float32)[0])
        assert (rig.latent_bits() == Rig.PREFILL).all()
        assert rig.launch(tick, flags) == 0
        due, _ = R.due_sets(s["N"], 1, tick, 3, True, flags, el)
        bits, got = rig.latent_bits(), rig.latent()
        assert (bits[~due] == Rig.PREFILL).all(), f"tick {tick}: a row that is not due was written"
        assert not np.isnan(got[due]).any(), f"tick {tick}: a due row was not written"
        want, bound = R.encode(frames_of(s, hist), params, s["s1"], s["s2"], True)
        assert (np.abs(got[due] - want[due]) <= bound[due]).all()
        out.append((due, got))
    assert [int(d.sum()) for d, _ in out] == [3, 2, 3, 1, 0, 7, 3]
    return out
