"""CPU: the depth-encoder source (isaacgymloco_amd/csrc/ls_depth_encoder.h) compiled by g++ under LS_EMU, against the numpy fp64 reference of
tests/depth_encoder_reference.py (written from include/lsim.h; its docstring derives the per-output error bound), the torch twin
(learn/depth_encoder.py) against the same reference, and envs/sensors.py attach_encoder on the emulated LeggedRobot.  The same shapes and
the same schedule run on the HIP launch in tests/test_gpu_depth_encoder.py."""
import ctypes

import numpy as np
import pytest
import torch

import depth_encoder_emu_binding as DB
import depth_encoder_reference as R
from helpers import abi


@pytest.mark.parametrize("name", sorted(DB.SHAPES))
def test_torch_twin_in_fp64_equals_the_reference(name):
    """pins the weight layouts and the flatten order of the header to torch's"""
    s = DB.SHAPES[name]
    mod = DB.module(s, 5)
    x = DB.frames_of(s, DB.images(s, 6))
    want, _ = R.encode(x, DB.params_of(mod), s["s1"], s["s2"], s.get("final_act", True))
    with torch.no_grad():
        got = mod.double()(torch.from_numpy(x).double()).numpy()
    assert got.shape == (s["N"], s["latent_dim"])
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("name", sorted(DB.SHAPES))
def test_shim_within_the_bound_of_the_reference(name):
    DB.check_shape(name, DB.Rig)


def test_the_bound_is_tight_enough_to_see_a_wrong_layout():
    """conditions on the test's own inputs (shape A), not measurements of the code under test"""
    s = DB.SHAPES["A"]
    params, hist = DB.params_of(DB.module(s, 0)), DB.images(s, 1)
    x = DB.frames_of(s, hist)
    want, bound = R.encode(x, params, s["s1"], s["s2"], True)
    rms = float(np.sqrt((want ** 2).mean()))
    print(f"shape A: bound max {bound.max():.3e} = {100 * bound.max() / rms:.4f} % of the latent's rms {rms:.3e}")
    assert bound.max() < 0.05 * rms
    wrong, _ = R.encode(x, params, s["s1"], s["s2"], True, transpose_w2=True)
    far = np.abs(wrong - want) > 10 * bound
    print(f"w2 with ky / kx transposed: {100 * far.mean():.1f} % of the outputs differ by more than 10 bounds")
    assert far.mean() > 0.5


def test_due_rule_and_untouched_rows():
    DB.schedule(DB.Rig)


def test_sizes():
    L = DB.lib()
    n = ctypes.c_size_t(7)
    rig = DB.Rig(DB.SHAPES["C"], DB.params_of(DB.module(DB.SHAPES["C"])), DB.images(DB.SHAPES["C"]))
    assert L.emu_depth_encode_sizes(ctypes.byref(rig.de), ctypes.byref(n)) == 0
    assert n.value == 4 * (max(2 * 48 * 64, 32 * 10 * 14) + 16 * 22 * 30 + 2 * 25 + 16 * 9)
    de = abi.LsimDepthEncoder.from_buffer_copy(rig.de)
    de.height, de.width = 200, 200
    n.value = 7
    assert L.emu_depth_encode_sizes(ctypes.byref(de), ctypes.byref(n)) == abi.E_INVALID and n.value == 7
    assert L.emu_depth_encode_sizes(None, ctypes.byref(n)) == abi.E_INVALID and L.emu_depth_encode_sizes(ctypes.byref(rig.de), None) == abi.E_INVALID


def test_every_invalid_argument_is_refused_and_nothing_is_written():
    s = DB.SHAPES["A"]
    params, hist = DB.params_of(DB.module(s)), DB.images(s)

    def rv(edit):
        rig = DB.Rig(s, params, hist)
        r = rig.launch(3, 0, edit)
        if r != 0:
            assert (rig.latent_bits() == DB.Rig.PREFILL).all()
        return r

    def f(name, value):
        return lambda de: setattr(de, name, value)

    def off(name, by):
        return lambda de: setattr(de, name, getattr(de, name) + by)

    assert rv(None) == 0
    assert DB.lib().emu_depth_encode(None, None) == abi.E_INVALID
    edits = {"flag 4": f("flags", 4), "both flags": f("flags", 3), "tick < 0": f("tick", -1), "period 0": f("period", 0), "period < 0": f("period", -2),
             "stagger 2": f("stagger", 2), "frames > slots": f("frames", 4), "frames 0": f("frames", 0), "slots 9": f("hist_slots", 9),
             "H * W > hist_stride": f("hist_stride", 220), "hist_stride odd": f("hist_stride", 222), "num_envs 0": f("num_envs", 0),
             "env_stride 0": f("env_stride", 0), "height 0": f("height", 0), "width 0": f("width", 0),
             "k1 > height": f("k1", 14), "k1 > 8": f("k1", 9), "k1 0": f("k1", 0), "s1 0": f("s1", 0), "s1 5": f("s1", 5), "c1 0": f("c1", 0), "c1 65": f("c1", 65),
             "k2 > h1": f("k2", 7), "k2 0": f("k2", 0), "s2 0": f("s2", 0), "s2 5": f("s2", 5), "c2 0": f("c2", 0), "c2 65": f("c2", 65),
             "latent_dim 0": f("latent_dim", 0), "latent_dim 257": f("latent_dim", 257), "final_act 2": f("final_act", 2),
             "latent_stride short": f("latent_stride", 32), "latent_stride odd": f("latent_stride", 38),
             "hist misaligned": off("hist", 8), "latent misaligned": off("latent", 4), "episode_length misaligned": off("episode_length", 4)}
    for p in ("hist", "episode_length", "latent", "w1", "b1", "w2", "b2", "w3", "b3"):
        edits[p + " NULL"] = f(p, None)
    for p in ("w1", "b1", "w2", "b2", "w3", "b3"):
        edits[p + " misaligned"] = off(p, 2)
    for what, edit in edits.items():
        assert rv(edit) == abi.E_INVALID, what
    # the limits themselves are accepted
    assert rv(f("flags", DB.FILL_ALL)) == 0 and rv(f("flags", DB.RESETS_ONLY)) == 0 and rv(f("hist_stride", 224)) == 0
    big = dict(DB.SHAPES["B"], latent_dim=256)
    rig = DB.Rig(big, DB.params_of(DB.module(big)), DB.images(big))
    assert rig.launch(0) == 0


def test_attach_encoder_on_the_emulated_env():
    import eval_emu_binding
    from helpers import C
    from isaacgymloco_amd.envs import sensors
    from isaacgymloco_amd.learn.depth_encoder import DepthEncoder
    cfg = C.mixed_cfg("aliengo", {"aliengo": 0.5, "go2": 0.5})[0]
    cfg.env.num_envs = 4
    cfg.terrain.num_rows, cfg.terrain.num_cols = 2, 2
    cfg.terrain.terrain_proportions = [0.0, 0.0, 0.0, 0.0, 0.5, 0.5]
    env = eval_emu_binding.emu_mixed_env(cfg)
    env.reset()
    api = DB.EmuApi()
    kw = dict(mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, api=api, see_robot=True)
    torch.manual_seed(2)
    enc = DepthEncoder(4, 6, 2, c1=3, k1=2, s1=1, c2=5, k2=2, s2=1, latent_dim=6)

    # a sensor without a model: no encoder, and nothing more is launched than before
    plain = env.add_sensor("plain", sensors.depth_camera(env, 6, 4, 87.0, **kw))
    with pytest.raises(ValueError):
        plain.attach_encoder(enc)
    with pytest.raises(ValueError):
        plain.latent()
    bare = env.add_sensor("bare", sensors.depth_camera(env, 6, 4, 87.0, model=sensors.SensorModel(period=2, frames=2), **kw))
    env.step_device(torch.zeros(4, 12))
    assert api.calls == {"lsim_raycast": 0, "lsim_raycast_bodies": 1, "lsim_sensor_capture": 2, "lsim_depth_encode": 0}
    assert plain.stage("encoder") is None and bare.stage("encoder") is None and bare.encoder is None
    with pytest.raises(ValueError):
        bare.latent()

    m = sensors.SensorModel(period=2, stagger=True, latency=1, frames=2, clip=(0.1, 3.0), normalise=True)
    cam = sensors.depth_camera(env, 6, 4, 87.0, model=m, **kw)
    assert cam.attach_encoder(enc) is enc and api.calls["lsim_depth_encode"] == 0      # no capture yet: nothing to encode
    env.add_sensor("depth", cam)                                                        # one refresh: FILL_ALL, every env encoded
    assert api.calls["lsim_depth_encode"] == 1 and cam.latent().shape == (4, 6)
    params = DB.params_of(enc)

    def reference():
        x = cam.frame_images().numpy().astype(np.float64)
        return R.encode(x, params, 1, 1, True)

    want, bound = reference()
    assert (np.abs(cam.latent().numpy() - want) <= bound).all() and np.abs(want).max() > 1e-3
    g = torch.Generator().manual_seed(4)
    for _ in range(3):
        before, t = cam.latent().numpy().copy(), env.common_step_counter
        calls = api.calls["lsim_depth_encode"]
        env.step_device(torch.randn(4, 12, generator=g) * 0.3)
        assert api.calls["lsim_depth_encode"] == calls + 1 and cam.tick == t
        due, _ = R.due_sets(4, 1, t, 2, True, 0, env.episode_length_buf.numpy())
        want, bound = reference()
        after = cam.latent().numpy()
        assert due.any() and not due.all()
        assert (np.abs(after[due] - want[due]) <= bound[due]).all()
        np.testing.assert_array_equal(after[~due].view(np.uint32), before[~due].view(np.uint32))
    # a reset by hand: RESETS_ONLY reaches the encoder with the sensor's flags
    before = cam.latent().numpy().copy()
    env.reset_idx([2])
    after = cam.latent().numpy()
    want, bound = reference()
    np.testing.assert_array_equal(after[[0, 1, 3]], before[[0, 1, 3]])
    assert (np.abs(after[2] - want[2]) <= bound[2]).all() and not (after[2] == before[2]).all()
    # the parameters must be where and what the launch reads
    with pytest.raises(ValueError, match="fp32"):
        DepthEncoder(4, 6, 2, c1=3, k1=2, s1=1, c2=5, k2=2, s2=1, latent_dim=6).double().encode_device(cam, 0)
    strided = DepthEncoder(4, 6, 2, c1=3, k1=2, s1=1, c2=5, k2=2, s2=1, latent_dim=6)
    strided.fc.weight = torch.nn.Parameter(torch.zeros(strided.fc.weight.shape[1], 6).t())
    with pytest.raises(ValueError, match="contiguous"):
        strided.encode_device(cam, 0)
    with pytest.raises(ValueError, match="on cpu"):
        DepthEncoder(4, 6, 2, c1=3, k1=2, s1=1, c2=5, k2=2, s2=1, latent_dim=6).to("meta").encode_device(cam, 0)
    with pytest.raises(ValueError, match="frames"):
        DepthEncoder(4, 6, 1, c1=3, k1=2, s1=1, c2=5, k2=2, s2=1, latent_dim=6).encode_device(cam, 0)
