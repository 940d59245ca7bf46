"""CPU: the shaded frames through the Python surface (envs/sensors.py Shading, depth_camera(shading=...), set_shading(), chase_camera(),
spec() / from_spec(), write_ppm; learn/evaluate.py frames=...) on the emulated LeggedRobot, every launch through the CPU builds of the
kernel sources.  The launch itself is held to its reference in tests/test_sensor_shade.py."""
import json
import math
import os

import numpy as np
import pytest
import torch

import emu_binding
import eval_columns_emu_binding as CB
import sensor_shade_scenes as SS
from helpers import C, abi
from isaacgymloco_amd.envs import sensors

N, W, H = 8, 16, 12
ORDER = ("rays", "odometry", "mount_jitter", "instrument", "capture", "map", "map_rows", "encoder", "memory")


def _api():
    SS.shim()
    return emu_binding.api("raycast", "raycast_bodies", "sensor_model", SS.shim(), count=("lsim_raycast_bodies", "lsim_sensor_shade", "lsim_sensor_capture"))


def _env(seed=3):
    from emu_env import EmuLeggedRobot
    from isaacgymloco_amd.learn.evaluate import play_cfg
    cfg = play_cfg(C.aliengo_cfg())
    cfg.env.num_envs = N
    cfg.terrain.num_rows, cfg.terrain.num_cols = 2, 2
    cfg.terrain.terrain_proportions = [0.0, 0.0, 0.0, 0.0, 0.5, 0.5]
    env = EmuLeggedRobot(cfg, seed=seed)
    env.reset()
    return env


def _camera(env, api, **kw):
    kw.setdefault("see_robot", True)
    kw.setdefault("labels", True)
    return sensors.depth_camera(env, W, H, 60.0, mount_pos=(-1.2, 0.0, 0.7), pitch_deg=28.0, near=0.05, far=6.0, api=api, frame="yaw", **kw)


def test_shading_values_and_text():
    d = sensors.Shading()
    assert sensors.Shading.FIELDS == tuple(sensors.Shading.TEXT) == ("sun", "ambient", "shadows", "checker", "checker_gain", "palette", "shadow_bias", "shadow_far")
    assert d.record() == {"sun": [145.0, 50.0], "ambient": 0.35, "shadows": True, "checker": 0.5, "checker_gain": 0.8, "palette": None, "shadow_bias": 0.002,
                          "shadow_far": 4.0}
    s = sensors.Shading(sun=(200.0, 20.0), ambient=0.2, shadows=False, checker=0.0, palette=tuple(range(19)))
    assert sensors.Shading(**s.record()) == s and s != d and json.loads(json.dumps(s.record())) == s.record() and eval("sensors." + repr(s)) == s
    assert sensors.parse_shading("") == d and sensors.parse_shading("default") == d and sensors.parse_option(sensors.Shading, "palette=none") == d
    assert sensors.parse_shading("sun=200:20,ambient=0.2,shadows=0,checker=0,palette=" + ":".join(f"{w:x}" for w in range(19))) == s
    v = d.sun_vector()
    assert abs(sum(x * x for x in v) - 1.0) < 1e-12 and v[2] == pytest.approx(math.sin(math.radians(50.0))) and v[0] < 0 < v[1]
    words = d.palette_words()
    assert len(words) == 19 and len(set(words)) == 19, "sky, terrain, trunk and every leg body are told apart"
    kinds = [[words[2 + 1 + 4 * leg + k] for leg in range(4)] for k in range(4)]          # hips, thighs, calves, feet
    dominant = lambda w: int(np.argmax([w & 255, (w >> 8) & 255, (w >> 16) & 255]))
    assert [len({dominant(w) for w in ws}) for ws in kinds] == [1, 1, 1, 1] and len({tuple(sorted(set(map(dominant, ws)))) for ws in kinds[1:]}) == 3
    for bad in (dict(sun=(0.0, 0.0)), dict(sun=(0.0, 91.0)), dict(sun=(math.nan, 30.0)), dict(sun=(1.0, 2.0, 3.0)), dict(ambient=-0.1), dict(ambient=1.1),
                dict(checker=-1.0), dict(checker_gain=math.inf), dict(shadow_bias=-1e-3), dict(shadow_far=math.nan), dict(palette=(1, 2, 3)),
                dict(palette=(1 << 24,) * 19)):
        with pytest.raises(ValueError):
            sensors.Shading(**bad)
    for bad in ("sun", "sun=1", "gain=3", "ambient=0.1,ambient=0.2"):
        with pytest.raises(ValueError):
            sensors.parse_shading(bad)


def test_the_order_tuple_is_the_pinned_one_and_shade_sits_behind_the_rays():
    assert sensors._ORDER == ORDER and sensors._BEHIND["shade"] == "rays"
    assert sensors._LAUNCH_ORDER[:2] == ("rays", "shade")


def test_without_the_option_nothing_is_allocated_or_launched():
    env, api = _env(), _api()
    cam = env.add_sensor("chase", _camera(env, api))
    for _ in range(2):
        env.step_device(torch.zeros(N, 12))
    assert api.calls["lsim_sensor_shade"] == 0 and api.calls["lsim_raycast_bodies"] == 2
    assert cam.shading is None and cam.stage("shade") is None and cam.chain() == ("lsim_raycast_bodies",)
    for view in (cam.rgba_image, cam.rgb_image, cam.surface):
        with pytest.raises(ValueError, match="shading"):
            view()
    assert list(cam.spec()) == ["kind", "width", "height", "dirs", "scale", "near", "far", "env_stride", "see_robot", "labels", "frame", "ignore_bodies",
                                "model", "mount"]


def test_the_three_refusals():
    env, api = _env(), _api()
    s = sensors.Shading()
    with pytest.raises(ValueError, match="labels=True"):
        _camera(env, api, labels=False, shading=s)
    with pytest.raises(ValueError, match="labels=True"):
        sensors.depth_camera(env, W, H, 60.0, api=api, shading=s)
    with pytest.raises(ValueError, match="stale range"):
        _camera(env, api, model=sensors.SensorModel(period=2), shading=s)
    with pytest.raises(ValueError, match="no lsim_sensor_shade"):
        _camera(env, emu_binding.api("raycast", "raycast_bodies"), shading=s)           # a library from before the entry point: no torch fall-back
    with pytest.raises(TypeError):
        _camera(env, api, shading={"sun": (1, 2)})
    assert api.calls["lsim_sensor_shade"] == 0


def test_launch_order_struct_and_views():
    env, api = _env(), _api()
    order = []
    for name in ("lsim_raycast_bodies", "lsim_sensor_shade"):
        fn = getattr(api, name)
        setattr(api, name, lambda *a, _fn=fn, _n=name: (order.append(_n), _fn(*a))[1])
    opt = sensors.Shading(sun=(185.0, 22.0))
    cam = env.add_sensor("chase", _camera(env, api, env_stride=2, shading=opt))
    assert cam.chain() == ("lsim_raycast_bodies", "lsim_sensor_shade") and cam.shading == opt
    env.step_device(torch.zeros(N, 12))
    assert order == ["lsim_raycast_bodies", "lsim_sensor_shade"]
    st, ss = cam.stage("shade"), cam.stage("shade").struct
    R, stride = W * H, (W * H + 3) // 4 * 4
    assert bytes(ss.rb) == bytes(cam.bodies_struct), "the struct the rays are launched with, embedded"
    assert ss.rb.rc.out == cam.out_rows.data_ptr() and ss.rb.labels == cam.label_rows.data_ptr() and ss.rb.rc.mount == cam.mount.data_ptr()
    assert ss.rb.flags == abi.RAYCAST_FRAME_YAW and ss.rb.rc.env_stride == 2
    assert ss.rgba == st.buffers["rgba"].data_ptr() and ss.surface == st.buffers["surface"].data_ptr() and ss.palette == st.buffers["palette"].data_ptr()
    assert (ss.rgba_stride, ss.shade_flags) == (stride, abi.DEFINES["LSIM_SHADE_SHADOWS"])
    assert [ss.sun[k] for k in range(3)] == [float(np.float32(v)) for v in opt.sun_vector()]
    assert (ss.ambient, ss.checker, ss.checker_gain, ss.shadow_bias, ss.shadow_far) == tuple(float(np.float32(v)) for v in (0.35, 0.5, 0.8, 2e-3, 4.0))
    assert st.buffers["palette"].tolist() == list(opt.palette_words())
    rgba, rgb, surf = cam.rgba_image(), cam.rgb_image(), cam.surface()
    assert rgba.shape == (N, H, W, 4) and rgba.dtype == torch.uint8 and rgb.shape == (N, H, W, 3) and surf.shape == (N, R, 4)
    assert rgba.data_ptr() == ss.rgba and rgb.data_ptr() == ss.rgba and surf.data_ptr() == ss.surface, "views of the buffers that are launched"
    assert bool((rgba[0::2, ..., 3] == 255).all()) and bool((rgba[1::2] == 0).all()), "every second env is drawn"
    lab = cam.label_image()
    assert bool((lab[0] >= 2).any()) and bool((lab[0] == 1).any())
    words = np.asarray(opt.palette_words(), np.uint32)
    sky = lab[0] == 0
    if bool(sky.any()):
        assert set(map(tuple, rgb[0][sky].tolist())) == {(int(words[0]) & 255, (int(words[0]) >> 8) & 255, (int(words[0]) >> 16) & 255)}
    n = surf[0][(lab[0] > 0).reshape(-1), :3]
    assert torch.allclose(n.norm(dim=1), torch.ones(len(n)), atol=1e-5)
    # set_shading(None) drops the launch and the buffers; set again, the frame is the one of before
    before = rgba.clone()
    cam.set_shading(None)
    assert cam.chain() == ("lsim_raycast_bodies",) and cam.stage("shade") is None
    cam.set_shading(opt)
    cam.update()
    assert torch.equal(cam.rgba_image(), before)


def test_spec_round_trip_and_chase_camera():
    env, api = _env(), _api()
    opt = sensors.Shading(sun=(95.0, 40.0), shadows=False, checker=0.25)
    cam = _camera(env, api, shading=opt)
    spec = cam.spec()
    assert list(spec)[-1] == "shading" and spec["shading"] == opt.record() and json.loads(json.dumps(spec)) == spec
    back = sensors.from_spec(env, spec, api=api)
    assert back.shading == opt and back.chain() == cam.chain() and back.spec() == spec
    assert sensors.from_spec(env, spec, api=api, shading=None).shading is None
    other = sensors.Shading(ambient=0.1)
    assert sensors.from_spec(env, spec, api=api, shading=other).shading == other
    with pytest.raises(ValueError, match="shading"):
        sensors.from_spec(env, spec, api=api, shading="yes")
    cam.update(), back.update()
    assert torch.equal(cam.rgba_image(), back.rgba_image())
    chase = sensors.chase_camera(env, 16, 12, api=api, env_stride=4)
    assert (chase.width, chase.height, chase.frame, chase.see_robot, chase.env_stride) == (16, 12, "yaw", True, 4)
    assert chase.shading == sensors.Shading() and chase.chain() == ("lsim_raycast_bodies", "lsim_sensor_shade")
    assert chase.mount[0].tolist() == pytest.approx([-1.2, 0.0, 0.7] + list(sensors.quat_from_pitch(28.0)))
    assert sensors.chase_camera(env, 16, 12, api=api, shading=None).chain() == ("lsim_raycast_bodies",)
    with pytest.raises(ValueError, match="LSIM_RAYCAST_MAX_RAYS"):
        sensors.chase_camera(env, 200, 100, api=api)


def test_ppm_bytes(tmp_path):
    img = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3)
    sensors.write_ppm(tmp_path / "a.ppm", img)
    assert (tmp_path / "a.ppm").read_bytes() == b"P6\n3 2\n255\n" + bytes(range(18))
    with pytest.raises(ValueError):
        sensors.write_ppm(tmp_path / "b.ppm", img[..., :2])
    import importlib.util
    spec = importlib.util.spec_from_file_location("sensor_frames", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "sensor_frames.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tool.write_ppm(tmp_path / "c.ppm", img)
    assert (tmp_path / "c.ppm").read_bytes() == (tmp_path / "a.ppm").read_bytes()


def _policy():
    from isaacgymloco_amd.learn.modules import HIMActorCritic
    torch.manual_seed(0)
    return HIMActorCritic(270, 238, 45, 12, actor_hidden_dims=[32], critic_hidden_dims=[32], activation="elu", init_noise_std=1.0)


def _evaluate(env, ac, **kw):
    from isaacgymloco_amd.learn.evaluate import Evaluator, evaluate
    return evaluate(env, ac, 7, commands=(0.5, 0.0, 0.0), evaluator=Evaluator(env, api=CB.EmuApi()), fused=False, **kw)


def test_evaluate_writes_the_expected_frames_and_the_same_result(tmp_path):
    ac = _policy()
    plain = _evaluate(_env(), ac)
    assert not hasattr(plain, "frames_written")
    api = _api()
    env = _env()
    ev = _evaluate(env, ac, frames={"dir": str(tmp_path / "f"), "every": 3, "envs": (0, 4), "size": (16, 12), "shading": sensors.Shading(sun=(185.0, 22.0)), "api": api})
    names = sorted(os.listdir(tmp_path / "f"))
    ppm = ["e0_s00003.ppm", "e0_s00006.ppm", "e4_s00003.ppm", "e4_s00006.ppm"]
    try:
        import PIL  # noqa: F401
        assert names == sorted(["e0.gif", "e4.gif"] + ppm) and len(ev.frames_written["gifs"]) == 2
    except ImportError:
        assert names == ppm and ev.frames_written["gifs"] == []
    assert [os.path.basename(p) for p in ev.frames_written["frames"]] == ["e0_s00003.ppm", "e4_s00003.ppm", "e0_s00006.ppm", "e4_s00006.ppm"]
    assert api.calls["lsim_sensor_shade"] == 2 == api.calls["lsim_raycast_bodies"], "launched on the steps that write, nothing on the others"
    data = (tmp_path / "f" / "e4_s00006.ppm").read_bytes()
    assert data[:12] == b"P6\n16 12\n255" and len(data) == 13 + 16 * 12 * 3 and len(set(data[13:])) > 4
    assert "frames" not in env.sensors and json.dumps(ev.result(), sort_keys=True) == json.dumps(plain.result(), sort_keys=True)
    for bad in ({"every": 3}, {"dir": str(tmp_path), "every": 0, "api": api}, {"dir": str(tmp_path), "envs": (N,), "api": api}, {"dir": str(tmp_path), "fps": 3}):
        with pytest.raises(ValueError, match="frames"):
            _evaluate(_env(), ac, frames=bad)


def test_cli_parses_the_frames_options():
    from isaacgymloco_amd.learn.evaluate import parse_args
    base = ["--task", "aliengo", "--checkpoint", "m.pt", "--out", "r.json"]
    assert parse_args(base).frames is None
    a = parse_args(base + ["--frames", "out", "--frames-every", "5", "--frames-envs", "0,7", "--frames-size", "64x48", "--frames-shading", "sun=200:20,shadows=0"])
    assert a.frames == {"dir": "out", "every": 5, "envs": (0, 7), "size": (64, 48), "shading": sensors.Shading(sun=(200.0, 20.0), shadows=False)}
    for bad in (["--frames-size", "64"], ["--frames-shading", "moon=1"], ["--frames-envs", "a"]):
        with pytest.raises(SystemExit):
            parse_args(base + ["--frames", "out"] + bad)
