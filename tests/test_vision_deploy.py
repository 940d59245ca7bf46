"""CPU: what is done with a trained vision policy (learn/vision.py) -- the checkpoint's record of encoder and camera, evaluate() on it, and
the exported TorchScript module (learn/export.py, PolicyExporterVision).  The env is the product's LeggedRobot surface over the lane
emulator of kernels A / B, sensor, encoder and evaluator run through the CPU builds of their kernel sources."""
import os

import numpy as np
import pytest
import torch

import depth_encoder_emu_binding as DB
import eval_columns_emu_binding as CB
from helpers import C
from isaacgymloco_amd.envs import sensors
from isaacgymloco_amd.learn import vision as V
from isaacgymloco_amd.learn.depth_encoder import DepthEncoder
from isaacgymloco_amd.learn.export import PolicyExporterHIM, PolicyExporterVision, export_policy_as_jit
from isaacgymloco_amd.learn.modules import HIMActorCritic

O, P, N1, A = 270, 238, 45, 12
L = 10
ENC = dict(c1=4, k1=3, s1=2, c2=8, k2=3, s2=1, latent_dim=L)
MODEL = dict(period=2, stagger=True, latency=1, frames=2, clip=(0.1, 3.0), normalise=True)


def _perturb(module, scale=0.05):
    with torch.no_grad():
        for p in module.parameters():
            p.add_(scale * torch.randn_like(p))


def _env(N=8, seed=3, mixed=False):
    from emu_env import EmuLeggedRobot
    from isaacgymloco_amd.learn.evaluate import play_cfg
    cfg = play_cfg(C.mixed_cfg("aliengo", {"aliengo": 0.5, "go2": 0.5})[0] if mixed else C.aliengo_cfg())
    cfg.env.num_envs = N
    cfg.terrain.num_rows, cfg.terrain.num_cols = 2, 2
    cfg.terrain.terrain_proportions = [0.0, 0.0, 0.0, 0.0, 0.5, 0.5]
    env = EmuLeggedRobot(cfg, seed=seed)
    env.reset()
    return env


def _camera(env, api, **kw):
    return sensors.depth_camera(env, 16, 12, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, api=api, model=sensors.SensorModel(**MODEL), **kw)


def _policy(seed=3, spec=None):
    """(VisionActorCritic, DepthEncoder, sensor spec) away from their initialisation"""
    torch.manual_seed(seed)
    ac = V.VisionActorCritic(O, P, N1, A, depth_latent_dim=L)
    enc = DepthEncoder(12, 16, 2, **ENC)
    _perturb(ac)
    _perturb(enc)
    return ac, enc


@pytest.fixture(scope="module")
def cam_spec():
    env = _env()
    return _camera(env, DB.EmuApi()).spec()


# ---- export
def test_exported_vision_module_reproduces_the_policy(tmp_path, cam_spec):
    """forward == act_inference(obs, encoder(frames)) and act(obs, encode(frames)) == forward, at the tolerance tests/test_export.py applies"""
    ac, enc = _policy()
    path = export_policy_as_jit(ac, str(tmp_path / "exported"), encoder=enc, sensor=cam_spec)
    assert os.path.basename(path) == "policy.pt"
    mod = torch.jit.load(path)
    obs, frames = torch.randn(37, O), torch.rand(37, 2, 12, 16) - 0.5
    with torch.no_grad():
        want = ac.act_inference(obs, depth_latent=enc(frames))
        got = mod(obs, frames)
        z = mod.encode(frames)
        np.testing.assert_allclose(z.numpy(), enc(frames).numpy(), rtol=0, atol=1e-6)
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=1e-6)
        assert torch.equal(mod.act(obs, z), got)
    assert got.shape == (37, A) and z.shape == (37, L)
    assert (mod.clip_lo, mod.clip_hi) == (float(np.float32(0.1)), 3.0) and (mod.period, mod.latency, mod.frames, mod.height, mod.width) == (2, 1, 2, 12, 16)
    assert mod.offset == float(np.float32(1.55)) and mod.gain == float(np.float32(1.0 / 2.9))
    assert all(k.split(".")[0] in ("actor", "estimator", "conv1", "conv2", "fc") for k in mod.state_dict())


def test_warm_started_twin_exports_to_the_him_policys_outputs(tmp_path, cam_spec):
    torch.manual_seed(1)
    him = HIMActorCritic(O, P, N1, A)
    _perturb(him)
    vis = V.VisionActorCritic(O, P, N1, A, depth_latent_dim=L)
    vis.load_him_state_dict(him.state_dict())
    _, enc = _policy(4)
    a = torch.jit.load(export_policy_as_jit(him, str(tmp_path / "him")))
    b = torch.jit.load(export_policy_as_jit(vis, str(tmp_path / "vis"), encoder=enc, sensor=cam_spec))
    obs = torch.randn(9, O)
    with torch.no_grad():
        want = a(obs)
        for frames in (torch.rand(9, 2, 12, 16), 1e3 * torch.randn(9, 2, 12, 16), torch.zeros(9, 2, 12, 16)):
            assert torch.equal(b(obs, frames), want)


def test_export_refusals_and_unchanged_him_export(tmp_path, cam_spec):
    ac, enc = _policy()
    for kw in ({}, {"encoder": enc}, {"sensor": cam_spec}):
        with pytest.raises(ValueError, match="encoder"):
            export_policy_as_jit(ac, str(tmp_path / "no"), **kw)
    assert not os.path.exists(str(tmp_path / "no" / "policy.pt"))
    with pytest.raises(ValueError, match="SensorModel"):
        PolicyExporterVision(ac, enc, dict(cam_spec, model=None))
    with pytest.raises(ValueError, match="frames"):
        PolicyExporterVision(ac, DepthEncoder(12, 16, 1, **ENC), cam_spec)
    # the HIM export: the module tree and state-dict keys of before (tests/test_export.py holds the outputs)
    him = HIMActorCritic(O, P, N1, A)
    mod = torch.jit.load(export_policy_as_jit(him, str(tmp_path / "him")))
    keys = [f"{net}.{i}.{w}" for net, idx in (("actor", (0, 2, 4, 6)), ("estimator", (0, 2, 4))) for i in idx for w in ("weight", "bias")]
    assert list(mod.state_dict()) == keys == list(PolicyExporterHIM(him).state_dict())
    assert [n for n, _ in mod.named_children()] == ["actor", "estimator"]
    assert not hasattr(mod, "encode") and not hasattr(mod, "preprocess")

    class Bare(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.actor = torch.nn.Sequential(torch.nn.Linear(5, 3))
    assert os.path.basename(export_policy_as_jit(Bare(), str(tmp_path / "bare"))) == "policy_1.pt"


def test_preprocess_is_the_sensor_models_clip_and_normalisation():
    """a sensor with zero noise, zero dropout, latency 0, one frame, normalise: its frame is preprocess(its clean image), bit for bit"""
    env = _env(N=4)
    cam = env.add_sensor("depth", sensors.depth_camera(env, 16, 12, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, near=0.05, far=5.0, api=DB.EmuApi(),
                                                       model=sensors.SensorModel(latency=0, frames=1, clip=(0.3, 1.1), normalise=True)))
    g = torch.Generator().manual_seed(0)
    for _ in range(3):
        env.step_device(torch.randn(4, 12, generator=g) * 0.3)
    ac, _ = _policy()
    enc = DepthEncoder(12, 16, 1, **ENC)
    mod = torch.jit.script(PolicyExporterVision(ac, enc, cam))
    img, frame = cam.image().clone(), cam.frame_images()[:, 0].clone()
    assert (img < 0.3).any() or (img > 1.1).any(), "the clip must act"
    assert frame.min() >= -0.5 - 1e-6 and frame.max() <= 0.5 + 1e-6 and frame.min() < frame.max()      # fp32: (hi - offset) * gain may round past 0.5
    assert torch.equal(mod.preprocess(img), frame)


# ---- the checkpoint's record
def test_spec_round_trips_through_from_spec():
    env = _env(N=8, mixed=True)
    api = DB.EmuApi()
    mounts = {"aliengo": (0.3, 0.0, 0.05), "go2": (0.25, 0.0, 0.03)}
    cam = sensors.depth_camera(env, 8, 6, 87.0, mount_pos=mounts, pitch_deg=30.0, near=0.07, far=4.0, api=api, see_robot=True,
                               ignore_bodies=("base", "FL_calf"), labels=True, frame="yaw",
                               model=sensors.SensorModel(period=3, stagger=True, latency=1, frames=2, noise=(0.01, 0.002), dropout=0.02, drop_value=0.5,
                                                         clip=(0.1, 3.0), normalise=True))
    spec = cam.spec()
    import json
    assert json.loads(json.dumps(spec)) == spec                           # plain values and lists
    assert spec["kind"] == "camera" and (spec["width"], spec["height"]) == (8, 6) and set(spec["mount"]) == {"aliengo", "go2"}
    assert set(spec["ignore_bodies"]) == {n for n in cam.body_names if n == "base" or n == "FL_calf"} and len(spec["ignore_bodies"]) == 2
    twin = sensors.from_spec(env, spec, api=api)
    assert isinstance(twin, sensors.DepthCamera) and (twin.width, twin.height) == (8, 6)
    assert torch.equal(twin.dirs, cam.dirs) and torch.equal(twin.scale, cam.scale) and torch.equal(twin.mount, cam.mount)
    assert twin.body_mask == cam.body_mask and twin.body_mask != (1 << 17) - 1 and twin.frame == "yaw" and twin.see_robot and twin.label_rows is not None
    assert (twin.near, twin.far, twin.env_stride) == (cam.near, cam.far, cam.env_stride)
    for k in ("period", "stagger", "latency", "frames", "sigma0", "sigma2", "p_drop", "drop_value", "clip_lo", "clip_hi", "offset", "gain"):
        assert getattr(twin.stage("capture").struct, k) == getattr(cam.stage("capture").struct, k), k
    assert twin.spec() == spec
    # one pose for all envs; a lidar; a mount that differs from env to env
    one = sensors.depth_camera(env, 8, 6, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, api=api).spec()
    assert one["mount"] == {"pos": [np.float32(0.3), 0.0, np.float32(0.05)], "quat": one["mount"]["quat"]} and one["model"] is None and one["ignore_bodies"] == []
    lid = sensors.lidar(env, 2, 20.0, 24, mount_pos=(0.0, 0.0, 0.12), far=6.0, api=api)
    back = sensors.from_spec(env, lid.spec(), api=api)
    assert lid.spec()["kind"] == "lidar" and (back.channels, back.points_per_rev) == (2, 24) and back.scale is None and torch.equal(back.dirs, lid.dirs)
    per_env = torch.zeros(8, 3)
    per_env[:, 0] = torch.arange(8) * 0.01
    odd = sensors.RaySensor(env, lid.dirs.numpy(), mount_pos=per_env, api=api)
    assert odd.spec()["mount"] is None and odd.spec()["kind"] == "rays"
    with pytest.raises(ValueError, match="mount"):
        sensors.from_spec(env, odd.spec(), api=api)
    again = sensors.from_spec(env, odd.spec(), mount_pos=per_env, mount_quat=(0.0, 0.0, 0.0, 1.0), api=api)
    assert torch.equal(again.mount, odd.mount)


def test_encoder_config_rebuilds_the_encoder():
    enc = DepthEncoder(13, 17, 3, c1=5, k1=3, s1=2, c2=19, k2=3, s2=1, latent_dim=33, final_act=False)
    cfg = enc.config()
    assert cfg == dict(height=13, width=17, frames=3, c1=5, k1=3, s1=2, c2=19, k2=3, s2=1, latent_dim=33, final_act=False)
    assert all(type(v) in (int, bool) for v in cfg.values())
    twin = DepthEncoder(**cfg)
    twin.load_state_dict(enc.state_dict())
    assert twin.config() == cfg


# ---- evaluate() on a vision checkpoint
def _runner(env, cam):
    from isaacgymloco_amd.learn.bench_train import train_cfg_dict
    tc = train_cfg_dict("aliengo")
    tc["runner"]["num_steps_per_env"] = 4
    torch.manual_seed(7)
    enc = DepthEncoder(12, 16, 2, **ENC)
    return V.VisionOnPolicyRunner(env, tc, sensor=cam, encoder=enc, device="cpu")


def _evaluate(env, policy, steps=8, **kw):
    from isaacgymloco_amd.learn.evaluate import Evaluator, evaluate
    recorded = []
    step_device = env.step_device
    env.step_device = lambda a, flags=0: (recorded.append(a.clone()), step_device(a, flags))[1]
    ev = evaluate(env, policy, steps, commands=(0.5, 0.0, 0.0), evaluator=Evaluator(env, api=CB.EmuApi()), **kw)
    env.step_device = step_device
    return ev, recorded


def test_checkpoint_holds_the_vision_record_and_evaluates(tmp_path):
    api = DB.EmuApi()
    env = _env()
    cam = env.add_sensor("depth", _camera(env, api))
    run = _runner(env, cam)
    _perturb(run.alg.actor_critic)
    _perturb(run.alg.depth_head, 0.2)
    path = str(tmp_path / "vision.pt")
    run.save(path)
    d = torch.load(path, weights_only=False)
    assert d["vision"] == {"encoder": run.alg.encoder.config(), "sensor": cam.spec(), "latent_dim": L}
    exported = torch.jit.load(run.export(str(tmp_path / "exported")))
    assert exported.latent_dim == L
    # a fresh env whose camera comes from the record, as the command line builds it
    env2 = _env()
    cam2 = env2.add_sensor("depth", sensors.from_spec(env2, d["vision"]["sensor"], api=api))
    ev, recorded = _evaluate(env2, path)
    res = ev.result()
    assert res["steps"] == 8 and len(recorded) == 8 and res["conventions"]["columns"] == ["depth_influence", "scan_error"]
    assert cam2.encoder is not None and all(torch.equal(a, b) for a, b in zip(cam2.encoder.state_dict().values(), run.alg.encoder.state_dict().values()))
    tot = res["total"]
    assert tot["samples"] + tot["episodes"] == 64 and tot["samples"] > 0
    assert tot["columns"]["depth_influence"]["mean"] > 0 and tot["columns"]["scan_error"]["mean"] > 0
    assert tot["columns"]["depth_influence"]["nonfinite"] == 0 and tot["columns"]["scan_error"]["nonfinite"] == 0
    np.testing.assert_array_equal(ev.col_table.numpy()[:, 0], ev.table.numpy()[:, 0])
    # the module with explicit parts resolves to the same policy: same actions on a same-seeded env, same tables
    env3 = _env()
    cam3 = env3.add_sensor("depth", sensors.from_spec(env3, d["vision"]["sensor"], api=api))
    ev3, rec3 = _evaluate(env3, run.alg.actor_critic, sensor=cam3, encoder=run.alg.encoder, depth_head=run.alg.depth_head)
    assert all(torch.equal(a, b) for a, b in zip(rec3, recorded))
    np.testing.assert_array_equal(ev3.col_table.numpy(), ev.col_table.numpy())
    # the runner itself brings sensor, encoder and head (its constructor resets the env: another run, the same bookkeeping)
    ev_r, rec_r = _evaluate(env, run, steps=3)
    assert len(rec_r) == 3 and ev_r.result()["conventions"]["columns"] == ["depth_influence", "scan_error"]
    np.testing.assert_array_equal(ev_r.col_table.numpy()[:, 0], ev_r.table.numpy()[:, 0])
    # metrics are dropped, not zero, when their inputs are missing; none at all makes no columns launch
    env4 = _env()
    env4.add_sensor("depth", sensors.from_spec(env4, d["vision"]["sensor"], api=api))
    stripped = {k: v for k, v in d.items() if k != "depth_head_state_dict"}
    torch.save(stripped, str(tmp_path / "headless.pt"))
    ev4, _ = _evaluate(env4, str(tmp_path / "headless.pt"))
    assert ev4.result()["conventions"]["columns"] == ["depth_influence"]
    env5 = _env()
    env5.add_sensor("depth", sensors.from_spec(env5, d["vision"]["sensor"], api=api))
    ev5, rec5 = _evaluate(env5, path, vision_metrics=())
    assert ev5.columns is None and "columns" not in ev5.result()["total"] and all(torch.equal(a, b) for a, b in zip(rec5, recorded))


def test_checkpoint_without_the_record_raises_and_runs_with_an_encoder(tmp_path):
    api = DB.EmuApi()
    env = _env()
    cam = env.add_sensor("depth", _camera(env, api))
    run = _runner(env, cam)
    path, bare = str(tmp_path / "vision.pt"), str(tmp_path / "bare.pt")
    run.save(path)
    d = torch.load(path, weights_only=False)
    torch.save({k: v for k, v in d.items() if k != "vision"}, bare)
    from isaacgymloco_amd.learn.evaluate import Evaluator, evaluate
    with pytest.raises(ValueError, match="'vision'"):
        evaluate(env, bare, 2, evaluator=Evaluator(env, api=CB.EmuApi()))
    ev, _ = _evaluate(env, bare, steps=3, encoder=DepthEncoder(12, 16, 2, **ENC))
    assert ev.result()["steps"] == 3
    run2 = _runner(_env(), cam)                                            # loading a checkpoint that lacks the record works as before
    run2.load(bare)
    env_blind = _env()                                                    # and a vision policy without any sensor raises
    with pytest.raises(ValueError, match="sensor"):
        evaluate(env_blind, path, 2, evaluator=Evaluator(env_blind, api=CB.EmuApi()))
    with pytest.raises(ValueError, match="SensorModel"):
        evaluate(env_blind, path, 2, evaluator=Evaluator(env_blind, api=CB.EmuApi()),
                 sensor=sensors.depth_camera(env_blind, 16, 12, 87.0, api=api))


def test_blind_warm_started_twin_acts_as_the_him_policy():
    api = DB.EmuApi()
    torch.manual_seed(2)
    him = HIMActorCritic(O, P, N1, A)
    _perturb(him)
    vis = V.VisionActorCritic(O, P, N1, A, depth_latent_dim=L)
    vis.load_him_state_dict(him.state_dict())
    _, enc = _policy(5)
    env_h = _env(seed=4)
    ev_h, rec_h = _evaluate(env_h, him)
    runs = {}
    for blind in (True, False):
        env_v = _env(seed=4)
        cam = env_v.add_sensor("depth", _camera(env_v, api))
        ev_v, rec_v = _evaluate(env_v, vis, sensor=cam, encoder=enc, blind=blind)
        assert len(rec_v) == len(rec_h) == 8 and all(torch.equal(a, b) for a, b in zip(rec_v, rec_h))
        np.testing.assert_array_equal(ev_v.table.numpy(), ev_h.table.numpy())
        runs[blind] = ev_v.result()
    for res in runs.values():                                             # zero depth columns: the latent changes nothing, exactly
        inf = res["total"]["columns"]["depth_influence"]
        assert inf == {"mean": 0.0, "rms": 0.0, "nonfinite": 0} and res["conventions"]["columns"] == ["depth_influence"]
    assert "columns" not in ev_h.result()["total"]
