"""GPU: a vision policy after training -- evaluate() on its checkpoint with the two vision metrics as evaluator columns, and the exported
TorchScript module (run on the CPU, as on a robot) against the device pipeline it was exported from."""
import numpy as np
import pytest
import torch

import depth_encoder_emu_binding as DB
import depth_encoder_reference as R
from helpers import abi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, L, STEPS = 64, 10, 20
ENC = dict(c1=4, k1=3, s1=2, c2=8, k2=3, s2=1, latent_dim=L)
W = abi.EVAL_WORDS
# |scan_error mean - float64 recomputation| measured on an MI355X at a mean of 0.452 (fused 9.21e-9, eager 9.13e-9; printed below, DESIGN.md
# section 7.11): the recomputation forms the head's output and the squares in float64 from the recorded rows and targets, the device in fp32
# (10 products and 187 squares per value, ~2e-8 relative) and then 2^-32 = 2.3e-10 fixed point.  The bound is 4 x the measured distance.
SCAN_ERROR_MEASURED = 9.21e-9


def _env(seed):
    from isaacgymloco_amd.envs import config as C
    from isaacgymloco_amd.envs.legged_robot import LeggedRobot
    from isaacgymloco_amd.learn.evaluate import play_cfg
    cfg = play_cfg(C.aliengo_cfg())
    cfg.env.num_envs = N
    cfg.env.episode_length_s = 0.3                  # 15 steps: episodes end inside an evaluation
    cfg.terrain.terrain_proportions = [0.5, 0.0, 0.0, 0.0, 0.25, 0.25]
    env = LeggedRobot(cfg, sim_device=DEV, seed=seed)
    env.reset()
    return env


def _camera(env):
    from isaacgymloco_amd.envs import sensors
    return sensors.depth_camera(env, 16, 12, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0,
                                model=sensors.SensorModel(period=2, stagger=True, latency=1, frames=2, normalise=True))


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """one learning iteration of a VisionOnPolicyRunner at 64 envs, saved: (path, checkpoint dict, runner)"""
    from isaacgymloco_amd.learn.bench_train import train_cfg_dict
    from isaacgymloco_amd.learn.depth_encoder import DepthEncoder
    from isaacgymloco_amd.learn.vision import VisionOnPolicyRunner
    env = _env(5)
    cam = env.add_sensor("depth", _camera(env))
    tc = train_cfg_dict("aliengo")
    tc["runner"]["num_steps_per_env"] = 6
    torch.manual_seed(5)
    run = VisionOnPolicyRunner(env, tc, sensor="depth", encoder=DepthEncoder(12, 16, 2, **ENC), device=DEV)
    run.learn(1)
    with torch.no_grad():                           # depth columns a policy would have after training: far from their small initialisation
        run.alg.actor_critic.actor[0].weight[:, -L:] = 0.5 * torch.randn(run.alg.actor_critic.actor[0].out_features, L, device=DEV)
    path = str(tmp_path_factory.mktemp("vision") / "model.pt")
    run.save(path)
    return path, torch.load(path, map_location="cpu", weights_only=False), run


def _recorded_evaluate(env, cam, policy, **kw):
    """evaluate() with, per step, what the columns were formed from (latent rows, privileged observation) and the step's reset flags"""
    from isaacgymloco_amd.learn.evaluate import evaluate
    rec = []
    step_device = env.step_device

    def recording(a, flags=0):
        rows, priv = cam.latent().clone(), env.get_privileged_observations().clone()
        out = step_device(a, flags)
        rec.append((rows, priv, env.reset_buf.clone(), a.clone()))
        return out
    env.step_device = recording
    ev = evaluate(env, policy, STEPS, commands=(0.8, 0.0, 0.0), **kw)
    env.step_device = step_device
    torch.cuda.synchronize()
    return ev, rec


@pytest.mark.parametrize("fused", [True, False])
def test_evaluate_a_vision_checkpoint_end_to_end(trained, fused):
    from isaacgymloco_amd.envs import sensors
    from isaacgymloco_amd.learn.vision import height_scan_block
    path, d, run = trained
    assert d["vision"]["latent_dim"] == L and d["vision"]["encoder"]["latent_dim"] == L and d["vision"]["sensor"]["kind"] == "camera"
    env = _env(9)
    cam = env.add_sensor("depth", sensors.from_spec(env, d["vision"]["sensor"]))     # as the command line builds it
    ev, rec = _recorded_evaluate(env, cam, path, fused=fused)
    res = ev.result()
    assert res["steps"] == STEPS and res["conventions"]["columns"] == ["depth_influence", "scan_error"]
    table, ctable = ev.table.cpu().numpy(), ev.col_table.cpu().numpy()
    np.testing.assert_array_equal(ctable[:, 0], table[:, W["samples"]])
    tot = res["total"]
    assert tot["samples"] + tot["episodes"] == N * STEPS and tot["episodes"] > 0 and tot["samples"] > N * STEPS // 2
    assert tot["columns"]["depth_influence"]["nonfinite"] == 0 and tot["columns"]["scan_error"]["nonfinite"] == 0
    assert tot["columns"]["depth_influence"]["mean"] > 0 and all(g["columns"]["depth_influence"]["mean"] > 0 for g in res["groups"] if g["samples"])
    # scan_error against a float64 recomputation from the recorded rows and targets, over the env-steps that were samples
    off, width = height_scan_block(env.cfg)
    hw, hb = (d["depth_head_state_dict"][k].double().numpy() for k in ("weight", "bias"))
    total, count = 0.0, 0
    for rows, priv, reset, _ in rec:
        live = ~reset.cpu().numpy().astype(bool)
        pred = rows.cpu().double().numpy() @ hw.T + hb
        err = ((pred - priv[:, off:off + width].cpu().double().numpy()) ** 2).mean(axis=1)
        total += float(err[live].sum())
        count += int(live.sum())
    assert count == tot["samples"]
    dist = abs(tot["columns"]["scan_error"]["mean"] - total / count)
    print(f"fused={fused}: scan_error mean {tot['columns']['scan_error']['mean']:.9e}, float64 recomputation {total / count:.9e}, distance {dist:.3e} "
          f"(relative {dist / (total / count):.3e})")
    assert dist <= 4 * SCAN_ERROR_MEASURED
    assert int(env.nonfinite_envs) == 0


@pytest.mark.parametrize("fused", [True, False])
def test_warm_started_twin_has_no_depth_influence(fused):
    from isaacgymloco_amd.learn.depth_encoder import DepthEncoder
    from isaacgymloco_amd.learn.evaluate import evaluate
    from isaacgymloco_amd.learn.modules import HIMActorCritic
    from isaacgymloco_amd.learn.vision import VisionActorCritic
    torch.manual_seed(3)
    env = _env(9)
    cam = env.add_sensor("depth", _camera(env))
    him = HIMActorCritic(env.num_obs, env.num_privileged_obs, env.num_one_step_obs, env.num_actions).to(DEV)
    vis = VisionActorCritic(env.num_obs, env.num_privileged_obs, env.num_one_step_obs, env.num_actions, depth_latent_dim=L).to(DEV)
    vis.load_him_state_dict(him.state_dict())
    ev = evaluate(env, vis, STEPS, commands=(0.8, 0.0, 0.0), sensor=cam, encoder=DepthEncoder(12, 16, 2, **ENC), fused=fused)
    res = ev.result()
    assert res["conventions"]["columns"] == ["depth_influence"]             # no head: scan_error is dropped, not zero
    assert res["total"]["columns"]["depth_influence"] == {"mean": 0.0, "rms": 0.0, "nonfinite": 0} and res["total"]["samples"] > 0
    assert cam.latent().abs().sum() > 0
    np.testing.assert_array_equal(ev.col_table.cpu().numpy()[:, 0], ev.table.cpu().numpy()[:, W["samples"]])


def test_exported_module_on_the_cpu_against_the_device_pipeline(trained, tmp_path):
    """two stages with the project's bounds: encode(frames) against the sensor's live latent (both are fp32 evaluations within the bound
    tests/test_gpu_depth_encoder.py holds the kernel to, so they are within twice it of each other), act(obs, latent) against
    lsim_policy_forward_ext's means at the tolerance of tests/test_gpu_vision_policy.py"""
    from isaacgymloco_amd.learn.vision import PackedVisionPolicy
    path, d, run = trained
    env, cam, ac, enc = run.env, run.sensor, run.alg.actor_critic, run.alg.encoder
    mod = torch.jit.load(run.export(str(tmp_path / "exported")))
    g = torch.Generator().manual_seed(1)
    for _ in range(3):
        env.step_device((torch.randn(N, 12, generator=g) * 0.5).to(DEV))
    torch.cuda.synchronize()
    frames, latent = cam.frame_images().cpu(), cam.latent().cpu()
    want, bound = R.encode(frames.numpy().astype(np.float64), DB.params_of(enc), ENC["s1"], ENC["s2"], True)
    with torch.no_grad():
        z = mod.encode(frames)
    print("encode: worst |export - fp64| / bound", float((np.abs(z.numpy() - want) / bound).max()), "worst |device - fp64| / bound",
          float((np.abs(latent.numpy() - want) / bound).max()))
    assert (np.abs(z.numpy() - want) <= bound).all() and (np.abs(latent.numpy() - want) <= bound).all()
    assert (np.abs(z.numpy() - latent.numpy()) <= 2 * bound).all() and np.abs(want).max() > 1e-3
    assert PackedVisionPolicy.supported(ac)
    obs, priv = env.get_observations(), env.get_privileged_observations()
    mean, values = torch.empty(N, env.num_actions, device=DEV), torch.empty(N, 1, device=DEV)
    PackedVisionPolicy(ac).forward(obs, priv, mean, values, rows=cam.latent())
    torch.cuda.synchronize()
    with torch.no_grad():
        got = mod.act(obs.cpu(), latent)
    print("act: max |export - device|", float((got - mean.cpu()).abs().max()), "scale", float(mean.abs().max()))
    torch.testing.assert_close(got, mean.cpu(), rtol=2e-4, atol=2e-5 * float(mean.abs().max()))
    # and the clip / normalisation constants are the sensor's
    assert (mod.clip_lo, mod.clip_hi, mod.offset, mod.gain) == tuple(float(getattr(cam.stage("capture").struct, k)) for k in ("clip_lo", "clip_hi", "offset", "gain"))
