"""CPU: the PPO gradient into the depth encoder (learn/vision.py, end_to_end=True) on the emulated env -- the sensor's
frame-log stage driven by the eager rollout, the de-duplicated update against the naive per-transition one in fp64, and what the switch
leaves alone when it is off.  tests/test_gpu_vision_end_to_end.py runs the device half."""
import numpy as np
import pytest
import torch

import frames_log_emu_binding as FB
import frames_log_reference as R
from helpers import C
from isaacgymloco_amd.envs import sensors
from isaacgymloco_amd.learn import vision as V
from isaacgymloco_amd.learn.depth_encoder import DepthEncoder
from isaacgymloco_amd.learn.him_ppo import HIMPPO

O, P, N1, A, L = 270, 238, 45, 12, 10
N, T, PERIOD = 8, 6, 3
ENC = dict(c1=4, k1=3, s1=2, c2=8, k2=3, s2=1, latent_dim=L)
MODEL = dict(period=PERIOD, stagger=True, latency=1, frames=2, normalise=True)


def _env(seed=3):
    from emu_env import EmuLeggedRobot
    cfg = C.aliengo_cfg()
    cfg.env.num_envs = N
    cfg.terrain.num_rows, cfg.terrain.num_cols = 2, 2
    cfg.terrain.terrain_proportions = [0.0, 0.0, 0.0, 0.0, 0.5, 0.5]
    env = EmuLeggedRobot(cfg, seed=seed)
    env.reset()
    return env


def _camera(env, api, **kw):
    return sensors.depth_camera(env, 16, 12, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, api=api, model=sensors.SensorModel(**MODEL), **kw)


@pytest.fixture
def fp64():
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(torch.float32)


def _step(env, alg, obs, crit):
    """HIMOnPolicyRunner._rollout_step's device branch"""
    actions = alg.act(obs, crit)
    o, p, rewards, dones = env.step_device(actions.float())
    o, crit = o.to(actions.dtype), p.to(actions.dtype)        # copies: the live buffers are fp32, the learner may be fp64
    alg.process_env_step(rewards, dones, env.extras, torch.where(dones.unsqueeze(1), env.termination_privileged_obs_buf.to(crit.dtype), crit))
    return o, crit, dones


def test_the_log_path_is_the_per_transition_computation(fp64):
    """N = 8, T = 6, a 16 x 12 camera of period 3, a reset inside the rollout, everything above the sensor in fp64: the gradient of the
    first minibatch's PPO loss with respect to the six encoder parameters through frame log, join and one encoder pass over the logged
    images equals the one through encoder(frames[t, n]) per transition to 1e-9 of its largest entry, and the latent recomputed from the
    log is the stored one bit for bit"""
    torch.manual_seed(0)
    env, api = _env(), FB.EmuApi()
    cam = env.add_sensor("depth", _camera(env, api))
    cam.attach_encoder(DepthEncoder(12, 16, 2, **ENC).float())          # the sensor's own fp32 launch: the log stage needs one; its rows are not read here
    ac, enc = V.VisionActorCritic(O, P, N1, A, depth_latent_dim=L), DepthEncoder(12, 16, 2, **ENC)
    assert enc.fc.weight.dtype == torch.float64
    alg = V.VisionPPO(ac, encoder=enc, latent_source=lambda: enc(cam.frame_images().double()), frames_source=cam.frame_images, aux_snapshots=0,
                      end_to_end=True, num_learning_epochs=2, num_mini_batches=2, device="cpu")
    alg.init_storage(N, T, [O], [P], [A])
    st = alg.storage
    assert st.frame_row.dtype == torch.int32 and st.frame_row.shape == (T, N) and alg.e2e_learning_rate == alg.aux_learning_rate
    with pytest.raises(RuntimeError, match="no frame log"):
        next(alg._sample_stream())
    cam.attach_frames_log(T, row_of=st.frame_row)
    alg.attach_frame_log(cam)
    assert cam.chain() == ("lsim_sensor_capture", "lsim_sensor_frames_log", "lsim_depth_encode")
    env.episode_length_buf[2] = int(env.max_episode_length) - 2          # env 2 times out, and resets, inside the rollout
    frames = torch.zeros(T, N, 2, 12, 16, dtype=torch.float32)
    ticks, fresh = [], []
    obs, crit = env.get_observations().double(), env.get_privileged_observations().double()
    with torch.inference_mode():
        for t in range(T):
            frames[t] = cam.frame_images()
            ticks.append(int(env.common_step_counter))
            obs, crit, dones = _step(env, alg, obs, crit)
            fresh.append(dones.clone())
        alg.compute_returns(crit)
    assert cam.stage("frames_log").step is None and int(torch.stack(fresh).sum()) >= 1 and bool(torch.stack(fresh)[:, 2].any())
    # the stage wrote what the state machine writes for this rollout's ticks and resets
    ref = R.FramesLog(N, T, cam.frames_log().shape[0], 2, 192, 192, PERIOD, 1, log_fill=np.float32(0.0), int_fill=-1)
    assert cam.frames_log().shape[0] == R.default_capacity(N, T, PERIOD) == N * 5
    el = np.ones(N, dtype=np.int64)
    ref.launch(frames[0].flatten(2).numpy(), el, max(ticks[0] - 1, 0), 0, R.FILL_ALL)
    for t in range(1, T):
        ref.launch(frames[t].flatten(2).numpy(), np.where(fresh[t - 1].numpy(), 0, 1).astype(np.int64), ticks[t - 1], t, 0)
    rows = int(ref.state[R.COUNT])
    assert cam.frames_log_state()[:2].tolist() == [rows, 0] and N < rows < T * N
    assert np.array_equal(st.frame_row.numpy(), ref.row_of) and np.array_equal(cam.frames_log_sources().numpy()[:rows], ref.row_src[:rows])
    assert np.array_equal(cam.frames_log().numpy()[:rows], ref.log[:rows])
    assert torch.equal(cam.frames_log()[st.frame_row.long()].unflatten(3, (12, 16)), frames)         # every transition finds its own frames in the log

    gen = alg._sample_stream()
    batch, _ = next(gen)
    batch = tuple(b.double() if b.is_floating_point() else b for b in batch)         # the storage's ten fields are fp32 whatever the learner is
    assert len(batch) == 12 and alg._e2e_minibatch == 0 and alg._e2e_rows == rows
    B = batch[0].shape[0]
    picked = st.last_perm[:B]
    assert torch.equal(batch[11], st.frame_row.flatten()[picked]) and bool((batch[11] >= 0).all())
    params = list(enc.parameters())
    assert len(params) == 6
    joined = alg.joined_rows(batch[10], batch[11], 0)
    assert joined.requires_grad and torch.equal(joined.detach(), batch[10]), "the latent recomputed from the log is the stored row, bit for bit"
    mb = alg._mb_forward(ac, batch, False)
    g_log = torch.autograd.grad(mb.loss, params)
    naive = enc(frames.flatten(0, 1)[picked].double())
    with ac.bound_latent(naive, live=True):
        mb2 = HIMPPO._mb_forward(alg, ac, batch[:10], False)
    g_naive = torch.autograd.grad(mb2.loss, params)
    for name, a, b in zip(("w1", "b1", "w2", "b2", "w3", "b3"), g_log, g_naive):
        scale = float(b.abs().max())
        err = float((a - b).abs().max())
        print(name, "max |log path - per transition|", err, "largest entry", scale)
        assert scale > 0.0 and err <= 1e-9 * scale, (name, err, scale)
    gen.close()
    assert alg._e2e_minibatch is None


def _runner(env, cam, end_to_end, epochs=2, **alg_keys):
    from isaacgymloco_amd.learn.bench_train import train_cfg_dict
    tc = train_cfg_dict("aliengo")
    tc["runner"]["num_steps_per_env"] = T
    tc["algorithm"].update(num_learning_epochs=epochs, num_mini_batches=2, aux_snapshots=0, **alg_keys)
    torch.manual_seed(7)
    return V.VisionOnPolicyRunner(env, tc, sensor=cam, encoder=DepthEncoder(12, 16, 2, **ENC), device="cpu", end_to_end=end_to_end)


def test_one_iteration_moves_the_encoder_only_with_the_switch_on_and_the_checkpoint_follows(tmp_path):
    moved = {}
    for on in (False, True):
        env, api = _env(), FB.EmuApi()
        cam = env.add_sensor("depth", _camera(env, api))
        before_spec = cam.spec()
        run = _runner(env, cam, on, e2e_epochs=1, e2e_learning_rate=3e-4) if on else _runner(env, cam, on)
        alg = run.alg
        start = [p.detach().clone() for p in alg.encoder.parameters()]
        run.learn(1)
        moved[on] = [bool((p != q).any()) for p, q in zip(alg.encoder.parameters(), start)]
        assert all(p.grad is None for p in alg.encoder.parameters())
        path = str(tmp_path / f"e2e_{on}.pt")
        run.save(path)
        d = torch.load(path, weights_only=False)
        assert cam.spec() == before_spec == d["vision"]["sensor"], "the log is no part of the camera's record"
        if not on:
            assert cam.chain() == ("lsim_sensor_capture", "lsim_depth_encode") and cam.stage("frames_log") is None
            assert alg.storage.frame_row is None and alg.e2e_optimizer is None and len(alg.storage._extra_fields()) == 1
            assert "depth_e2e_optimizer_state_dict" not in d and "end_to_end" not in d["vision"]
            with pytest.raises(ValueError, match="frame log"):
                cam.frame_rows()
            continue
        assert cam.chain() == ("lsim_sensor_capture", "lsim_sensor_frames_log", "lsim_depth_encode")
        assert alg.storage.frame_row.data_ptr() == cam.frame_rows().data_ptr() and alg.e2e_optimizer.param_groups[0]["lr"] == 3e-4
        assert d["vision"]["end_to_end"] == {"epochs": 1, "learning_rate": 3e-4, "capacity": N * 5}
        assert len(d["depth_e2e_optimizer_state_dict"]["state"]) == 6
        env2 = _env()
        cam2 = env2.add_sensor("depth", _camera(env2, api))
        run2 = _runner(env2, cam2, True, e2e_epochs=1, e2e_learning_rate=3e-4)
        run2.load(path)
        for a, b in zip(alg.encoder.parameters(), run2.alg.encoder.parameters()):
            assert torch.equal(a, b)
        sa, sb = alg.e2e_optimizer.state_dict()["state"], run2.alg.e2e_optimizer.state_dict()["state"]
        assert all(torch.equal(sa[k]["exp_avg"], sb[k]["exp_avg"]) and torch.equal(sa[k]["exp_avg_sq"], sb[k]["exp_avg_sq"]) for k in sa)
        run2.learn(1)
        assert all(bool(torch.isfinite(p).all()) for p in run2.alg.encoder.parameters())
    assert moved[True] == [True] * 6 and moved[False] == [False] * 6, moved


def test_the_stage_refuses_what_it_cannot_log_and_idles_between_rollouts():
    env, api = _env(), FB.EmuApi()
    cam = env.add_sensor("depth", _camera(env, api))
    with pytest.raises(ValueError, match="no encoder"):
        cam.attach_frames_log(T)
    strided = _camera(env, api, env_stride=2)
    strided.attach_encoder(DepthEncoder(12, 16, 2, **ENC))
    with pytest.raises(ValueError, match="env_stride"):
        strided.attach_frames_log(T)
    cam.attach_encoder(DepthEncoder(12, 16, 2, **ENC))
    with pytest.raises(ValueError, match="row_of"):
        cam.attach_frames_log(T, row_of=torch.zeros(T, N, dtype=torch.int64))
    stage = cam.attach_frames_log(T, capacity=13)
    assert set(stage.buffers) == {"log", "row_of", "row_src", "state"} and cam.frames_log().shape == (13, 2, 192) and stage.option == (T, 13)
    calls = []
    inner = api.lsim_sensor_frames_log
    api.lsim_sensor_frames_log = lambda *a: (calls.append(1), inner(*a))[1]
    env.step_device(torch.zeros(N, 12))                      # nobody drives the log: idle
    env.reset_idx([1])
    cam.refresh()
    assert not calls and cam.frames_log_state().tolist() == [0, 0, 0, 0]
    cam.begin_rollout()
    assert len(calls) == 1 and cam.frames_log_state()[0] == N and stage.step == 1
    assert cam.frame_rows()[0].tolist() == list(range(N)) and bool((cam.frame_rows()[1:] == -1).all())
    env.step_device(torch.zeros(N, 12))
    env.reset_idx([1])                                       # a reset by hand inside the rollout: RESETS_ONLY, the same storage row
    assert len(calls) == 3 and cam.frame_rows()[1, 1] == cam.frames_log_state()[0] - 1
    with pytest.raises(RuntimeError, match="middle of a rollout"):
        cam.refresh()
    for s in range(2, T + 1):
        cam.set_frames_log_step(s)
        env.step_device(torch.zeros(N, 12))
    assert len(calls) == 3 + (T - 2) and stage.step is None         # the step behind the rollout's last row launched nothing
    assert cam.frames_log_state()[0] == 13 and cam.frames_log_state()[1] > 0      # thirteen rows were too few, and the launch said so
    cam.attach_encoder(None)                                  # the log goes with the encoder
    assert cam.stage("frames_log") is None and cam.chain() == ("lsim_sensor_capture",)
