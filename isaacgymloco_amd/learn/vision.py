"""Vision policy: the depth encoder's latent row (learn/depth_encoder.py) as one more input segment of the HIM actor, from the rollout to
the PPO update.

    cam = env.add_sensor("depth", depth_camera(env, 64, 48, 87.0, model=SensorModel(period=5, stagger=True, latency=1, frames=2, normalise=True)))
    runner = VisionOnPolicyRunner(env, train_cfg, sensor="depth", device=dev)
    runner.enable_graphs()
    runner.learn(n)

Three decisions bound the memory and the code:
  1. The actor reads the latent DETACHED, as it reads the estimator's output (HAC:136-141): the rollout stores, per transition, the row the
     actor saw ([T, N, L] floats; the frames would be [T, N, frames, H, W]) and the update feeds that row back.  By default no PPO gradient
     reaches the encoder.  `end_to_end=True` adds one: the sensor logs every image a capture of the rollout showed
     the encoder ONCE (envs/sensors.py, attach_frames_log: with a period-5 camera a fifth of the transitions), the storage keeps per
     transition the row of that log (frame_row), and in the first `e2e_epochs` epochs of the update every minibatch encodes the logged
     images again under autograd, the actor reads those rows, and lsim_latent_rows_grad sums the minibatch's latent gradients per image
     for the encoder's backward.  The encoder then takes an Adam step of its own behind the minibatch's PPO step.
  2. The encoder is trained by an auxiliary regression of its own: frames -> latent -> linear head -> the height scan the critic already
     receives as privileged information, on a few snapshots of one rollout, with its own Adam.  Encoder, head and that optimiser belong to
     VisionPPO, not to the actor-critic: HIMPPO.optimizer, the GradArena buckets and the fused clip + Adam step see the parameters they
     see for a HIM policy, the first actor layer merely being wider.
  3. The depth columns come LAST in the actor input, [obs_now (n1) | vel (3) | z (nl) | depth (L)]: a HIM policy warm-starts a vision policy
     by copying actor.0.weight into the first n1 + 3 + nl columns and zeroing the rest (load_him_state_dict), and is then arithmetically
     the HIM policy.
On the device the rollout step is the fused launch with the extra segment (include/lsim.h, lsim_policy_act_post_at_ext); topologies that
launch does not take use the eager rollout.  One rank only."""
import contextlib
import copy
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import abi, lib
from . import policy_io
from .fused_policy import PackedHimPolicy
from .graph_rollout import GraphedRollout
from .him_ppo import HIMPPO
from .modules import HIMActorCritic, get_activation, mlp
from .runner import _ALGOS, _POLICIES, HIMOnPolicyRunner
from .storage import HIMRolloutStorage, Transition


def height_scan_block(cfg=None):
    """(offset, width) of the height scan inside a privileged observation row, from the layout the env assembles (csrc/ls_post.h,
    ph_build_obs: the LSIM_NUM_HEIGHT_PTS samples are the row's last entries).  `cfg`: the env's config; one without measure_heights
    has zeros there, which is no regression target, and raises."""
    if cfg is not None and not bool(getattr(getattr(cfg, "terrain", None), "measure_heights", False)):
        raise ValueError("the vision policy's encoder regresses the height scan of the privileged observation: the config needs terrain.measure_heights")
    width = abi.DEFINES["LSIM_NUM_HEIGHT_PTS"]
    return abi.DEFINES["LSIM_NUM_PRIV_OBS"] - width, width


class VisionActorCritic(HIMActorCritic):
    """HIMActorCritic whose actor reads `depth_latent_dim` more columns: actor = mlp([n1 + 3 + 16 + L, ...]); critic and estimator unchanged.
    The latent is an explicit argument wherever the actor is evaluated (act, act_inference, update_distribution, _actor_input), or bound for
    the extent of a `with bound_latent(rows):` block (HIMPPO._mb_forward calls _actor_input(obs)).  A missing latent raises."""

    def __init__(self, num_actor_obs, num_critic_obs, num_one_step_obs, num_actions, depth_latent_dim=64, actor_hidden_dims=(512, 256, 128),
                 activation="elu", **kwargs):
        super().__init__(num_actor_obs, num_critic_obs, num_one_step_obs, num_actions, actor_hidden_dims=actor_hidden_dims, activation=activation, **kwargs)
        self.depth_latent_dim = int(depth_latent_dim)
        if self.depth_latent_dim < 1:
            raise ValueError("VisionActorCritic: depth_latent_dim >= 1")
        self.num_him_actor_inputs = self.actor[0].in_features
        self.actor = mlp([self.num_him_actor_inputs + self.depth_latent_dim, *actor_hidden_dims, num_actions], get_activation(activation))
        self._bound_latent, self._latent_live = None, False

    @contextlib.contextmanager
    def bound_latent(self, rows, live=False):
        """inside the block the actor reads `rows` [B, L] wherever no latent is passed (one minibatch of the update).  `live`: the rows
        keep their autograd history, so a loss on the actor's output reaches whatever produced them (the end-to-end update)"""
        prev, self._bound_latent, self._latent_live = (self._bound_latent, self._latent_live), rows, bool(live)
        try:
            yield self
        finally:
            self._bound_latent, self._latent_live = prev

    def _latent_rows(self, depth_latent, batch):
        rows = depth_latent if depth_latent is not None else self._bound_latent
        if rows is None:
            raise ValueError("VisionActorCritic: no depth latent (pass depth_latent=..., or evaluate inside `with bound_latent(rows):`)")
        if rows.dim() != 2 or rows.shape[0] != batch or rows.shape[1] != self.depth_latent_dim:
            raise ValueError(f"VisionActorCritic: the depth latent must be [{batch}, {self.depth_latent_dim}], got {tuple(rows.shape)}")
        return rows if depth_latent is None and self._latent_live else rows.detach()

    def _actor_input(self, obs_history, depth_latent=None):
        rows = self._latent_rows(depth_latent, obs_history.shape[0])
        return torch.cat((super()._actor_input(obs_history), rows), dim=-1)

    def update_distribution(self, obs_history, depth_latent=None):
        with self.bound_latent(self._latent_rows(depth_latent, obs_history.shape[0]), live=self._latent_live):
            super().update_distribution(obs_history)

    def act(self, obs_history=None, depth_latent=None, **kwargs):
        self.update_distribution(obs_history, depth_latent)
        return self.distribution.sample()

    def act_inference(self, obs_history, depth_latent=None, observations=None):
        return self.actor(self._actor_input(obs_history, depth_latent))

    @torch.no_grad()
    def load_him_state_dict(self, sd):
        """warm start from a HIMActorCritic's state dict: actor.0.weight goes into the first n1 + 3 + nl columns, the depth columns are zero --
        the policy then computes the HIM policy's means whatever the latent holds"""
        sd = dict(sd)
        w = sd["actor.0.weight"]
        k = self.num_him_actor_inputs
        if tuple(w.shape) != (self.actor[0].out_features, k):
            raise ValueError(f"load_him_state_dict: actor.0.weight must be {(self.actor[0].out_features, k)}, got {tuple(w.shape)}")
        wide = torch.zeros_like(self.actor[0].weight)
        wide[:, :k] = w
        sd["actor.0.weight"] = wide
        return self.load_state_dict(sd)


    @torch.no_grad()
    def load_vision_state_dict(self, sd):
        """warm start from a narrower VisionActorCritic's state dict (a vision policy without the depth memory): actor.0.weight goes into
        the first columns, the new ones -- the memory's hidden state -- are zero, so the policy computes that policy's means bit for bit"""
        sd = dict(sd)
        w = sd["actor.0.weight"]
        rows, wide_k = self.actor[0].weight.shape
        if w.dim() != 2 or w.shape[0] != rows or not self.num_him_actor_inputs < w.shape[1] <= wide_k:
            raise ValueError(f"load_vision_state_dict: actor.0.weight must be [{rows}, k] with {self.num_him_actor_inputs} < k <= {wide_k}, got {tuple(w.shape)}")
        wide = torch.zeros_like(self.actor[0].weight)
        wide[:, :w.shape[1]] = w
        sd["actor.0.weight"] = wide
        return self.load_state_dict(sd)

    @torch.no_grad()
    def load_scan_teacher_state_dict(self, sd, scan_dim):
        """warm start a camera student from a scan policy's state dict (learn/scan_policy.py; learn/distill.py): everything is copied,
        of actor.0.weight the first n1 + 3 + nl columns; the teacher's `scan_dim` scan columns are dropped and this policy's depth columns
        are zero -- the student starts as the teacher with a flat scan of zeros, whatever its camera shows"""
        sd = dict(sd)
        w = sd["actor.0.weight"]
        k = self.num_him_actor_inputs
        if tuple(w.shape) != (self.actor[0].out_features, k + int(scan_dim)):
            raise ValueError(f"load_scan_teacher_state_dict: actor.0.weight must be {(self.actor[0].out_features, k + int(scan_dim))}, got {tuple(w.shape)}")
        wide = torch.zeros_like(self.actor[0].weight)
        wide[:, :k] = w[:, :k]
        sd["actor.0.weight"] = wide
        return self.load_state_dict(sd)


class VisionTransition:
    __slots__ = Transition.__slots__ + ("depth_latent",)
    __init__ = Transition.__init__
    clear = Transition.clear


class VisionRolloutStorage(HIMRolloutStorage):
    """HIMRolloutStorage + depth_latent [T, N, L]: the row the actor saw at each transition; the minibatch generator yields it as an
    eleventh field, gathered through the same permutation (and, on the GPU, into a persistent shuffle buffer like the other ten).
    `frame_rows=True` (the end-to-end update): + frame_row [T, N] int32, the row of the sensor's frame log that holds the image the latent
    came from, or -1 -- the log's own row_of, which the sensor's stage writes in place -- yielded as a twelfth field; `last_perm` is then
    the permutation of the latest mini_batch_generator (minibatch i holds the transitions last_perm[i * mb : (i + 1) * mb])."""
    Transition = VisionTransition
    frame_row = last_perm = None

    def __init__(self, num_envs, num_transitions_per_env, obs_shape, privileged_obs_shape, actions_shape, depth_latent_dim, device="cpu", frame_rows=False):
        super().__init__(num_envs, num_transitions_per_env, obs_shape, privileged_obs_shape, actions_shape, device)
        self.depth_latent = torch.zeros(num_transitions_per_env, num_envs, int(depth_latent_dim), device=device)
        if frame_rows:
            self.frame_row = torch.full((num_transitions_per_env, num_envs), -1, dtype=torch.int32, device=device)

    def add_transitions(self, t):
        if self.step >= self.num_transitions_per_env:
            raise AssertionError("Rollout buffer overflow")
        if t.depth_latent is None:
            raise ValueError("VisionRolloutStorage: the transition carries no depth latent")
        self.depth_latent[self.step].copy_(t.depth_latent)
        super().add_transitions(t)

    def _extra_fields(self):
        if self.frame_row is None:
            return (self.depth_latent.flatten(0, 1),)
        return (self.depth_latent.flatten(0, 1), self.frame_row.flatten(0, 1))

    def _shuffle(self, fields, perm):
        if self.frame_row is not None:
            self.last_perm = perm
        return super()._shuffle(fields, perm)


class ActorRowsPPO(HIMPPO):
    """HIMPPO over a VisionActorCritic, whatever the extra actor rows are: act() records `latent_source()` ([N, L], live) with the
    transition and the update binds each minibatch's stored rows to the actor.  Nothing but the actor-critic is trained and update()
    returns HIMPPO.update()'s tuple: learn/map_policy.py's MapPPO is this class; VisionPPO adds the encoder.  One rank only."""
    encoder = None          # VisionPPO's

    def __init__(self, actor_critic, latent_source=None, dist_ctx=None, **kwargs):
        if dist_ctx is not None and getattr(dist_ctx, "world", 1) > 1:
            raise NotImplementedError("VisionPPO: one rank only (the encoder's gradients are not reduced over ranks)")
        super().__init__(actor_critic, dist_ctx=dist_ctx, **kwargs)
        self.transition = VisionRolloutStorage.Transition()
        self.latent_source = latent_source

    def init_storage(self, num_envs, num_transitions_per_env, actor_obs_shape, critic_obs_shape, action_shape):
        self.storage = VisionRolloutStorage(num_envs, num_transitions_per_env, actor_obs_shape, critic_obs_shape, action_shape,
                                            self.actor_critic.depth_latent_dim, self.device, **self._storage_options())

    def _storage_options(self):
        return {}

    def drive_frame_log(self, step):
        """called once per rollout step, before the env steps (act(), VisionRollout._act): nothing to drive here"""

    def _latent_now(self):
        if self.latent_source is None:
            raise RuntimeError("VisionPPO: no latent source (attach(encoder, latent_source, frames_source))")
        return self.latent_source()

    def snapshot_steps(self):
        return []

    def snapshot_if_due(self, step, critic_obs):
        """called once per rollout step, before the env steps (act(), VisionRollout._act): nothing to keep here"""

    def act(self, obs, critic_obs):
        rows = self._latent_now().detach().clone()          # a live sensor buffer: the transition keeps what the actor saw
        self.drive_frame_log(self.storage.step)
        self.snapshot_if_due(self.storage.step, critic_obs)
        with self.actor_critic.bound_latent(rows):
            actions = super().act(obs, critic_obs)
        self.transition.depth_latent = rows
        return actions

    def _mb_forward(self, ac, batch, two_streams):
        with ac.bound_latent(batch[10]):
            return super()._mb_forward(ac, batch[:10], two_streams)


class _LatentJoinFn(torch.autograd.Function):
    """The rows a minibatch's actor reads in an end-to-end epoch: column j < L of row i is z_live[frame_row[i]][j] where frame_row[i] >= 0,
    else stored[i][j]; the columns from L on (a memory's hidden state) are stored[i]'s and stay data.  Backward: G [R, L], the gradient of
    z_live, is lsim_latent_rows_grad over the minibatch's gradient rows on the device -- one fixed-order sum per logged image -- and the
    index_add_ of the same terms elsewhere.  `mb_of`, `row_of`, `row_src`: as in include/lsim.h."""

    @staticmethod
    def forward(ctx, z_live, stored, frame_row, mb_of, row_of, row_src):
        L = z_live.shape[1]
        frame_row = frame_row.reshape(-1)
        logged = frame_row >= 0
        z = torch.where(logged.unsqueeze(1), z_live.index_select(0, frame_row.clamp_min(0).long()), stored[:, :L].to(z_live.dtype))
        ctx.save_for_backward(frame_row, mb_of, row_of, row_src)
        ctx.shape = tuple(z_live.shape)
        return z if stored.shape[1] == L else torch.cat((z, stored[:, L:].to(z.dtype)), dim=1)

    @staticmethod
    def backward(ctx, g):
        frame_row, mb_of, row_of, row_src = ctx.saved_tensors
        R, L = ctx.shape
        if not (g.is_cuda and g.dtype == torch.float32):
            logged = frame_row >= 0
            G = torch.zeros(R, L, dtype=g.dtype, device=g.device)
            G.index_add_(0, frame_row[logged].long(), g[logged][:, :L])
            return G, None, None, None, None, None
        if g.stride(1) != 1:
            g = g.contiguous()
        G = torch.empty(R, (L + 3) // 4 * 4, device=g.device, dtype=torch.float32)
        lg = abi.LsimLatentRowsGrad()
        lg.g, lg.mb_of, lg.row_of, lg.row_src, lg.G = g.data_ptr(), mb_of.data_ptr(), row_of.data_ptr(), row_src.data_ptr(), G.data_ptr()
        lg.batch, lg.rows, lg.latent_dim, lg.g_stride, lg.G_stride = g.shape[0], R, L, g.stride(0), G.stride(0)
        lg.num_steps, lg.num_envs = row_of.shape
        entry = lib.entry(lib.load(), "lsim_latent_rows_grad", "the end-to-end update")
        lib.check(entry(ctypes.byref(lg), torch.cuda.current_stream(g.device).cuda_stream), what="lsim_latent_rows_grad")
        return G[:, :L], None, None, None, None, None


class VisionPPO(ActorRowsPPO):
    """ActorRowsPPO whose rows are a depth encoder's latent (the runner passes sensor.latent), with the encoder's own steps behind the
    update: `aux_snapshots` rollout steps, spread evenly over the T steps, each keep a copy of (frames_source(), height scan of the same
    step's critic observation); one pass over them, one minibatch per snapshot, of  z = encoder(frames), loss = mse(head(z), target),
    Adam(aux_learning_rate) over encoder and head.  update() returns HIMPPO's values plus the mean auxiliary loss."""

    def __init__(self, actor_critic, encoder=None, latent_source=None, frames_source=None, height_scan=None, aux_snapshots=4, aux_learning_rate=1e-3,
                 memory_env_minibatches=4, memory_learning_rate=1e-3, end_to_end=False, e2e_epochs=1, e2e_learning_rate=None, e2e_capacity=None,
                 dist_ctx=None, **kwargs):
        super().__init__(actor_critic, dist_ctx=dist_ctx, **kwargs)
        self.aux_snapshots, self.aux_learning_rate = int(aux_snapshots), float(aux_learning_rate)
        # the PPO gradient into the encoder (module docstring, decision 1): off unless the runner was built with end_to_end=True
        self.end_to_end, self.e2e_epochs = bool(end_to_end), int(e2e_epochs)
        self.e2e_learning_rate = self.aux_learning_rate if e2e_learning_rate is None else float(e2e_learning_rate)
        self.e2e_capacity = None if e2e_capacity is None else int(e2e_capacity)
        self.e2e_optimizer = self.frame_log = None
        self._e2e_minibatch, self._e2e_rows = None, 0
        self.last_e2e_overflow = 0
        self.encoder = self.depth_head = self.aux_optimizer = None
        self.frames_source = self.height_scan = None
        self._snap, self._snap_filled = [], []
        self.last_aux_loss = float("nan")
        self.memory = self.memory_head = self.memory_optimizer = None
        self.memory_env_minibatches, self.memory_learning_rate = int(memory_env_minibatches), float(memory_learning_rate)
        self.memory_api = None                      # tests: the CPU shim behind DepthMemory.sequence_device
        self.last_memory_loss = float("nan")
        if encoder is not None:
            self.attach(encoder, latent_source, frames_source, height_scan)

    def attach(self, encoder, latent_source, frames_source, height_scan=None, memory=None):
        """`encoder`: the DepthEncoder whose latent `latent_source()` returns ([N, L], live); `frames_source()`: the [N, frames, H, W] it
        encodes; `height_scan`: (offset, width) of the regression target inside a critic observation row (default: the env's layout);
        `memory`: a DepthMemory -- `latent_source()` then returns [z | h] ([N, L + H]) and memory_step() trains the cell"""
        L = self.actor_critic.depth_latent_dim - (memory.hidden if memory is not None else 0)
        if encoder.latent_dim != L or (memory is not None and memory.latent_dim != L):
            raise ValueError(f"VisionPPO: the encoder's latent has {encoder.latent_dim} columns, the actor reads {self.actor_critic.depth_latent_dim}"
                             + (f" of which the memory's hidden state is {memory.hidden} and its input {memory.latent_dim}" if memory is not None else ""))
        self.height_scan = tuple(int(v) for v in (height_scan if height_scan is not None else height_scan_block()))
        self.encoder = encoder.to(self.device)
        self.depth_head = nn.Linear(L, self.height_scan[1]).to(self.device)
        self.aux_optimizer = torch.optim.Adam(list(self.encoder.parameters()) + list(self.depth_head.parameters()), lr=self.aux_learning_rate)
        self.latent_source, self.frames_source = latent_source, frames_source
        self._snap, self._snap_filled = [], []
        if memory is not None:
            self.memory = memory.to(self.device)
            self.memory_head = nn.Linear(memory.hidden, self.height_scan[1]).to(self.device)
            self.memory_optimizer = torch.optim.Adam(list(self.memory.parameters()) + list(self.memory_head.parameters()), lr=self.memory_learning_rate)
        if self.end_to_end:
            self.e2e_optimizer = torch.optim.Adam(list(self.encoder.parameters()), lr=self.e2e_learning_rate)

    # ---- the PPO gradient into the encoder (end_to_end=True): the sensor's frame log, driven by the rollout and read by the update
    def _storage_options(self):
        return {"frame_rows": True} if self.end_to_end else {}

    def attach_frame_log(self, sensor):
        """`sensor`: the one whose latent the actor reads, with its frame log attached over this storage's frame_row
        (sensor.attach_frames_log(T, capacity, row_of=storage.frame_row))"""
        if not self.end_to_end or self.encoder is None:
            raise RuntimeError("VisionPPO: attach_frame_log needs end_to_end=True and an attached encoder")
        if sensor.frame_rows().data_ptr() != self.storage.frame_row.data_ptr():
            raise ValueError("VisionPPO: the sensor's frame log must write the storage's frame_row (attach_frames_log(..., row_of=storage.frame_row))")
        self.frame_log = sensor

    def drive_frame_log(self, step):
        """the start of a rollout logs every env's present image as row 0; then the capture behind this step's env step belongs to row
        step + 1, and after the rollout's last step the stage is idle"""
        if self.frame_log is None:
            return
        if step == 0:
            self.frame_log.begin_rollout()
        self.frame_log.set_frames_log_step(step + 1)

    def _sample_stream(self):
        if self.frame_log is None:
            if self.end_to_end:
                raise RuntimeError("VisionPPO: end_to_end=True but no frame log (attach_frame_log(sensor))")
            yield from super()._sample_stream()
            return
        state = self.frame_log.frames_log_state()[:2].tolist()       # the feature's one read-back per update: the rows in use, the images that found no room
        self._e2e_rows, self.last_e2e_overflow = int(state[0]), int(state[1])
        if self.last_e2e_overflow:
            self.frame_log.frames_log_state()[1].zero_()
        try:
            for k, item in enumerate(super()._sample_stream()):
                self._e2e_minibatch = k % self.num_mini_batches if k < self.e2e_epochs * self.num_mini_batches and self._e2e_rows > 0 else None
                yield item
        finally:
            self._e2e_minibatch = None

    def live_latent(self):
        """the latent of every logged image under the present weights, with autograd to the encoder: [R, L]"""
        cam, enc, R = self.frame_log, self.encoder, self._e2e_rows
        log = cam.frames_log()[:R]
        if next(enc.parameters()).is_cuda:
            return enc.forward_device_rows(log)
        frames = log[:, :, :enc.height * enc.width].unflatten(2, (enc.height, enc.width))
        return enc(frames.to(next(enc.parameters()).dtype))

    def joined_rows(self, stored, frame_row, minibatch):
        """the rows the actor reads for minibatch `minibatch` of the latest permutation in an end-to-end epoch (_LatentJoinFn): the live
        latent of the logged images where the transition has a frame row, the stored row elsewhere and in a memory's h columns"""
        st, cam = self.storage, self.frame_log
        B = stored.shape[0]
        picked = st.last_perm[minibatch * B:(minibatch + 1) * B]
        mb_of = torch.full((st.num_transitions_per_env * st.num_envs,), -1, dtype=torch.int32, device=stored.device)
        mb_of[picked] = torch.arange(B, dtype=torch.int32, device=stored.device)
        return _LatentJoinFn.apply(self.live_latent(), stored, frame_row, mb_of, st.frame_row, cam.frames_log_sources())

    def _mb_forward(self, ac, batch, two_streams):
        if self._e2e_minibatch is None:
            return super()._mb_forward(ac, batch[:11], two_streams)
        for p in self.encoder.parameters():                     # whatever the encoder's own step left behind is not this minibatch's
            p.grad = None
        rows = self.joined_rows(batch[10], batch[11], self._e2e_minibatch)
        with ac.bound_latent(rows, live=True):
            return HIMPPO._mb_forward(self, ac, batch[:10], two_streams)

    def _after_step(self, ac, mb):
        """behind the minibatch's PPO step of an end-to-end epoch: the encoder's own clipped Adam step on the gradient the PPO backward
        left, then no gradient -- encoder_step() and memory_step() find the encoder as they always did"""
        super()._after_step(ac, mb)
        if self._e2e_minibatch is None:
            return
        params = [p for p in self.encoder.parameters() if p.grad is not None]
        if params:
            nn.utils.clip_grad_norm_(params, self.max_grad_norm)
            self.e2e_optimizer.step()
        for p in self.encoder.parameters():
            p.grad = None

    # ---- the encoder's own training data: a few (frames, target) pairs per rollout
    def snapshot_steps(self):
        T = self.storage.num_transitions_per_env
        k = max(0, min(self.aux_snapshots, T))
        return sorted({(2 * i + 1) * T // (2 * k) for i in range(k)})

    def snapshot_if_due(self, step, critic_obs):
        """called once per rollout step, before the env steps: on the steps of snapshot_steps() copy the frames and the height scan"""
        steps = self.snapshot_steps()
        if step not in steps:
            return
        if self.frames_source is None:
            raise RuntimeError("VisionPPO: no frames source (attach(encoder, latent_source, frames_source))")
        frames = self.frames_source()
        off, width = self.height_scan
        if critic_obs.shape[1] < off + width:
            raise ValueError(f"VisionPPO: the critic observation has {critic_obs.shape[1]} columns, the height scan is [{off}, {off + width})")
        if len(self._snap) != len(steps) or self._snap[0][0].shape != frames.shape or self._snap[0][0].device != frames.device:
            with torch.inference_mode(False):      # the rollout runs under inference_mode; these are inputs of a backward pass later
                self._snap = [(torch.zeros(tuple(frames.shape), device=frames.device), torch.zeros(frames.shape[0], width, device=frames.device))
                              for _ in steps]
            self._snap_filled = [False] * len(steps)
        slot = steps.index(step)
        self._snap[slot][0].copy_(frames)
        self._snap[slot][1].copy_(critic_obs[:, off:off + width])
        self._snap_filled[slot] = True

    def encoder_step(self):
        """one pass over this rollout's snapshots -> mean loss (a 0-d tensor), or None without a snapshot"""
        if self.encoder is None:
            raise RuntimeError("VisionPPO: no encoder (attach(encoder, latent_source, frames_source))")
        on_device = next(self.encoder.parameters()).is_cuda
        total, n = None, 0
        for (frames, target), filled in zip(self._snap, self._snap_filled):
            if not filled:
                continue
            z = self.encoder.forward_device(frames) if on_device else self.encoder(frames)
            loss = F.mse_loss(self.depth_head(z), target)
            self.aux_optimizer.zero_grad()
            loss.backward()
            self.aux_optimizer.step()
            total = loss.detach() if total is None else total + loss.detach()
            n += 1
        self._snap_filled = [False] * len(self._snap)
        return None if n == 0 else total / n

    def memory_data(self):
        """the BPTT data set a finished rollout IS, from the storage alone: steps 1 .. T-1 with x_t = [z_t | obs_t[:P]] (what the launch
        behind env step t-1 read), reset_t = dones[t-1] (the env was fresh then), h0 = the h columns of step 0's stored row, and the height
        scan of privileged_observations[t] as the target -> (x [T-1, N, I], h0 [N, H], reset [T-1, N] uint8, target [T-1, N, scan])"""
        mem, st = self.memory, self.storage
        L, P = mem.latent_dim, mem.proprio_dim
        off, width = self.height_scan
        rows = st.depth_latent
        x = torch.cat((rows[1:, :, :L], st.observations[1:, :, :P]), dim=-1)
        return x, rows[0][:, L:], st.dones[:-1, :, 0], st.privileged_observations[1:, :, off:off + width]

    def memory_step(self):
        """one pass over this rollout for the memory: memory_env_minibatches contiguous env slices, each ONE sequence pass over all T - 1
        steps (DepthMemory.sequence_device on the device), loss = mse(memory_head(hs), height scan), one Adam step over memory and head.
        The stored h0 (and, for later slices, every stored row) was produced by the weights of the rollout, not by the ones an earlier
        slice has just updated: the usual truncated-BPTT approximation.  No gradient reaches the encoder (the stored z is data) or the
        actor-critic.  -> mean loss (a 0-d tensor), or None for a rollout of fewer than 2 steps"""
        if self.memory is None:
            raise RuntimeError("VisionPPO: no memory (attach(..., memory=DepthMemory(...)))")
        if self.storage.num_transitions_per_env < 2:
            return None
        x, h0, reset, target = self.memory_data()
        N = x.shape[1]
        k = max(1, min(self.memory_env_minibatches, N))
        on_device = next(self.memory.parameters()).is_cuda or self.memory_api is not None
        total = None
        for i in range(k):
            a, b = i * N // k, (i + 1) * N // k
            xs, hs0, rs = x[:, a:b].contiguous(), h0[a:b].contiguous(), reset[:, a:b].contiguous()
            hs = self.memory.sequence_device(xs, hs0, rs, api=self.memory_api) if on_device else self.memory.sequence(xs, hs0, rs)
            loss = F.mse_loss(self.memory_head(hs), target[:, a:b])
            self.memory_optimizer.zero_grad()
            loss.backward()
            self.memory_optimizer.step()
            total = loss.detach() if total is None else total + loss.detach()
        return total / k

    def update(self):
        out = super().update()
        aux = self.encoder_step()
        self.last_aux_loss = float("nan") if aux is None else float(aux)
        if self.memory is None:
            return tuple(out) + (self.last_aux_loss,)
        loss = self.memory_step()
        self.last_memory_loss = float("nan") if loss is None else float(loss)
        return tuple(out) + (self.last_aux_loss, self.last_memory_loss)


class PackedVisionPolicy(PackedHimPolicy):
    """PackedHimPolicy (which packs whatever actor[0] is) launched through the entry points with the extra actor-input segment"""

    @staticmethod
    def supported(ac):
        wide_enough = (ac.actor[0].in_features + 15) // 16 * 16 <= 272
        return isinstance(ac, VisionActorCritic) and wide_enough and PackedHimPolicy.supported(ac)

    def _extra(self, rows, store=None):
        L = self.ac.depth_latent_dim
        if not (rows.is_cuda and rows.dtype == torch.float32 and rows.dim() == 2 and rows.shape[1] == L and rows.stride(1) == 1):
            raise ValueError(f"PackedVisionPolicy: the latent rows must be fp32 [N, {L}] on the device with unit column stride")
        x = abi.LsimPolicyExtra()
        x.rows, x.dim, x.ld = rows.data_ptr(), L, rows.stride(0)
        if store is not None:
            if not (store.is_cuda and store.dtype == torch.float32 and store.is_contiguous() and store.dim() == 3 and store.shape[2] == L):
                raise ValueError(f"PackedVisionPolicy: the latent store must be a contiguous fp32 [T, N, {L}] device tensor")
            x.store = store.data_ptr()
        return x

    def forward(self, obs, priv_obs, mean_out, values_out, rows=None):
        if rows is None:
            raise ValueError("PackedVisionPolicy.forward: no depth latent rows")
        if rows.shape[0] != obs.shape[0]:
            raise ValueError("PackedVisionPolicy.forward: one latent row per env")
        x = self._extra(rows)
        lib.check(self._L.lsim_policy_forward_ext(ctypes.byref(self._P), ctypes.byref(x), obs.data_ptr(), priv_obs.data_ptr(), obs.shape[0], mean_out.data_ptr(),
                                                  values_out.data_ptr(), torch.cuda.current_stream(self.dev).cuda_stream), what="lsim_policy_forward_ext")

    def forward_act(self, storage_struct, step, draw, obs, priv_obs, std, seed, rank, mean_out, values_out, actions_out, prev=None, rows=None, store=None):
        """lsim_policy_act_post_at_ext; prev as PackedHimPolicy.forward_act's (None: no post-step store), `store` [T, N, L] or None"""
        if rows is None:
            raise ValueError("PackedVisionPolicy.forward_act: no depth latent rows")
        if rows.shape[0] != storage_struct.num_envs or (store is not None and (store.shape[0] != storage_struct.num_steps or store.shape[1] != storage_struct.num_envs)):
            raise ValueError("PackedVisionPolicy.forward_act: the latent rows / store do not match the storage's [T, N]")
        x = self._extra(rows, store)
        pstep, dones, touts, rewards, term, gamma = prev if prev is not None else (-1, None, None, None, None, 0.0)
        ptr = lambda t: t.data_ptr() if t is not None else None
        lib.check(self._L.lsim_policy_act_post_at_ext(ctypes.byref(self._P), ctypes.byref(x), ctypes.byref(storage_struct), int(step), int(draw), obs.data_ptr(),
                                                      priv_obs.data_ptr(), std.data_ptr(), seed, rank, mean_out.data_ptr(), values_out.data_ptr(),
                                                      actions_out.data_ptr(), int(pstep), ptr(dones), ptr(touts), ptr(rewards), ptr(term), float(gamma),
                                                      torch.cuda.current_stream(self.dev).cuda_stream), what="lsim_policy_act_post_at_ext")


class VisionRollout(GraphedRollout):
    """GraphedRollout whose policy launch also reads the sensor's live latent rows and stores them in storage.depth_latent[step]; the
    previous step's deferred post-step store rides along as in the parent.  Only the fused launch: no captured-graph form."""

    def __init__(self, runner, sensor):
        self.sensor = sensor
        super().__init__(runner)

    def _make_packed(self):
        ac = self.alg.actor_critic
        if not PackedVisionPolicy.supported(ac):
            raise lib.LsimError("VisionRollout: the fused policy launch does not take this topology (use the eager rollout)")
        return PackedVisionPolicy(ac)

    def _act(self):
        env, ac = self.env, self.alg.actor_critic
        self.alg.drive_frame_log(self.storage.step)
        self.alg.snapshot_if_due(self.storage.step, env.privileged_obs_buf)
        prev, self._pending_post = self._pending_post, None
        self.packed.forward_act(self._S, self.storage.step, self._draw_host, env.obs_buf, env.privileged_obs_buf, ac.std, self._seed, self._rank,
                                self.mean, self.values, self.actions, prev=prev, rows=self.alg._latent_now(), store=self.storage.depth_latent)


class ActorRowsRunner(HIMOnPolicyRunner):
    """what the runners of a policy whose actor reads a sensor's rows (`self.sensor`) share: the train_cfg, the fused policy launch's width
    limit and rollout, and the checkpoint's parts (learn/policy_io.py).  A subclass sets `policy_kind` and has policy_record()."""

    def _rows_cfg(self, train_cfg, learner, depth_latent_dim):
        """a copy of `train_cfg` for a VisionActorCritic that reads `depth_latent_dim` more columns, trained by `learner`, both registered"""
        _POLICIES["VisionActorCritic"], _ALGOS[learner.__name__] = VisionActorCritic, learner
        cfg = {k: copy.copy(v) for k, v in train_cfg.items()}
        cfg["runner"]["policy_class_name"], cfg["runner"]["algorithm_class_name"] = "VisionActorCritic", learner.__name__
        cfg["policy"]["depth_latent_dim"] = int(depth_latent_dim)
        return cfg

    def _extra_checkpoint_state(self):
        return {**super()._extra_checkpoint_state(), **policy_io.checkpoint_state(self.alg, self.policy_kind, self.policy_record())}

    def _load_extra_checkpoint_state(self, d):
        super()._load_extra_checkpoint_state(d)
        policy_io.load_checkpoint_state(self.alg, d)

    def _check_first_layer(self, env, **widths):
        first = env.num_one_step_obs + 3 + 16 + sum(widths.values())
        if first > 272:         # LS_POL_MAX_IN (csrc/ls_policy.h): the fused policy launch's widest input row
            raise ValueError(f"{type(self).__name__}: the first actor layer would read {first} columns ({env.num_one_step_obs} + 3 + 16 + "
                             f"{' + '.join(f'{k} {v}' for k, v in widths.items())}), the fused policy launch takes at most 272")

    def _make_fused_rollout(self):
        return VisionRollout(self, self.sensor) if PackedVisionPolicy.supported(self.alg.actor_critic) else None


class VisionOnPolicyRunner(ActorRowsRunner):
    """HIMOnPolicyRunner for a vision policy.  `sensor`: the name of a sensor already added to the env (env.add_sensor), or the sensor; it needs a
    SensorModel (the frame history).  `encoder`: a DepthEncoder for its frames; default DepthEncoder(height, width, frames).  The runner
    attaches the encoder to the sensor.  train_cfg is HIMOnPolicyRunner's; policy["depth_latent_dim"] is set from the encoder and
    algorithm["aux_snapshots"] / ["aux_learning_rate"] are optional.  `memory`: True builds DepthMemory(L, env.num_one_step_obs, 64), an
    instance is taken as is; the actor then reads [z | h] (policy["depth_latent_dim"] = L + H, the stored row likewise) and VisionPPO trains
    the cell behind the encoder's step (algorithm["memory_env_minibatches"] / ["memory_learning_rate"] are optional).  Without it nothing
    is allocated, launched, stored or saved that was not before.  `end_to_end=True`: the PPO gradient reaches the encoder (module
    docstring, decision 1) -- the sensor gets a frame log over the storage's frame_row (algorithm["e2e_capacity"] rows, default the
    stage's), the first algorithm["e2e_epochs"] (default 1) learning epochs carry the gradient and the encoder steps with
    algorithm["e2e_learning_rate"] (default aux_learning_rate); one rank, and no gradient through the memory.  Without it, likewise,
    nothing is allocated, launched, stored or saved that was not before."""

    policy_kind = "vision"
    algorithm_class = None      # the learner: VisionPPO; learn/distill.py's DistillRunner names VisionDistill

    def __init__(self, env, train_cfg, sensor="depth", encoder=None, log_dir=None, device="cpu", fast=None, memory=None, end_to_end=False):
        cam = env.sensors[sensor] if isinstance(sensor, str) else sensor
        if getattr(cam, "model", None) is None:
            raise ValueError("VisionOnPolicyRunner: the sensor has no SensorModel, so no frame history to encode")
        scan = height_scan_block(env.cfg)
        if encoder is None:
            if not (hasattr(cam, "height") and hasattr(cam, "width")):
                raise ValueError("VisionOnPolicyRunner: the sensor is no camera (no height / width): pass an encoder for its frames")
            from .depth_encoder import DepthEncoder
            encoder = DepthEncoder(cam.height, cam.width, cam.model.frames)
        encoder = encoder.to(device)
        if memory is not None and memory is not False:
            from .depth_memory import DepthMemory
            memory = DepthMemory(encoder.latent_dim, env.num_one_step_obs, 64) if memory is True else memory
            if memory.latent_dim != encoder.latent_dim or memory.proprio_dim > env.num_one_step_obs:
                raise ValueError(f"VisionOnPolicyRunner: the memory reads {memory.latent_dim} latent and {memory.proprio_dim} observation columns, "
                                 f"the encoder writes {encoder.latent_dim} and a one-step observation has {env.num_one_step_obs}")
            memory = memory.to(device)
            self._check_first_layer(env, latent=encoder.latent_dim, hidden=memory.hidden)
        else:
            memory = None
        cfg = self._rows_cfg(train_cfg, self.algorithm_class or VisionPPO, encoder.latent_dim + (memory.hidden if memory is not None else 0))
        if end_to_end:
            if getattr(cam, "env_stride", 1) != 1:
                raise ValueError("VisionOnPolicyRunner: end_to_end needs a sensor that renders every env (env_stride == 1)")
            cfg["algorithm"]["end_to_end"] = True
        self.sensor, self.memory = cam, memory
        super().__init__(env, cfg, log_dir=log_dir, device=device, fast=fast)
        cam.attach_encoder(encoder)         # behind the parent's env.reset(): the sensor has captured, so every env is encoded now
        frames = cam.frame_images if hasattr(cam, "frame_images") else (lambda: cam.frames().unflatten(2, (encoder.height, encoder.width)))
        if memory is None:
            self.alg.attach(encoder, cam.latent, frames, scan)
        else:
            cam.attach_memory(memory)       # every env steps once from h = 0
            self.alg.attach(encoder, cam.memory_rows, frames, scan, memory=memory)
        if end_to_end:
            cam.attach_frames_log(self.num_steps_per_env, capacity=self.alg.e2e_capacity, row_of=self.alg.storage.frame_row)
            self.alg.attach_frame_log(cam)

    def policy_record(self):
        """what the policy was trained with: learn/policy_io.py rebuilds encoder and memory from it, learn/evaluate.py the camera"""
        alg, cam = self.alg, getattr(self, "sensor", None)
        record = {"encoder": alg.encoder.config(), "sensor": cam.spec() if hasattr(cam, "spec") else None,
                  "latent_dim": int(alg.actor_critic.depth_latent_dim)}
        if alg.memory is not None:
            record["memory"] = alg.memory.config()
        if alg.end_to_end:
            record["end_to_end"] = {"epochs": alg.e2e_epochs, "learning_rate": alg.e2e_learning_rate, "capacity": int(self.sensor.frames_log().shape[0])}
        return record

    def export(self, path):
        """learn/export.py: export_policy_as_jit of this runner's actor-critic, encoder and sensor; `path` is a directory"""
        from .export import export_policy_as_jit
        self.get_inference_policy()
        return export_policy_as_jit(self.alg.actor_critic, path, encoder=self.alg.encoder, sensor=self.sensor, memory=self.alg.memory)
