"""Vision distillation: a camera student regressed onto a scan-reading teacher's action means, on the states the STUDENT visits
(DAgger).

    teacher = ScanOnPolicyRunner(env, train_cfg, device=dev)          # learn/scan_policy.py: the actor reads the true height scan
    teacher.learn(n); teacher.save("teacher.pt")
    cam = env.add_sensor("depth", depth_camera(env, 64, 48, 87.0, model=SensorModel(period=5, stagger=True, latency=1, frames=2, normalise=True)))
    runner = DistillRunner(env, train_cfg, teacher="teacher.pt", sensor="depth", device=dev)
    runner.enable_graphs()
    runner.learn(m); runner.save("student.pt")                        # an ordinary vision checkpoint: VisionOnPolicyRunner.load, evaluate, export

The rollout is VisionOnPolicyRunner's own with end_to_end=True: the student acts (sampled with the teacher's frozen std), the sensor logs
every image once, the storage keeps observation, privileged observation -- which contains the scan -- and the frame row of every
transition.  The update then
  1. labels the rollout: the teacher's action means of all T * N stored transitions, ONE lsim_policy_forward_ext with the packed teacher
     (rows = the scan block of storage.privileged_observations, ld = num_priv_obs) into a persistent buffer; torch's act_inference elsewhere;
  2. for distill_epochs x num_mini_batches minibatches of the storage's generator, every one an end-to-end minibatch: the student's means
     under the live latent of the logged images, the mean squared error against the labels through lsim_distill_loss -- which finds a
     minibatch row's label through the shuffle's permutation, so the labels are never gathered --, backward, a clipped Adam step over the
     ACTOR's parameters and the encoder's own clipped step, as VisionPPO._after_step takes it;
  3. the parent's encoder_step() on the height-scan snapshots.
Estimator, critic and std are the teacher's and are never stepped.  Nothing here runs unless these classes are used.  Open: a student
with a depth memory, a teacher-action mixing schedule, a KL loss or a learned std, more than one rank."""
import ctypes

import torch
import torch.nn as nn

from .. import abi, lib
from . import fused_linear as FL
from . import policy_io
from .scan_policy import ScanOnPolicyRunner
from .vision import PackedVisionPolicy, VisionOnPolicyRunner, VisionPPO, height_scan_block


class _DistillLossFn(torch.autograd.Function):
    """loss = mean over the rows that carry one of (mu[i][j] - target[index[i]][j])^2 ... precisely 0.5 * scale * sum d^2 with scale =
    2 / (B * A) formed in mu's precision, d = 0 for a row whose index lies outside 0 .. rows - 1; d loss / d mu = d * scale.  On fp32
    device tensors forward and backward are ONE lsim_distill_loss launch (include/lsim.h) plus the sum of its 256 partial results;
    elsewhere the same statements in torch."""

    @staticmethod
    def forward(ctx, mu, target, index):
        B, A = mu.shape
        scale = float(torch.tensor(2.0, dtype=mu.dtype) / (B * A))
        if mu.is_cuda and mu.dtype == torch.float32:
            if mu.stride(1) != 1:
                mu = mu.contiguous()
            if not (target.is_cuda and target.dtype == torch.float32 and target.dim() == 2 and target.stride(1) == 1 and target.shape[1] >= A):
                raise ValueError(f"distillation loss: the labels must be fp32 [rows, >= {A}] on the device with unit column stride")
            if not (index.is_cuda and index.dtype == torch.int32 and index.is_contiguous() and index.numel() == B):
                raise ValueError(f"distillation loss: the index must be a contiguous int32 [{B}] device tensor")
            g = torch.empty(B, A, device=mu.device, dtype=torch.float32)
            partial = torch.empty(abi.DEFINES["LSIM_DISTILL_PARTIALS"], device=mu.device, dtype=torch.float32)
            dl = abi.LsimDistillLoss()
            dl.mu, dl.target, dl.index, dl.g, dl.partial = mu.data_ptr(), target.data_ptr(), index.data_ptr(), g.data_ptr(), partial.data_ptr()
            dl.batch, dl.actions, dl.target_rows = B, A, target.shape[0]
            dl.mu_stride, dl.target_stride, dl.g_stride, dl.scale = mu.stride(0), target.stride(0), g.stride(0), scale
            entry = lib.entry(lib.load(), "lsim_distill_loss", "the distillation update")
            lib.check(entry(ctypes.byref(dl), torch.cuda.current_stream(mu.device).cuda_stream), what="lsim_distill_loss")
            loss = partial.sum() * (0.5 * scale)
        else:
            ok = ((index >= 0) & (index < target.shape[0])).unsqueeze(1)
            picked = target.index_select(0, index.clamp(0, target.shape[0] - 1).long())[:, :A].to(mu.dtype)
            d = torch.where(ok, mu - picked, torch.zeros((), dtype=mu.dtype, device=mu.device))
            g = d * scale
            loss = (d * d).sum() * (0.5 * scale)
        ctx.save_for_backward(g)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        g, = ctx.saved_tensors
        return g * grad_loss, None, None


def distill_loss(mu, target, index):
    """the distillation loss of a minibatch: `mu` [B, A] the student's means, `target` [rows, A] the teacher's means of every stored
    transition, `index` [B] int32 the transition each minibatch row holds"""
    return _DistillLossFn.apply(mu, target, index)


class VisionDistill(VisionPPO):
    """VisionPPO with end_to_end=True whose update() is the regression above instead of PPO.  `attach_teacher(teacher, scan)` hands it
    the frozen teacher (a VisionActorCritic whose depth rows are the scan block `scan` = (offset, width) of a privileged observation).
    update() returns (mean distillation loss, last_aux_loss); one read-back per update beyond the frame log's own, for the loss."""

    def __init__(self, actor_critic, distill_epochs=1, distill_learning_rate=1e-3, **kwargs):
        kwargs["end_to_end"] = True
        super().__init__(actor_critic, **kwargs)
        self.distill_epochs, self.distill_learning_rate = int(distill_epochs), float(distill_learning_rate)
        if self.distill_epochs < 1:
            raise ValueError("VisionDistill: distill_epochs >= 1")
        self.distill_optimizer = torch.optim.Adam(self.actor_critic.actor.parameters(), lr=self.distill_learning_rate)
        self.teacher = self.teacher_scan = self.teacher_means = None
        self._teacher_packed = self._teacher_values = None
        self.last_distill_loss = float("nan")

    def attach_teacher(self, teacher, scan):
        off, width = (int(v) for v in scan)
        if teacher.depth_latent_dim != width:
            raise ValueError(f"VisionDistill: the teacher's actor reads {teacher.depth_latent_dim} more columns, the scan block has {width}")
        self.teacher = teacher.to(self.device).eval()
        for p in self.teacher.parameters():
            p.requires_grad_(False)
        self.teacher_scan = (off, width)
        self.teacher_means = self._teacher_packed = self._teacher_values = None

    @torch.no_grad()
    def label_rollout(self):
        """the labelling pass: the teacher's action means of every stored transition -> teacher_means [T * N, A], a persistent buffer.
        On the device one lsim_policy_forward_ext with the packed teacher (packed once: it never changes), whose critic half is wasted
        work; a topology that launch does not take, and the CPU, run teacher.act_inference(obs, depth_latent=scan)."""
        if self.teacher is None:
            raise RuntimeError("VisionDistill: no teacher (attach_teacher(teacher, scan))")
        st, (off, width) = self.storage, self.teacher_scan
        obs, priv = st.observations.flatten(0, 1), st.privileged_observations.flatten(0, 1)
        if priv.shape[1] < off + width:
            raise ValueError(f"VisionDistill: the stored privileged observation has {priv.shape[1]} columns, the height scan is [{off}, {off + width})")
        dtype = next(self.teacher.parameters()).dtype
        if self.teacher_means is None or self.teacher_means.shape[0] != obs.shape[0]:
            self.teacher_means = torch.zeros(obs.shape[0], self.teacher.num_actions, device=obs.device, dtype=dtype)
        scan = priv[:, off:off + width]
        if obs.is_cuda and dtype == torch.float32 and PackedVisionPolicy.supported(self.teacher):
            if self._teacher_packed is None:
                self._teacher_packed = PackedVisionPolicy(self.teacher)
                self._teacher_values = torch.empty(obs.shape[0], 1, device=obs.device)
            self._teacher_packed.forward(obs, priv, self.teacher_means, self._teacher_values, rows=scan)
        else:
            self.teacher_means.copy_(self.teacher.act_inference(obs.to(dtype), depth_latent=scan.to(dtype)))
        return self.teacher_means

    def _student_means(self, ac, batch, minibatch):
        """the student's action means of one minibatch under the live latent of the logged images (joined_rows), with autograd to the
        actor and the encoder"""
        dtype = next(ac.actor.parameters()).dtype
        rows = self.joined_rows(batch[10], batch[11], minibatch) if self._e2e_rows > 0 else batch[10].to(dtype)
        with ac.bound_latent(rows, live=True):
            return ac.actor(ac._actor_input(batch[0].to(dtype)))

    def minibatch_loss(self, ac, batch, minibatch):
        """the distillation loss of minibatch `minibatch` of the latest permutation (label_rollout() first)"""
        mu = self._student_means(ac, batch, minibatch)
        B = mu.shape[0]
        index = self.storage.last_perm[minibatch * B:(minibatch + 1) * B].to(torch.int32)
        return distill_loss(mu, self.teacher_means, index)

    def update(self):
        if self.frame_log is None:
            raise RuntimeError("VisionDistill: no frame log (attach_frame_log(sensor))")
        ac, st = self.actor_critic, self.storage
        FL.set_grad_arena(None)         # this learner's gradients are plain tensors (a PPO learner of the same process sets its own arena again)
        self.label_rollout()
        state = self.frame_log.frames_log_state()[:2].tolist()       # the frame log's read-back: the rows in use, the images that found no room
        self._e2e_rows, self.last_e2e_overflow = int(state[0]), int(state[1])
        if self.last_e2e_overflow:
            self.frame_log.frames_log_state()[1].zero_()
        actor_params = list(ac.actor.parameters())
        total = torch.zeros((), device=self.device)
        n = 0
        for k, batch in enumerate(st.mini_batch_generator(self.num_mini_batches, self.distill_epochs)):
            for p in self.encoder.parameters():
                p.grad = None
            loss = self.minibatch_loss(ac, batch, k % self.num_mini_batches)
            self.distill_optimizer.zero_grad()
            loss.backward()
            nn.utils.clip_grad_norm_(actor_params, self.max_grad_norm)
            self.distill_optimizer.step()
            params = [p for p in self.encoder.parameters() if p.grad is not None]       # the encoder's own clipped step, as _after_step takes it
            if params:
                nn.utils.clip_grad_norm_(params, self.max_grad_norm)
                self.e2e_optimizer.step()
            for p in self.encoder.parameters():
                p.grad = None
            total = total + loss.detach().to(total.dtype)
            n += 1
        for p in ac.parameters():       # estimator, critic and std took no step; nothing is left for a later learner to find
            p.grad = None
        aux = self.encoder_step()
        self.last_aux_loss = float("nan") if aux is None else float(aux)
        self.last_distill_loss = float(total / max(n, 1))            # the update's one read-back
        st.clear()
        return self.last_distill_loss, self.last_aux_loss


def _teacher_checkpoint(teacher, device):
    """(model state dict, the scan policy's record) of `teacher`: a checkpoint path, a loaded checkpoint dict, or a ScanOnPolicyRunner.
    The module itself is built behind DistillRunner's own checks of the widths against the env."""
    if isinstance(teacher, ScanOnPolicyRunner):
        parts = policy_io.policy_parts(None, teacher)
        return {k: v.detach().clone() for k, v in parts.actor_critic.state_dict().items()}, parts.scan
    if isinstance(teacher, str):
        teacher = torch.load(teacher, map_location=device, weights_only=False)
    if not isinstance(teacher, dict) or "model_state_dict" not in teacher:
        raise TypeError("DistillRunner: teacher is a checkpoint path, a loaded checkpoint dict or a ScanOnPolicyRunner")
    kind, record = policy_io.policy_record(teacher)
    if kind != "scan":
        raise ValueError("DistillRunner: the teacher's checkpoint has no 'scan_policy' record (it is no ScanOnPolicyRunner's)")
    return teacher["model_state_dict"], dict(record)


class DistillRunner(VisionOnPolicyRunner):
    """VisionOnPolicyRunner(end_to_end=True) whose learner is VisionDistill.  `teacher`: a ScanOnPolicyRunner's checkpoint (path or loaded
    dict) or the runner itself; its widths are checked against the env, the student is warm-started from it
    (VisionActorCritic.load_scan_teacher_state_dict: everything copied, the scan columns dropped, the depth columns zero) and
    algorithm["distill_epochs"] / ["distill_learning_rate"] are optional.  learn() is the parent's loop (compute_returns still runs,
    harmlessly); the checkpoint is the parent's plus a "distill" record, so VisionOnPolicyRunner.load, evaluate and the exporter take it
    as it is and PPO fine-tuning continues from it.  One rank; `memory=` is refused (open: a student with memory)."""

    algorithm_class = VisionDistill

    def __init__(self, env, train_cfg, teacher=None, sensor="depth", encoder=None, log_dir=None, device="cpu", fast=None, memory=None):
        if memory is not None and memory is not False:
            raise NotImplementedError("DistillRunner: a student with a depth memory is not supported (no gradient goes through the memory)")
        if teacher is None:
            raise ValueError("DistillRunner: teacher= (a ScanOnPolicyRunner, its checkpoint's path or the loaded checkpoint)")
        sd, record = _teacher_checkpoint(teacher, device)
        if record.get("foot_scan") is not None:
            raise NotImplementedError("DistillRunner: the teacher reads true foot scans (ScanOnPolicyRunner(foot_scan=...)); distillation from a "
                                      "foot-scan teacher is not built (the student's warm start and the labels assume the height-scan block)")
        off, width = height_scan_block(env.cfg)
        if (int(record["offset"]), int(record["width"])) != (off, width) or int(record["dim"]) != width:
            raise ValueError(f"DistillRunner: the teacher read the scan block {record}, the env's is offset {off}, width {width}")
        num_critic_obs = env.num_privileged_obs if env.num_privileged_obs is not None else env.num_obs
        actor = policy_io.layer_widths(sd)[0]
        want = {"estimator.encoder.0.weight": env.num_obs, "critic.0.weight": num_critic_obs, "actor.0.weight": env.num_one_step_obs + 3 + 16 + width}
        for key, cols in want.items():
            if sd[key].shape[1] != cols:
                raise ValueError(f"DistillRunner: the teacher's {key} reads {sd[key].shape[1]} columns, the env gives {cols}")
        if actor[-1] != env.num_actions:
            raise ValueError(f"DistillRunner: the teacher has {actor[-1]} actions, the env {env.num_actions}")
        teacher_ac = policy_io.actor_critic_from_state_dict(env, sd, rows=True, activation=train_cfg["policy"].get("activation", "elu"))
        super().__init__(env, train_cfg, sensor=sensor, encoder=encoder, log_dir=log_dir, device=device, fast=fast, memory=None, end_to_end=True)
        dtype = next(self.alg.actor_critic.parameters()).dtype
        self.alg.actor_critic.load_scan_teacher_state_dict(sd, width)
        self.alg.attach_teacher(teacher_ac.to(dtype), (off, width))
        self.teacher_record = {"offset": off, "width": width, "dim": width}

    def _extra_checkpoint_state(self):
        alg = self.alg
        return {**super()._extra_checkpoint_state(), "distill": {"teacher": dict(self.teacher_record), "epochs": alg.distill_epochs,
                "learning_rate": alg.distill_learning_rate, "distill_optimizer_state_dict": alg.distill_optimizer.state_dict()}}

    def _load_extra_checkpoint_state(self, d):
        super()._load_extra_checkpoint_state(d)
        state = (d.get("distill") or {}).get("distill_optimizer_state_dict")
        if state is not None:
            self.alg.distill_optimizer.load_state_dict(state)
