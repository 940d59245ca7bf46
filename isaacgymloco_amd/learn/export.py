"""Deployment export of a trained policy: the counterpart of legged_gym.utils.helpers.export_policy_as_jit / PolicyExporterHIM
(HLP:201-212, HLP:248-264), which play.py calls (PLAY:71-74) to write `<log_dir>/exported/policies/policy.pt`.

The exported TorchScript module maps an observation history [B, 270] to action means [B, 12]:
    encoder(obs)[:, :19] -> (velocity[3], L2-normalised latent[16]);  actor(cat(obs[:, :45], velocity, latent)).
A vision policy (learn/vision.py) exports as PolicyExporterVision: the same two networks with the wider first actor layer, plain copies of
the depth encoder's three layers and the sensor model's clip / normalisation constants, so that the robot's program needs nothing but the file:
    preprocess(depth in metres) -> frames;  encode(frames) -> latent, at camera rate;  act(obs_history, latent) -> action means, at control rate.
The exported module takes frames and knows no mount: a sensor's per-episode mount jitter (envs/sensors.py MountJitter, a record's
"mount_jitter") is a property of the simulated instrument that trained the policy, and leaves the exported file what it was.
The build's networks are `HimMLP` / `SkinnyLinear` modules (nn.Sequential / nn.Linear subclasses whose forward dispatches to the HIP
weight-gradient kernels under autograd), which TorchScript cannot script; the exporter therefore re-materialises the two networks as plain
`nn.Sequential(nn.Linear, nn.ELU, ...)` with the SAME weights -- exactly the module tree the reference scripts, so a file written here loads
wherever the reference's file does (torch.jit.load, C++ libtorch on the robot) and gives the same outputs.
"""
import copy
import os
from typing import Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F


def plain_sequential(seq):
    """nn.Sequential of plain nn.Linear / activation modules with copies of `seq`'s parameters (state_dict keys unchanged)."""
    layers = []
    for m in seq:
        if isinstance(m, nn.Linear):
            lin = nn.Linear(m.in_features, m.out_features, bias=m.bias is not None)
            with torch.no_grad():
                lin.weight.copy_(m.weight.detach().cpu())
                if m.bias is not None:
                    lin.bias.copy_(m.bias.detach().cpu())
            layers.append(lin)
        else:
            layers.append(copy.deepcopy(m).cpu())
    return nn.Sequential(*layers)


class PolicyExporterHIM(nn.Module):
    """HLP:248-264: actor + estimator encoder, forward(obs_history) -> action means."""

    def __init__(self, actor_critic):
        super().__init__()
        self.actor = plain_sequential(actor_critic.actor)
        self.estimator = plain_sequential(actor_critic.estimator.encoder)
        self.num_one_step_obs = int(actor_critic.num_one_step_obs)
        self.num_enc_out = int(actor_critic.estimator.num_latent) + 3

    def forward(self, obs_history: torch.Tensor) -> torch.Tensor:
        parts = self.estimator(obs_history)[:, 0:self.num_enc_out]
        vel, z = parts[..., :3], parts[..., 3:]
        z = F.normalize(z, dim=-1, p=2.0)
        return self.actor(torch.cat((obs_history[:, 0:self.num_one_step_obs], vel, z), dim=1))

    def export(self, path):
        os.makedirs(path, exist_ok=True)
        path = os.path.join(path, "policy.pt")
        self.to("cpu")
        torch.jit.script(self).save(path)
        return path


class PolicyExporterVision(PolicyExporterHIM):
    """A VisionActorCritic with its DepthEncoder and the constants of the sensor it was trained with.  `sensor`: a RaySensor with a
    SensorModel (envs/sensors.py) or its spec() (a checkpoint's record of it, learn/policy_io.py's sensor_record).  Attributes clip_lo, clip_hi, offset, gain (lsim_sensor_capture's
    clip and normalisation), period, latency, frames (how the robot must pace and delay its captures), height, width."""

    def __init__(self, actor_critic, encoder, sensor):
        super().__init__(actor_critic)          # actor, estimator and their two widths
        from ..envs.sensors import SensorModel
        spec = sensor if isinstance(sensor, dict) else sensor.spec()
        m = spec.get("model")
        if m is None:
            raise ValueError("PolicyExporterVision: the sensor has no SensorModel, so no frame history the encoder could have read")
        model = SensorModel(**m)
        if encoder.frames != model.frames or encoder.latent_dim + self._memory_columns() != actor_critic.depth_latent_dim:
            raise ValueError(f"PolicyExporterVision: the encoder reads {encoder.frames} frames and writes {encoder.latent_dim} columns; the sensor "
                             f"keeps {model.frames}, the actor reads {actor_critic.depth_latent_dim}")
        self.conv1, self.conv2, self.fc = copy.deepcopy(encoder.conv1).cpu(), copy.deepcopy(encoder.conv2).cpu(), copy.deepcopy(encoder.fc).cpu()
        for p in self.parameters():
            p.requires_grad_(False)
        self.final_act = bool(encoder.final_act)
        (lo, hi), offset, gain = model.offset_gain(float(spec["near"]), float(spec["far"]))
        # the launch's own fp32 constants (lsim_sensor_model_t holds floats), so that preprocess is its arithmetic bit for bit
        f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
        self.clip_lo, self.clip_hi, self.offset, self.gain = f32(lo), f32(hi), f32(offset), f32(gain)
        self.period, self.latency, self.frames = model.period, model.latency, model.frames
        self.height, self.width = int(encoder.height), int(encoder.width)
        self.latent_dim = int(encoder.latent_dim)

    @torch.jit.ignore
    def _memory_columns(self):
        """columns of the actor's depth segment that are not the encoder's: none here"""
        return 0

    @torch.jit.export
    def preprocess(self, depth_m: torch.Tensor) -> torch.Tensor:
        """[B, H, W] depth in metres -> one frame as the policy was trained on it: the clip and normalise lines of lsim_sensor_capture, in
        their order, without noise and holes"""
        lo = torch.full_like(depth_m, self.clip_lo)
        hi = torch.full_like(depth_m, self.clip_hi)
        return (torch.minimum(torch.maximum(depth_m, lo), hi) - self.offset) * self.gain

    @torch.jit.export
    def encode(self, frames: torch.Tensor) -> torch.Tensor:
        """[B, frames, H, W], oldest first -> latent [B, L]"""
        x = F.elu(self.conv1(frames))
        x = F.elu(self.conv2(x))
        z = self.fc(torch.flatten(x, 1))
        if self.final_act:
            z = F.elu(z)
        return z

    @torch.jit.export
    def act(self, obs_history: torch.Tensor, latent: torch.Tensor) -> torch.Tensor:
        """PolicyExporterHIM.forward's estimator path, the depth columns last"""
        parts = self.estimator(obs_history)[:, 0:self.num_enc_out]
        vel, z = parts[..., :3], parts[..., 3:]
        z = F.normalize(z, dim=-1, p=2.0)
        return self.actor(torch.cat((obs_history[:, 0:self.num_one_step_obs], vel, z, latent), dim=1))

    def forward(self, obs_history: torch.Tensor, frames: torch.Tensor) -> torch.Tensor:
        return self.act(obs_history, self.encode(frames))


class PolicyExporterVisionMemory(PolicyExporterVision):
    """PolicyExporterVision for a policy trained with a depth memory (learn/depth_memory.py): the actor reads rows = cat(latent, h).  The
    robot keeps h between control steps, zero at the start of an episode: `remember` runs at CONTROL rate with the latest latent (held
    between captures) and the current observation history, whose first proprio_dim columns are the cell's second input.  Attribute `hidden`."""

    def __init__(self, actor_critic, encoder, sensor, memory):
        self.hidden = int(memory.hidden)
        super().__init__(actor_critic, encoder, sensor)
        if memory.latent_dim != encoder.latent_dim or memory.proprio_dim > actor_critic.num_one_step_obs:
            raise ValueError(f"PolicyExporterVisionMemory: the memory reads {memory.latent_dim} latent and {memory.proprio_dim} observation columns; the "
                             f"encoder writes {encoder.latent_dim}, a one-step observation has {actor_critic.num_one_step_obs}")
        self.cell = copy.deepcopy(memory.cell).cpu()
        for p in self.cell.parameters():
            p.requires_grad_(False)
        self.proprio_dim = int(memory.proprio_dim)

    @torch.jit.ignore
    def _memory_columns(self):
        return self.hidden

    @torch.jit.export
    def remember(self, latent: torch.Tensor, obs_history: torch.Tensor, h: torch.Tensor) -> torch.Tensor:
        """latent [B, L], obs_history [B, num_obs], h [B, hidden] (zeros after a reset) -> h' [B, hidden]"""
        return self.cell(torch.cat((latent, obs_history[:, 0:self.proprio_dim]), dim=1), h)

    def forward(self, obs_history: torch.Tensor, frames: torch.Tensor, h: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(actions, h'): encode, remember, act on rows = cat(latent, h')"""
        latent = self.encode(frames)
        h2 = self.remember(latent, obs_history, h)
        return self.act(obs_history, torch.cat((latent, h2), dim=1)), h2


def export_policy_as_jit(actor_critic, path, encoder=None, sensor=None, memory=None):
    """HLP:201-212.  `path` is a directory; returns the file written (policy.pt for HIM and vision policies, policy_1.pt for a bare actor).
    A vision policy needs its `encoder` and `sensor` (or the sensor's spec()): without them the module could not run, and this raises;
    one trained with a depth memory also its `memory` (the exported module then has remember() and forward(obs_history, frames, h))."""
    if hasattr(actor_critic, "depth_latent_dim"):
        if encoder is None or sensor is None:
            raise ValueError("export_policy_as_jit: a vision policy exports with its depth encoder and sensor (encoder=..., sensor=...)")
        if memory is not None:
            return PolicyExporterVisionMemory(actor_critic, encoder, sensor, memory).export(path)
        return PolicyExporterVision(actor_critic, encoder, sensor).export(path)
    if hasattr(actor_critic, "estimator"):
        return PolicyExporterHIM(actor_critic).export(path)
    os.makedirs(path, exist_ok=True)
    out = os.path.join(path, "policy_1.pt")
    torch.jit.script(plain_sequential(actor_critic.actor)).save(out)
    return out
