"""Depth encoder: a small CNN over the frame history of a modelled range sensor (envs/sensors.py, SensorModel) -> a latent row per env.

    cam = env.add_sensor("depth", depth_camera(env, 64, 48, 87.0, model=SensorModel(period=5, stagger=True, latency=1, frames=2, normalise=True)))
    enc = DepthEncoder(48, 64, frames=2).to(env.device)
    cam.attach_encoder(enc)                 # from now on every capture is followed by ONE more launch on the same stream
    z = cam.latent()                        # [N, 64], live: row e is the encoding of env e's last capture

Two paths over ONE set of parameters (nn.Conv2d, nn.Conv2d, nn.Linear; include/lsim.h, lsim_depth_encode, states the formulas):
  * `forward(frames)` is plain torch -- autograd, the PPO update, the CPU;
  * `encode_device(sensor, tick)` is the fused HIP launch of the rollout: forward only, one workgroup per env that is DUE on `tick` (the
    sensor model's rule, so with a staggered period P it encodes 1 env in P), activations in LDS, the parameters read where torch keeps
    them -- no packing step, so an optimiser step is seen by the next launch.  There is no torch fall-back: a library without the entry
    point raises.
Not here: a backward kernel, the latent as an input of HIMActorCritic / the runner / the rollout storage, a
device-side tick."""
import ctypes

import torch
from torch import nn
from torch.nn import functional as F

from .. import abi, lib


class DepthEncoder(nn.Module):
    """ELU(conv1) -> ELU(conv2) -> fc (-> ELU when `final_act`) on [B, frames, height, width]; no padding, no dilation"""

    def __init__(self, height, width, frames, c1=16, k1=5, s1=2, c2=32, k2=3, s2=2, latent_dim=64, final_act=True):
        super().__init__()
        self.height, self.width, self.frames = int(height), int(width), int(frames)
        self.latent_dim, self.final_act = int(latent_dim), bool(final_act)
        de = abi.LsimDepthEncoder()
        de.height, de.width, de.frames = self.height, self.width, self.frames
        de.c1, de.k1, de.s1, de.c2, de.k2, de.s2, de.latent_dim = int(c1), int(k1), int(s1), int(c2), int(k2), int(s2), self.latent_dim
        self._extents = de
        d = abi.DEFINES
        if not (1 <= de.k1 <= min(self.height, self.width, d["LSIM_DEPTH_ENC_MAX_KERNEL"]) and 1 <= de.s1 and 1 <= de.c1 and self.frames >= 1):
            raise ValueError("DepthEncoder: 1 <= k1 <= min(height, width, 8), s1 >= 1, c1 >= 1, frames >= 1")
        self.h1, self.w1 = (self.height - de.k1) // de.s1 + 1, (self.width - de.k1) // de.s1 + 1
        if not (1 <= de.k2 <= min(self.h1, self.w1) and 1 <= de.s2 and 1 <= de.c2 and self.latent_dim >= 1):
            raise ValueError(f"DepthEncoder: 1 <= k2 <= min(h1, w1) = {min(self.h1, self.w1)}, s2 >= 1, c2 >= 1, latent_dim >= 1")
        self.h2, self.w2 = (self.h1 - de.k2) // de.s2 + 1, (self.w1 - de.k2) // de.s2 + 1
        self.conv1 = nn.Conv2d(self.frames, de.c1, de.k1, de.s1)
        self.conv2 = nn.Conv2d(de.c1, de.c2, de.k2, de.s2)
        self.fc = nn.Linear(de.c2 * self.h2 * self.w2, self.latent_dim)

    def forward(self, frames):
        x = F.elu(self.conv1(frames))
        x = F.elu(self.conv2(x))
        z = self.fc(torch.flatten(x, 1))
        return F.elu(z) if self.final_act else z

    def device_params(self):
        """(w1, b1, w2, b2, w3, b3): the parameters in the order of lsim_depth_encoder_t"""
        return (self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias, self.fc.weight, self.fc.bias)

    def lds_bytes(self, api=None):
        """dynamic LDS of the launch for this configuration (lsim_depth_encode_sizes); raises when the kernel does not support it"""
        api = api if api is not None else lib.load()
        n = ctypes.c_size_t()
        lib.check(api.lsim_depth_encode_sizes(ctypes.byref(self._extents), ctypes.byref(n)), what="lsim_depth_encode_sizes")
        return n.value

    def encode_device(self, sensor, tick, flags=0, stream=None):
        """ONE launch of lsim_depth_encode on `stream` (default: the sensor's) over `sensor`'s frame history: the envs due on `tick` under
        `flags` (the values of the sensor's capture) get a new latent row, the others keep theirs.  Returns the live [N, latent_dim] buffer
        (sensor.latent()).  The launch reads the parameters' own storage: they must be fp32, contiguous and on the env's device."""
        model = getattr(sensor, "model", None)
        if model is None:
            raise ValueError("encode_device: the sensor has no model, so no frame history (RaySensor(model=SensorModel(...)))")
        if sensor.num_rays != self.height * self.width or model.frames != self.frames:
            raise ValueError(f"encode_device: the encoder expects {self.frames} frames of {self.height} x {self.width} rays, the sensor has "
                             f"{model.frames} of {sensor.num_rays}")
        entry = getattr(sensor._api, "lsim_depth_encode", None)
        if entry is None:
            raise lib.LsimError("the loaded library has no lsim_depth_encode: rebuild it (there is no torch fall-back for the depth encoder)")
        hist = sensor._hist
        for name, p in zip(("w1", "b1", "w2", "b2", "w3", "b3"), self.device_params()):
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != hist.device:
                raise ValueError(f"encode_device: parameter {name} must be fp32, contiguous and on {hist.device} (is {p.dtype}, "
                                 f"{'contiguous' if p.is_contiguous() else 'strided'}, {p.device})")
        latent = sensor._latent_buffer(self.latent_dim)
        de = abi.LsimDepthEncoder.from_buffer_copy(self._extents)
        sm = sensor._sm
        de.hist, de.hist_stride, de.hist_slots = hist.data_ptr(), hist.shape[2], hist.shape[1]
        de.episode_length, de.num_envs, de.env_stride = sm.episode_length, hist.shape[0], sensor.env_stride
        de.w1, de.b1, de.w2, de.b2, de.w3, de.b3 = (p.data_ptr() for p in self.device_params())
        de.final_act = int(self.final_act)
        de.latent, de.latent_stride = latent.data_ptr(), latent.shape[1]
        de.tick, de.period, de.stagger, de.flags = int(tick), model.period, int(model.stagger), int(flags)
        lib.check(entry(ctypes.byref(de), sensor._stream(stream)), what="lsim_depth_encode")
        return latent[:, :self.latent_dim]
