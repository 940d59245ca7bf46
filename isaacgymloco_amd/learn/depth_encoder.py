"""Depth encoder: a small CNN over the frame history of a modelled range sensor (envs/sensors.py, SensorModel) -> a latent row per env.

    cam = env.add_sensor("depth", depth_camera(env, 64, 48, 87.0, model=SensorModel(period=5, stagger=True, latency=1, frames=2, normalise=True)))
    enc = DepthEncoder(48, 64, frames=2).to(env.device)
    cam.attach_encoder(enc)                 # from now on every capture is followed by ONE more launch on the same stream
    z = cam.latent()                        # [N, 64], live: row e is the encoding of env e's last capture

Three paths over ONE set of parameters (nn.Conv2d, nn.Conv2d, nn.Linear; include/lsim.h, lsim_depth_encode, states the formulas):
  * `forward(frames)` is plain torch -- autograd through six library launches, the CPU;
  * `encode_device(sensor, tick)` is the fused HIP launch of the rollout: forward only, one workgroup per env that is DUE on `tick` (the
    sensor model's rule, so with a staggered period P it encodes 1 env in P), activations in LDS, the parameters read where torch keeps
    them -- no packing step, so an optimiser step is seen by the next launch;
  * `forward_device(frames)` is the training path on the device: the same fused launch over a batch of frames with autograd attached, whose
    backward is lsim_depth_encode_backward -- the conv activations are recomputed per sample in LDS, so nothing of their size is saved or
    written.  The gradients go where learn/fused_linear.py puts its own: into a GradArena's slices when one is set.
There is no torch fall-back behind the two device paths: a library without the entry points raises.
The latent as an input of the actor, the rollout storage and the runner is learn/vision.py.  Not here: a gradient
with respect to the frames, a device-side tick."""
import contextlib
import ctypes

import torch
from torch import nn
from torch.nn import functional as F

from .. import abi, lib
from . import fused_linear

_PARAM_NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")
_live_rows = {}


def _all_live(device, batch):
    """[batch] int64 zeros: the episode_length of lsim_depth_encode for rows that are all encoded (FILL_ALL)"""
    t = _live_rows.get(device)
    if t is None or t.numel() < batch:
        t = _live_rows[device] = torch.zeros(batch, dtype=torch.int64, device=device)
    return t


def check_params(what, names, params, dev):
    """the launches read the parameters' own storage: each must be fp32, contiguous and on `dev`"""
    for name, p in zip(names, params):
        if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
            raise ValueError(f"{what}: parameter {name} must be fp32, contiguous and on {dev} (is {p.dtype}, "
                             f"{'contiguous' if p.is_contiguous() else 'strided'}, {p.device})")


def _launch_struct(enc, hist_ptr, hist_stride, hist_slots, episode_length, num_envs, env_stride, latent, params, tick, period, stagger, flags):
    """the lsim_depth_encoder_t of ONE launch: `enc`'s extents, the frame history, the envs, the latent buffer and the parameters"""
    de = abi.LsimDepthEncoder.from_buffer_copy(enc._extents)
    de.hist, de.hist_stride, de.hist_slots = hist_ptr, hist_stride, hist_slots
    de.episode_length, de.num_envs, de.env_stride = episode_length, num_envs, env_stride
    de.w1, de.b1, de.w2, de.b2, de.w3, de.b3 = (p.data_ptr() for p in params)
    de.final_act = int(enc.final_act)
    de.latent, de.latent_stride = latent.data_ptr(), latent.shape[1]
    de.tick, de.period, de.stagger, de.flags = int(tick), int(period), int(stagger), int(flags)
    return de


def _copy_extents(enc, dst):
    """the ten extents of `enc` into another struct that names them alike (lsim_depth_encoder_bwd_t)"""
    for k in ("height", "width", "frames", "c1", "k1", "s1", "c2", "k2", "s2", "latent_dim"):
        setattr(dst, k, getattr(enc._extents, k))
    return dst


class _DepthEncodeFn(torch.autograd.Function):
    """latent = lsim_depth_encode over a batch of frames (hist_slots = frames, FILL_ALL); backward = lsim_depth_encode_backward"""

    @staticmethod
    def forward(ctx, enc, api, hist, hist_stride, *params):
        B, L = hist.shape[0], enc.latent_dim
        latent = torch.empty(B, (L + 3) // 4 * 4, device=hist.device, dtype=torch.float32)
        de = _launch_struct(enc, hist.data_ptr(), hist_stride, enc.frames, _all_live(hist.device, B).data_ptr(), B, 1, latent, params,
                            0, 1, 0, abi.DEFINES["LSIM_SENSOR_FILL_ALL"])
        lib.check(api.lsim_depth_encode(ctypes.byref(de), torch.cuda.current_stream(hist.device).cuda_stream), what="lsim_depth_encode")
        out = latent[:, :L]
        ctx.enc, ctx.api, ctx.hist_stride = enc, api, hist_stride
        ctx.save_for_backward(hist, out, *params)
        return out

    @staticmethod
    def backward(ctx, g):
        hist, latent, *params = ctx.saved_tensors
        enc, api = ctx.enc, ctx.api
        if g.dtype != torch.float32 or g.stride(1) != 1:
            g = g.float().contiguous()
        db = _copy_extents(enc, abi.LsimDepthEncoderBwd())
        db.hist, db.hist_stride, db.hist_slots, db.batch = hist.data_ptr(), ctx.hist_stride, enc.frames, hist.shape[0]
        db.final_act, db.grid_limit = int(enc.final_act), 0
        db.g, db.g_stride, db.latent, db.latent_stride = g.data_ptr(), g.stride(0), latent.data_ptr(), latent.stride(0)
        lds, need = ctypes.c_size_t(), ctypes.c_size_t()
        lib.check(api.lsim_depth_encode_backward_sizes(ctypes.byref(db), ctypes.byref(lds), ctypes.byref(need)), what="lsim_depth_encode_backward_sizes")
        ws = fused_linear._workspace("depth_encoder_backward", hist.device, need.value)
        db.workspace, db.workspace_bytes = ws.data_ptr(), ws.numel()
        grads = []
        for name, p in zip(_PARAM_NAMES, params):
            setattr(db, name, p.data_ptr())
            grads.append(fused_linear._grad_out(p.data_ptr(), tuple(p.shape), hist.device))
            setattr(db, "g" + name, grads[-1].data_ptr())
        lib.check(api.lsim_depth_encode_backward(ctypes.byref(db), torch.cuda.current_stream(hist.device).cuda_stream), what="lsim_depth_encode_backward")
        return (None, None, None, None) + tuple(gr if need_ else None for gr, need_ in zip(grads, ctx.needs_input_grad[4:]))


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

    def config(self):
        """the constructor's keywords as plain Python values: DepthEncoder(**enc.config()) has this encoder's shapes (a checkpoint's record)"""
        de = self._extents
        return {"height": self.height, "width": self.width, "frames": self.frames, "c1": int(de.c1), "k1": int(de.k1), "s1": int(de.s1),
                "c2": int(de.c2), "k2": int(de.k2), "s2": int(de.s2), "latent_dim": self.latent_dim, "final_act": self.final_act}

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
        entry = lib.entry(sensor._api, "lsim_depth_encode", "the depth encoder")
        hist = sensor.history()
        params = self.device_params()
        check_params("encode_device", _PARAM_NAMES, params, hist.device)
        latent = sensor.latent_buffer(self.latent_dim)
        de = _launch_struct(self, hist.data_ptr(), hist.shape[2], hist.shape[1], sensor.episode_length_ptr, hist.shape[0], sensor.env_stride,
                            latent, params, tick, model.period, model.stagger, flags)
        lib.check(entry(ctypes.byref(de), sensor._stream(stream)), what="lsim_depth_encode")
        return latent[:, :self.latent_dim]

    def forward_device(self, frames, stream=None, api=None):
        """[B, frames, height, width] fp32 on the parameters' device -> [B, latent_dim] WITH autograd to the six parameters: ONE launch of
        lsim_depth_encode over the batch now, the launches of lsim_depth_encode_backward when the result is back-propagated (on `stream`, a
        torch.cuda.Stream; default: the current one).  Contiguous frames whose height * width is a multiple of 4 are read in place, others
        through a padded copy.  The frames are sensor data: there is no gradient with respect to them, and frames that ask for one raise."""
        api = api if api is not None else lib.load()
        for name in ("lsim_depth_encode", "lsim_depth_encode_backward_sizes", "lsim_depth_encode_backward"):
            lib.entry(api, name, "the depth encoder")
        if frames.requires_grad:
            raise ValueError("forward_device: frames.requires_grad is set, but the depth encoder has no gradient with respect to its frames")
        if frames.dim() != 4 or tuple(frames.shape[1:]) != (self.frames, self.height, self.width) or frames.shape[0] < 1:
            raise ValueError(f"forward_device: frames must be [B >= 1, {self.frames}, {self.height}, {self.width}], got {tuple(frames.shape)}")
        params = self.device_params()
        dev = params[0].device
        if frames.dtype != torch.float32 or frames.device != dev:
            raise ValueError(f"forward_device: frames must be fp32 on {dev} (are {frames.dtype}, {frames.device})")
        check_params("forward_device", _PARAM_NAMES, params, dev)
        R = self.height * self.width
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            if frames.is_contiguous() and R % 4 == 0 and frames.data_ptr() % 16 == 0:
                hist, stride = frames, R
            else:
                stride = (R + 3) // 4 * 4
                hist = torch.zeros(frames.shape[0], self.frames, stride, device=dev, dtype=torch.float32)
                hist[:, :, :R] = frames.reshape(frames.shape[0], self.frames, R)
            return _DepthEncodeFn.apply(self, api, hist, stride, *params)

    def forward_device_rows(self, rows, api=None):
        """forward_device over images that already lie as the launch reads them -- [B >= 1, frames, stride] fp32, contiguous, 16-byte
        aligned, stride >= height * width a multiple of 4 (a sensor's frame log) -- read in place whatever height * width is"""
        api = api if api is not None else lib.load()
        for name in ("lsim_depth_encode", "lsim_depth_encode_backward_sizes", "lsim_depth_encode_backward"):
            lib.entry(api, name, "the depth encoder")
        params = self.device_params()
        dev = params[0].device
        ok = (rows.dim() == 3 and rows.shape[0] >= 1 and rows.shape[1] == self.frames and rows.shape[2] >= self.height * self.width and rows.shape[2] % 4 == 0
              and rows.dtype == torch.float32 and rows.device == dev and rows.is_contiguous() and rows.data_ptr() % 16 == 0 and not rows.requires_grad)
        if not ok:
            raise ValueError(f"forward_device_rows: rows must be contiguous, 16-byte aligned fp32 [B >= 1, {self.frames}, stride] on {dev} without "
                             f"a gradient, stride >= {self.height * self.width} a multiple of 4, got {tuple(rows.shape)} {rows.dtype} on {rows.device}")
        check_params("forward_device_rows", _PARAM_NAMES, params, dev)
        return _DepthEncodeFn.apply(self, api, rows, rows.shape[2], *params)
