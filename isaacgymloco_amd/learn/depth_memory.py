"""Depth memory: one GRU cell behind the depth encoder (learn/depth_encoder.py), so that the actor reads [z | h] -- the encoding of the last
capture and what the cell has integrated over the captures before it.  The reference's precedent is the `Memory` of
rsl_rl/modules/actor_critic_recurrent.py: a recurrent cell whose hidden state is zeroed on `dones`.

    mem = DepthMemory(enc.latent_dim, env.num_one_step_obs, hidden=64).to(env.device)
    cam.attach_memory(mem)                  # behind the encoder's launch of every update(): ONE more launch on the same stream
    rows = cam.memory_rows()                # [N, L + H], live: row e = [z_e | h_e]; cam.memory_state() is h [N, H]

The module is the cell's weights and the launches over them.  Everything per env -- h and the rows -- belongs to the sensor it is attached
to (envs/sensors.py), next to the latent, so one DepthMemory serves any number of sensors and envs (a training env and an evaluation env).

Four paths over ONE nn.GRUCell (gate order r, z, n; include/lsim.h, lsim_depth_memory_step, states the formulas):
  * `forward(z, p, h, fresh)` is one step in plain torch; `sequence(x, h0, reset)` the loop over it -- the CPU path and the twin in tests;
  * `step_device(sensor, flags)` is the rollout launch: every env, every control step, z held between captures and p fresh, the parameters
    read where torch keeps them -- no packing step, so an optimiser step is seen by the next launch;
  * `sequence_device(x, h0, reset)` is the training path on the device: one library GEMM for the input projection of all T * n rows, the serial
    recurrence in lsim_gru_sequence_forward, and under autograd lsim_gru_sequence_backward followed by the four parameter-gradient GEMMs /
    column sums in torch.  There is no gradient with respect to x: the stored latent is detached by design.
There is no torch fall-back behind the two device paths: a library without the entry points raises."""
import ctypes

import torch
from torch import nn

from .. import abi, lib
from .depth_encoder import check_params

_PARAM_NAMES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
_ENTRIES = ("lsim_depth_memory_step", "lsim_gru_sequence_forward", "lsim_gru_sequence_backward", "lsim_depth_memory_sizes")


def _entry(api, name):
    return lib.entry(api, name, "the depth memory")


def _stream_of(t):
    return torch.cuda.current_stream(t.device).cuda_stream if t.is_cuda else None


class _GruSequenceFn(torch.autograd.Function):
    """hs = the recurrence over [T, n, I] rows; backward = lsim_gru_sequence_backward, then the parameter gradients as GEMMs over T * n rows"""

    @staticmethod
    def forward(ctx, api, x, h0, reset, w_ih, w_hh, b_ih, b_hh):
        T, n, I = x.shape
        H = h0.shape[1]
        gi = torch.addmm(b_ih, x.reshape(T * n, I), w_ih.t())
        hs = torch.empty(T, n, H, device=x.device, dtype=torch.float32)
        save = torch.empty(T, n, 4 * H, device=x.device, dtype=torch.float32)
        gs = abi.STRUCTS["lsim_gru_sequence_t"]()
        gs.gi, gs.h0, gs.reset, gs.weight_hh, gs.bias_hh = gi.data_ptr(), h0.data_ptr(), reset.data_ptr(), w_hh.data_ptr(), b_hh.data_ptr()
        gs.hs, gs.save, gs.steps, gs.num_envs, gs.hidden = hs.data_ptr(), save.data_ptr(), T, n, H
        lib.check(_entry(api, "lsim_gru_sequence_forward")(ctypes.byref(gs), _stream_of(x)), what="lsim_gru_sequence_forward")
        ctx.api = api
        ctx.save_for_backward(x, h0, reset, w_hh, hs, save)
        return hs

    @staticmethod
    def backward(ctx, dhs):
        x, h0, reset, w_hh, hs, save = ctx.saved_tensors
        T, n, I = x.shape
        H = h0.shape[1]
        dhs = dhs.float().contiguous()
        dgi = torch.empty(T, n, 3 * H, device=x.device, dtype=torch.float32)
        dghn = torch.empty(T, n, H, device=x.device, dtype=torch.float32)
        dh0 = torch.empty(n, H, device=x.device, dtype=torch.float32)
        gs = abi.STRUCTS["lsim_gru_sequence_t"]()
        gs.h0, gs.reset, gs.weight_hh, gs.hs, gs.save = h0.data_ptr(), reset.data_ptr(), w_hh.data_ptr(), hs.data_ptr(), save.data_ptr()
        gs.dhs, gs.dgi, gs.dghn, gs.dh0 = dhs.data_ptr(), dgi.data_ptr(), dghn.data_ptr(), dh0.data_ptr()
        gs.steps, gs.num_envs, gs.hidden = T, n, H
        lib.check(_entry(ctx.api, "lsim_gru_sequence_backward")(ctypes.byref(gs), _stream_of(x)), what="lsim_gru_sequence_backward")
        need = ctx.needs_input_grad
        g2 = dgi.reshape(T * n, 3 * H)
        gw_ih = g2.t() @ x.reshape(T * n, I) if need[4] else None
        gb_ih = g2.sum(0) if need[6] else None
        gw_hh = gb_hh = None
        if need[5] or need[7]:
            gh = torch.cat((g2[:, :2 * H], dghn.reshape(T * n, H)), dim=1)            # [dgi_r | dgi_u | dghn]
            if need[5]:
                h_prev = torch.cat((h0.unsqueeze(0), hs[:-1]), dim=0) * (reset == 0).unsqueeze(-1)
                gw_hh = gh.t() @ h_prev.reshape(T * n, H)
            gb_hh = gh.sum(0) if need[7] else None
        return None, None, (dh0 if need[2] else None), None, gw_ih, gw_hh, gb_ih, gb_hh


class DepthMemory(nn.Module):
    """h' = GRUCell([z | p], h) with h = 0 for a fresh env; `latent_dim` columns of the encoder's latent, `proprio_dim` columns of the env's
    current one-step observation (may be 0), `hidden` a multiple of 16 that lsim_depth_memory_sizes accepts (16 .. 96)"""

    def __init__(self, latent_dim, proprio_dim, hidden=64):
        super().__init__()
        self.latent_dim, self.proprio_dim, self.hidden = int(latent_dim), int(proprio_dim), int(hidden)
        d = abi.DEFINES
        if self.latent_dim < 1 or self.proprio_dim < 0 or self.latent_dim + self.proprio_dim > d["LSIM_GRU_MAX_INPUT"]:
            raise ValueError(f"DepthMemory: latent_dim >= 1, proprio_dim >= 0, latent_dim + proprio_dim <= {d['LSIM_GRU_MAX_INPUT']}")
        if self.hidden < 16 or self.hidden % 16 or self.hidden > d["LSIM_GRU_MAX_HIDDEN"]:
            raise ValueError(f"DepthMemory: hidden must be a multiple of 16 in 16 .. {d['LSIM_GRU_MAX_HIDDEN']}, got {self.hidden}")
        self.cell = nn.GRUCell(self.latent_dim + self.proprio_dim, self.hidden)

    @property
    def input_dim(self):
        return self.latent_dim + self.proprio_dim

    def config(self):
        """the constructor's keywords as plain Python values (a checkpoint's record)"""
        return {"latent_dim": self.latent_dim, "proprio_dim": self.proprio_dim, "hidden": self.hidden}

    def device_params(self):
        """(weight_ih, weight_hh, bias_ih, bias_hh): the parameters in the order of lsim_depth_memory_t"""
        c = self.cell
        return (c.weight_ih, c.weight_hh, c.bias_ih, c.bias_hh)

    def lds_bytes(self, api=None):
        """(step, forward, backward) bytes of dynamic LDS (lsim_depth_memory_sizes); raises when the kernels do not take this cell"""
        api = api if api is not None else lib.load()
        a, b, c = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        lib.check(_entry(api, "lsim_depth_memory_sizes")(self.hidden, self.input_dim, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)),
                  what="lsim_depth_memory_sizes")
        return a.value, b.value, c.value

    # ---- plain torch
    def forward(self, z, p, h, fresh=None):
        """one step: z [N, L], p [N, P] (None with proprio_dim 0), h [N, H], fresh [N] bool (h_prev = 0 there) -> h' [N, H]"""
        x = z if self.proprio_dim == 0 else torch.cat((z, p), dim=-1)
        if fresh is not None:
            h = h * (~fresh.bool()).unsqueeze(-1).to(h.dtype)
        return self.cell(x, h)

    def sequence(self, x, h0, reset):
        """x [T, n, I], h0 [n, H], reset [T, n] (nonzero: h_prev = 0 at that step) -> hs [T, n, H]; the torch loop"""
        h, out = h0, []
        for t in range(x.shape[0]):
            h = self.cell(x[t], h * (reset[t] == 0).unsqueeze(-1).to(h.dtype))
            out.append(h)
        return torch.stack(out)

    # ---- the library
    def sequence_device(self, x, h0, reset, api=None):
        """`sequence` through lsim_gru_sequence_forward, with autograd to the four parameters (and h0) through lsim_gru_sequence_backward;
        x must not ask for a gradient.  `api`: the library (default) or the CPU shim of the tests, which takes host tensors"""
        api = api if api is not None else lib.load()
        for name in _ENTRIES[1:3]:
            _entry(api, name)
        if x.requires_grad:
            raise ValueError("sequence_device: x.requires_grad is set, but the depth memory has no gradient with respect to its input rows")
        if x.dim() != 3 or x.shape[2] != self.input_dim or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError(f"sequence_device: x must be [T >= 1, n >= 1, {self.input_dim}], got {tuple(x.shape)}")
        T, n = x.shape[:2]
        if tuple(h0.shape) != (n, self.hidden) or tuple(reset.shape) != (T, n):
            raise ValueError(f"sequence_device: h0 must be [{n}, {self.hidden}] and reset [{T}, {n}], got {tuple(h0.shape)} and {tuple(reset.shape)}")
        check_params("sequence_device", _PARAM_NAMES, self.device_params(), x.device)
        if x.dtype != torch.float32 or h0.dtype != torch.float32 or h0.device != x.device or reset.device != x.device:
            raise ValueError("sequence_device: x and h0 must be fp32, and x, h0 and reset on the parameters' device")
        reset = (reset != 0).to(torch.uint8).contiguous()
        return _GruSequenceFn.apply(api, x.contiguous(), h0.contiguous(), reset, *self.device_params())

    def step_device(self, sensor, flags=0, stream=None):
        """ONE launch of lsim_depth_memory_step on `stream` (default: the sensor's): z = the sensor's live latent rows, p = the first
        proprio_dim columns of the env's obs_buf, freshness from the env's episode_length, h and the rows [N, L + H] the sensor's own
        (RaySensor.attach_memory).  Returns the live rows."""
        entry = _entry(sensor._api, "lsim_depth_memory_step")
        try:
            z = sensor.latent()
        except ValueError:
            raise ValueError("step_device: the sensor has no encoder (attach_encoder), so no latent rows") from None
        if z.shape[1] != self.latent_dim:
            raise ValueError(f"step_device: the memory reads {self.latent_dim} latent columns, the sensor's encoder writes {z.shape[1]}")
        check_params("step_device", _PARAM_NAMES, self.device_params(), z.device)
        held = sensor.stage("memory").buffers if sensor.stage("memory") is not None else {}
        h, rows = held.get("h"), held.get("rows")
        if h is None or h.shape[1] != self.hidden or rows.shape[1] != self.latent_dim + self.hidden:
            raise ValueError(f"step_device: the sensor holds no memory buffers of this cell's widths ({self.latent_dim} latent columns, "
                             f"{self.hidden} hidden): attach the memory to it (RaySensor.attach_memory)")
        dm = abi.STRUCTS["lsim_depth_memory_t"]()
        dm.z, dm.z_ld = z.data_ptr(), z.stride(0)
        if self.proprio_dim:
            obs = sensor.env.obs_buf
            if obs.dim() != 2 or obs.shape[1] < self.proprio_dim or obs.stride(1) != 1 or obs.dtype != torch.float32 or obs.device != z.device:
                raise ValueError(f"step_device: the env's obs_buf must be fp32 [N, >= {self.proprio_dim}] on {z.device}")
            dm.p, dm.p_ld = obs.data_ptr(), obs.stride(0)
        dm.episode_length = sensor.episode_length_ptr
        dm.weight_ih, dm.weight_hh, dm.bias_ih, dm.bias_hh = (p.data_ptr() for p in self.device_params())
        dm.h, dm.h_ld, dm.rows, dm.rows_ld = h.data_ptr(), h.stride(0), rows.data_ptr(), rows.stride(0)
        dm.num_envs, dm.latent_dim, dm.proprio_dim, dm.hidden, dm.flags = z.shape[0], self.latent_dim, self.proprio_dim, self.hidden, int(flags)
        lib.check(entry(ctypes.byref(dm), sensor._stream(stream)), what="lsim_depth_memory_step")
        return rows
