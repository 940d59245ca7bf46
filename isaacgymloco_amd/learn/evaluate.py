"""Evaluate a trained policy on the device: metrics per robot x terrain type x terrain level, and state traces of chosen envs.

    python -m isaacgymloco_amd.learn.evaluate --task aliengo [--robots aliengo=0.5,go2=0.5] --checkpoint model.pt --envs 4096 --steps 1000 \
        --commands 1.0,0,0 --out eval.json [--trace-envs 0,1 --trace-out trace.npz] [--blind] [--vision-metrics depth_influence,scan_error] \
        [--odometry trained|off|scale=0.02,yaw_per_m=0.01,z_per_m=0.01,noise=0.005:0.002:0.002]

The evaluation half of the reference's legged_gym/scripts/play.py (fixed commands, randomisation off, deterministic actions; play.py:66-85 and
play.py:124-133).  Every env-step costs ONE extra HIP launch, `lsim_eval_accumulate` (include/lsim.h states the semantics; csrc/ls_eval.h is the
kernel): sums in 2^-32 fixed-point int64 words per group, bitwise reproducible, no host synchronisation.  The evaluator only reads the
simulator's buffers.  The numbers are measurements of the policy on THIS simulator: its dynamics are not pinned against PhysX.
"""
import argparse
import copy
import ctypes
import json
import math
import os
import sys

import numpy as np
import torch

from .. import abi, lib
from ..envs import config as C
from ..envs import sensors
from .policy_io import policy_parts, policy_record

GROUP_BITS = {"robot": abi.DEFINES["LSIM_EVAL_BY_ROBOT"], "type": abi.DEFINES["LSIM_EVAL_BY_TYPE"], "level": abi.DEFINES["LSIM_EVAL_BY_LEVEL"]}
TRACE_DIM = abi.DEFINES["LSIM_EVAL_TRACE_DIM"]
MAX_TRACE_ENVS = abi.DEFINES["LSIM_EVAL_MAX_TRACE_ENVS"]
SAT_THRESHOLD = abi.DEFINES["LSIM_EVAL_SAT_PERMILLE"] / 1000.0
FIX_ONE = 2.0 ** 32
CLAMP = float(2 ** 20)
W = abi.EVAL_WORDS
MAX_COLUMNS = abi.DEFINES["LSIM_EVAL_MAX_COLUMNS"]
COL_WORDS = abi.DEFINES["LSIM_EVAL_COL_WORDS"]
# name -> (first column, width) of a trace row, in the order of the LSIM_EVAL_TR_* offsets
_TR = sorted(((v, k[len("LSIM_EVAL_TR_"):].lower()) for k, v in abi.DEFINES.items() if k.startswith("LSIM_EVAL_TR_")))
TRACE_COLUMNS = {name: (start, (_TR[i + 1][0] if i + 1 < len(_TR) else TRACE_DIM) - start) for i, (start, name) in enumerate(_TR)}


def play_cfg(cfg, keep_terminations=True):
    """A copy of an env config (single robot or mixed_cfg) with the evaluation overrides of the reference's play.py:66-85: observation noise,
    friction / payload randomisation, pushes and the disturbance force off; terrain curriculum off (robots start on random levels up to
    max_init_terrain_level = 5 and stay in their cell); heading command and command curriculum off; commands never resampled
    (resampling_time 1e4).  num_envs and the terrain's size stay the caller's.  play.py also empties terminate_after_contacts_on;
    falls are what an evaluation wants to count, so that is opt-in here: keep_terminations=False."""
    cfg = copy.deepcopy(cfg)
    cfg.terrain.curriculum = False
    cfg.terrain.max_init_terrain_level = 5
    cfg.noise.add_noise = False
    cfg.domain_rand.randomize_friction = False
    cfg.domain_rand.push_robots = False
    cfg.domain_rand.disturbance = False
    cfg.domain_rand.randomize_payload_mass = False
    cfg.commands.heading_command = False
    cfg.commands.curriculum = False
    cfg.commands.resampling_time = 10000.0
    if not keep_terminations:
        cfg.asset.terminate_after_contacts_on = []
        for r in getattr(cfg, "robots", None) or []:
            if "asset" in r["overrides"]:
                r["overrides"]["asset"].terminate_after_contacts_on = []
    return cfg


def group_mask(group_by):
    mask = 0
    for g in group_by:
        if g not in GROUP_BITS:
            raise ValueError(f"unknown group_by entry {g!r}: one of {sorted(GROUP_BITS)}")
        mask |= GROUP_BITS[g]
    return mask


def group_shape(mask, num_robots, num_types, num_levels):
    return (num_robots if mask & GROUP_BITS["robot"] else 1, num_types if mask & GROUP_BITS["type"] else 1, num_levels if mask & GROUP_BITS["level"] else 1)


def group_index(mask, shape, robot, ttype, level):
    """the table row of (robot, type, level): collapsed factors count as 0"""
    r = robot if mask & GROUP_BITS["robot"] else 0
    t = ttype if mask & GROUP_BITS["type"] else 0
    l = level if mask & GROUP_BITS["level"] else 0
    return (r * shape[1] + t) * shape[2] + l


def group_key(mask, shape, index, robot_names):
    """table row -> {"robot": name, "type": int, "level": int} with only the kept factors"""
    l = index % shape[2]
    t = (index // shape[2]) % shape[1]
    r = index // (shape[1] * shape[2])
    key = {}
    if mask & GROUP_BITS["robot"]:
        key["robot"] = robot_names[r]
    if mask & GROUP_BITS["type"]:
        key["type"] = int(t)
    if mask & GROUP_BITS["level"]:
        key["level"] = int(l)
    return key


def key_index(mask, shape, key, robot_names):
    """inverse of group_key"""
    return group_index(mask, shape, robot_names.index(key["robot"]) if "robot" in key else 0, key.get("type", 0), key.get("level", 0))


def metrics_of_row(row):
    """One table row (LSIM_EVAL_WORDS int64 words, or a sum of rows) -> float64 means / rates / RMS values with their counts.
    Per-sample means divide by `samples` (env-steps that did not end an episode), per-episode means by `episodes`."""
    row = [int(v) for v in row]
    n, ep = row[W["samples"]], row[W["episodes"]]
    per = lambda w, d: (row[W[w]] / FIX_ONE / d) if d else float("nan")
    cnt = lambda w, d: (row[W[w]] / d) if d else float("nan")
    return {
        "samples": n, "episodes": ep, "time_outs": row[W["time_outs"]], "falls": row[W["falls"]], "nonfinite": row[W["nonfinite"]],
        "lin_vel_error_mean": per("lin_err", n), "lin_vel_error_rms": per("lin_err_sq", n) ** 0.5 if n else float("nan"),
        "yaw_rate_error_mean": per("yaw_err", n), "yaw_rate_error_rms": per("yaw_err_sq", n) ** 0.5 if n else float("nan"),
        "mechanical_power_mean": per("power", n), "torque_rms": (per("torque_sq", n) / 12.0) ** 0.5 if n else float("nan"),
        "action_rate_mean": per("action_rate", n), "feet_in_contact_mean": cnt("feet_contact", n),
        "torque_saturation_rate": cnt("torque_sat", 12 * n), "peak_torque_ratio": row[W["peak_torque_ratio"]] / FIX_ONE,
        "fall_rate": cnt("falls", ep), "time_out_rate": cnt("time_outs", ep),
        "episode_return_mean": per("return", ep), "episode_length_mean": cnt("length", ep), "episode_distance_mean": per("distance", ep),
    }


def columns_of_row(row, names):
    """One row of the columns table ([samples | sum, sum of squares, non-finite count per column], or a sum of rows) -> {name: mean, rms, nonfinite}"""
    row = [int(v) for v in row]
    n = row[0]
    out = {}
    for k, name in enumerate(names):
        s, q, bad = row[1 + COL_WORDS * k:1 + COL_WORDS * (k + 1)]
        out[name] = {"mean": s / FIX_ONE / n if n else float("nan"), "rms": (q / FIX_ONE / n) ** 0.5 if n else float("nan"), "nonfinite": bad}
    return out


def total_row(table):
    """sum of the rows of an int64 table [groups, words]: integer sums, except the peak word (a maximum)"""
    tot = table.sum(axis=0)
    tot[W["peak_torque_ratio"]] = table[:, W["peak_torque_ratio"]].max()
    return tot


class Evaluator:
    """Owns the evaluator's device state for one env: `.accumulate()` after every `env.step_device(...)`, `.result()` / `.trace()` at the end."""

    def __init__(self, env, group_by=("robot", "type", "level"), trace_envs=(), trace_capacity=1024, api=None):
        """`api`: an object with lsim_eval_sizes / _clear / _accumulate in place of the HIP library's (the test suite's CPU shim of the kernel source)"""
        self.env = env
        dev = env.buf["rew"].device
        N = env.num_envs
        self.mask = group_mask(group_by)
        self.robot_names = list(getattr(env, "robot_names", None) or [getattr(env.cfg.asset, "name", "robot")])
        has_grid = env.cfg.terrain.mesh_type in ("heightfield", "trimesh")
        self.num_types = int(env.cfg.terrain.num_cols) if has_grid else 1
        self.num_levels = int(env.cfg.terrain.num_rows) if has_grid else 1
        self.shape = group_shape(self.mask, len(self.robot_names), self.num_types, self.num_levels)
        self.num_groups = self.shape[0] * self.shape[1] * self.shape[2]
        self.trace_envs = [int(i) for i in trace_envs]
        if len(self.trace_envs) > MAX_TRACE_ENVS:
            raise ValueError(f"at most {MAX_TRACE_ENVS} trace envs, got {len(self.trace_envs)}")
        self.trace_capacity = int(trace_capacity)
        self._L = api if api is not None else lib.load()
        sb, tb, rb = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        lib.check(self._L.lsim_eval_sizes(N, self.num_groups, len(self.trace_envs), self.trace_capacity, ctypes.byref(sb), ctypes.byref(tb), ctypes.byref(rb)),
                  what="lsim_eval_sizes")
        self.state = torch.zeros(sb.value // 8, dtype=torch.int64, device=dev)
        self.table = torch.zeros(self.num_groups, abi.NUM_EVAL_WORDS, dtype=torch.int64, device=dev)
        self.trace_buf = torch.zeros(self.trace_capacity, len(self.trace_envs), TRACE_DIM, dtype=torch.float32, device=dev)
        per_env = lambda t: t.to(device=dev, dtype=torch.float32).expand(N, 12).contiguous()
        self._const = {"torque_limits": per_env(env.torque_limits), "default_dof_pos": per_env(env.default_dof_pos), "action_scale": per_env(env.action_scales)}
        if getattr(env, "robots", None) is not None:
            self._const["robot_ids"] = env.robot_ids.to(torch.uint8).contiguous()
        e = abi.LsimEval()
        b = env.buf
        for field, name in (("rew", "rew"), ("reset_buf", "reset"), ("time_out_buf", "time_out"), ("commands", "commands"), ("base_lin_vel", "base_lin_vel"),
                            ("base_ang_vel", "base_ang_vel"), ("root_states", "root_states"), ("dof_state", "dof_state"), ("torques", "torques"),
                            ("actions", "actions"), ("last_actions", "last_actions"), ("contact_filt", "contact_filt"), ("contact_forces", "contact_forces"),
                            ("terrain_types", "terrain_types"), ("terrain_levels", "terrain_levels")):
            setattr(e, field, b[name].data_ptr())
        for field, t in self._const.items():
            setattr(e, field, t.data_ptr())
        e.state, e.table = self.state.data_ptr(), self.table.data_ptr()
        e.trace = self.trace_buf.data_ptr() if self.trace_envs else None
        e.num_envs, e.num_robots, e.num_types, e.num_levels = N, len(self.robot_names), self.num_types, self.num_levels
        e.group_by, e.num_groups = self.mask, self.num_groups
        e.num_trace_envs, e.trace_capacity = len(self.trace_envs), self.trace_capacity
        for k, body in enumerate(env.model.feet_bodies):
            e.feet_bodies[k] = int(body)
        for k, i in enumerate(self.trace_envs):
            e.trace_envs[k] = i
        self._e = e
        self.column_names, self.columns, self.col_table, self._c = (), None, None, None
        self.extra_conventions = {}       # what evaluate() adds to result()["conventions"] (a vision policy's camera_jitter, camera_instrument)
        self.clear()

    def add_columns(self, names):
        """Up to LSIM_EVAL_MAX_COLUMNS named per-env values of the caller's, accumulated per group next to the evaluator's own metrics
        (include/lsim.h, lsim_eval_columns): `.columns` is the [N, len(names)] fp32 device tensor to write before each
        `.accumulate_columns()`, which goes after `.accumulate()` of the same env-step.  Once per evaluator."""
        names = tuple(str(n) for n in names)
        if self._c is not None:
            raise ValueError("add_columns: the evaluator already has columns")
        if not 1 <= len(names) <= MAX_COLUMNS or len(set(names)) != len(names):
            raise ValueError(f"add_columns: 1 to {MAX_COLUMNS} unique names, got {list(names)}")
        for fn in ("lsim_eval_columns_sizes", "lsim_eval_columns_clear", "lsim_eval_columns_accumulate"):
            if not hasattr(self._L, fn):
                raise lib.LsimError(f"the loaded library has no {fn}: rebuild it (there is no torch fall-back for the evaluator's columns)")
        dev, N = self.table.device, int(self.env.num_envs)
        tb = ctypes.c_size_t()
        lib.check(self._L.lsim_eval_columns_sizes(self.num_groups, len(names), ctypes.byref(tb)), what="lsim_eval_columns_sizes")
        self.columns = torch.zeros(N, len(names), dtype=torch.float32, device=dev)
        self.col_table = torch.zeros(self.num_groups, tb.value // 8 // self.num_groups, dtype=torch.int64, device=dev)
        c = abi.LsimEvalColumns()
        c.state, c.reset_buf, c.values, c.table = self.state.data_ptr(), self._e.reset_buf, self.columns.data_ptr(), self.col_table.data_ptr()
        c.num_envs, c.num_groups, c.num_cols, c.ld = N, self.num_groups, len(names), self.columns.stride(0)
        self._c, self.column_names = c, names
        lib.check(self._L.lsim_eval_columns_clear(ctypes.byref(c), self._stream()), what="lsim_eval_columns_clear")
        return self.columns

    def accumulate_columns(self):
        if self._c is None:
            raise ValueError("accumulate_columns: the evaluator has no columns (add_columns)")
        lib.check(self._L.lsim_eval_columns_accumulate(ctypes.byref(self._c), self._stream()), what="lsim_eval_columns_accumulate")

    def _stream(self):
        return self.env._stream()

    def clear(self):
        lib.check(self._L.lsim_eval_clear(ctypes.byref(self._e), self._stream()), what="lsim_eval_clear")
        if self._c is not None:
            lib.check(self._L.lsim_eval_columns_clear(ctypes.byref(self._c), self._stream()), what="lsim_eval_columns_clear")

    def accumulate(self):
        lib.check(self._L.lsim_eval_accumulate(ctypes.byref(self._e), self._stream()), what="lsim_eval_accumulate")

    @property
    def steps(self):
        """launches since clear() (reads the device-side counter: a host sync)"""
        return int(self.state[0].item())

    def result(self):
        """plain dict (JSON-serialisable): `groups` = one entry per group that saw a sample or an episode, `total` = all groups together"""
        table = self.table.cpu().numpy()
        groups = []
        for g in range(self.num_groups):
            if table[g, W["samples"]] or table[g, W["episodes"]] or table[g, W["nonfinite"]]:
                groups.append({"key": group_key(self.mask, self.shape, g, self.robot_names), **metrics_of_row(table[g])})
        env = self.env
        conv = dict(env._conventions()) if hasattr(env, "_conventions") else {"abi_version": int(abi.ABI_VERSION)}
        conv.update({"addend_clamp": CLAMP, "fixed_point_scale": FIX_ONE, "torque_saturation_threshold": SAT_THRESHOLD,
                     "robot_names": self.robot_names, "num_types": self.num_types, "num_levels": self.num_levels})
        total = metrics_of_row(total_row(table))
        if self._c is not None:             # word 0 of a columns row is the main row's `samples`, so the same groups are listed
            ctable = self.col_table.cpu().numpy()
            for grp in groups:
                grp["columns"] = columns_of_row(ctable[key_index(self.mask, self.shape, grp["key"], self.robot_names)], self.column_names)
            total["columns"] = columns_of_row(ctable.sum(axis=0), self.column_names)
            conv["columns"] = list(self.column_names)
        conv.update(self.extra_conventions)
        return {"group_by": [g for g in ("robot", "type", "level") if self.mask & GROUP_BITS[g]], "num_envs": int(env.num_envs), "steps": self.steps,
                "dt": float(env.dt), "groups": groups, "total": total,
                "nonfinite": {"addends": int(table[:, W["nonfinite"]].sum()), "simulator_env_steps": int(env.nonfinite_envs.item())},
                "conventions": conv}

    def trace(self):
        """dict of named numpy arrays [steps kept, trace envs, width], oldest step first, plus "envs" and "step" (launch index of each row)"""
        t, cap = self.steps, self.trace_capacity
        kept = min(t, cap)
        rows = [(s % cap) for s in range(t - kept, t)]
        data = self.trace_buf.cpu().numpy()[rows]
        out = {name: data[:, :, start:start + width] for name, (start, width) in TRACE_COLUMNS.items()}
        out["envs"] = np.asarray(self.trace_envs, dtype=np.int64)
        out["step"] = np.arange(t - kept, t, dtype=np.int64)
        return out


def _policy_sensor(env, parts, device):
    """The sensor a vision or a map policy's rows come from -- the caller's, else the runner's (both in parts.sensor), else
    env.sensors["depth"], else, for a map policy's checkpoint, rebuilt with map and odometry from its record and added to the env as
    "depth" -- with what feeds the actor attached: the map rows, or the encoder and the memory (every capture is followed by their
    launches; the modules of `parts` end up on `device` in eval mode)."""
    ac, cam = parts.actor_critic, parts.sensor if parts.sensor is not None else getattr(env, "sensors", {}).get("depth")
    if parts.kind == "map":
        if cam is None and parts.sensor_record is not None:
            cam = env.add_sensor("depth", sensors.from_spec(env, parts.sensor_record))
        if cam is None or getattr(cam, "map", None) is None:
            raise ValueError("evaluate: a map policy needs a sensor with an elevation map (sensor=..., env.add_sensor('depth', ...), or a checkpoint "
                             "whose 'map_policy' record names one)")
        channels = tuple(parts.channels or getattr(cam, "map_channels", None) or ("height",))
        feet = None
        if channels in sensors.FOOT_CHANNELS:           # the pattern the policy was trained with: the record's, else what the sensor carries
            recorded = (parts.sensor_record or {}).get("foot_scan")
            feet = sensors.FootScan(**recorded) if recorded is not None else getattr(cam, "foot_scan", None) or sensors.FootScan()
        if getattr(cam, "map_channels", None) != channels or getattr(cam, "foot_scan", None) != feet:
            cam.attach_map_rows(channels, foot_scan=feet)
        if cam.map_rows().shape[1] != ac.depth_latent_dim:
            raise ValueError(f"evaluate: the map rows have {cam.map_rows().shape[1]} columns, the actor reads {ac.depth_latent_dim}")
        return cam
    if cam is None or getattr(cam, "model", None) is None:
        raise ValueError("evaluate: a vision policy needs a sensor with a SensorModel (sensor=..., or env.add_sensor('depth', ...))")
    enc, mem = parts.encoder, parts.memory
    if enc is None:
        raise ValueError("evaluate: the checkpoint has no 'vision' record (vision['encoder'], the depth encoder's hyperparameters): "
                         "pass encoder=DepthEncoder(...) with the shapes it was trained with" if parts.checkpoint is not None else
                         "evaluate: a VisionActorCritic needs its depth encoder (encoder=...): nobody else can hand it a latent")
    if enc.latent_dim + (mem.hidden if mem is not None else 0) != ac.depth_latent_dim:
        raise ValueError(f"evaluate: the encoder's latent has {enc.latent_dim} columns" + (f" and the memory {mem.hidden}" if mem is not None else "") +
                         f", the actor reads {ac.depth_latent_dim}")
    for module in (enc, parts.depth_head, mem, parts.memory_head):
        if module is not None:
            module.to(device).eval()
    if getattr(cam, "encoder", None) is not enc:
        cam.attach_encoder(enc)
    if mem is not None and getattr(cam, "memory", None) is not mem:
        cam.attach_memory(mem)
    return cam


def _sensor_option(cam, record, value, cls, key, name, apply):
    """evaluate()'s keyword `name` applied to the sensor's option `key` (the attribute of the sensor and the key of its record alike):
    "trained" -- what `record`, the checkpoint's record of the sensor, says (None -- a runner or a module brings no record: the sensor it
    is given carries what it was trained with, and stays as it is); None -- off; a `cls` -- that one.  `apply(want)` puts a choice that
    differs from what the sensor has in force.  Returns the entry of the result's conventions: the option's record, every value None
    when off, and the choice."""
    current = getattr(cam, key, None)
    if isinstance(value, str):
        if value != "trained":
            raise ValueError(f"evaluate: {name} is 'trained', None or of class {cls.__name__}, got {value!r}")
        want, choice = current if record is None else (cls(**record[key]) if record.get(key) else None), "trained"
    elif value is None:
        want, choice = None, "off"
    elif isinstance(value, cls):
        want, choice = value, "override"
    else:
        raise TypeError(f"evaluate: {name} is 'trained', None or of class {cls.__name__}, got {type(value).__name__}")
    if want != current:
        apply(want)
    return dict(dict.fromkeys(cls.FIELDS) if want is None else want.record(), choice=choice)


def _sensor_options(cam, record, camera_jitter, camera_instrument, odometry, camera_stereo="trained"):
    """the four options of evaluate() in their order -- behind the encoder and the memory, whose launches a refresh() runs too -- as the
    entries of the result's conventions.  A camera whose jitter or instrument changes has every env's mount or row redrawn and history
    refilled once (refresh()); a map whose odometry changes is attached anew: it starts empty, every env's drift at zero, and is filled
    once from the present capture.  A sensor without a map has no odometry entry."""
    def redrawn(setter):
        def apply(want):
            setter(want)
            if cam.tick >= 0:
                cam.refresh()
        return apply

    def reattached(want):
        channels, feet = getattr(cam, "map_channels", None), getattr(cam, "foot_scan", None)
        cam.attach_map(cam.map, odometry=want)
        if channels is not None:
            cam.attach_map_rows(channels, foot_scan=feet)

    out = {"camera_jitter": _sensor_option(cam, record, camera_jitter, sensors.MountJitter, "mount_jitter", "camera_jitter", redrawn(cam.set_mount_jitter)),
           "camera_instrument": _sensor_option(cam, record, camera_instrument, sensors.InstrumentError, "instrument", "camera_instrument", redrawn(cam.set_instrument))}
    out["camera_stereo"] = _sensor_option(cam, record, camera_stereo, sensors.StereoArtifacts, "stereo", "camera_stereo", redrawn(cam.set_stereo))
    if getattr(cam, "map", None) is not None:
        out["odometry"] = _sensor_option(cam, record, odometry, sensors.OdometryError, "odometry", "odometry", reattached)
    return out


def _parse_choice(cls, text):
    """a command-line option of a sensor: "trained", "off" (None), or the text envs.sensors.parse_option takes for a `cls`"""
    if text in ("trained", "off"):
        return "trained" if text == "trained" else None
    if text in ("", "default"):
        raise ValueError(f"expected trained, off or key=value pairs with the keys {', '.join(cls.TEXT)}, got {text!r}")
    return sensors.parse_option(cls, text)


def parse_odometry(text):
    """the command line's --odometry: "trained", "off" (None), or "scale=S,yaw_per_m=Y,z_per_m=Z,noise=a:b:c" (any key may be left out: 0)"""
    return _parse_choice(sensors.OdometryError, text)


def parse_camera_jitter(text):
    """the command line's --camera-jitter: "trained", "off" (None), or "pos=P,rot_deg=R" with P and R one number or three joined by "/"
    (either key may be left out: 0)"""
    return _parse_choice(sensors.MountJitter, text)


def parse_camera_instrument(text):
    """the command line's --camera-instrument: "trained", "off" (None), or "latency=LO:HI,noise_gain=LO:HI,depth_scale=S,depth_quad=Q,fov=F"
    (any key may be left out: the model's latency, gain 1, 0)"""
    return _parse_choice(sensors.InstrumentError, text)


def parse_camera_stereo(text):
    """the command line's --camera-stereo: "trained", "off" (None), or "baseline=B,max_disparity=D,window=W,max_range=R,edge_radius=N,edge_rel=E,
    edge_hole=P,edge_fatten=Q" (any key may be left out: envs.sensors.StereoArtifacts' defaults)"""
    return _parse_choice(sensors.StereoArtifacts, text)


VISION_METRICS = ("depth_influence", "scan_error", "memory_scan_error")
MAP_METRICS = ("map_scan_error", "map_coverage")        # accepted when named and the sensor carries an elevation map; never a default
MAP_FUSION_METRICS = ("map_variance", "map_z2")         # likewise, of a map with a fusion (envs.sensors.MapFusion); dropped without one
MAP_CLEANUP_METRICS = ("map_cleared",)                  # likewise, of a map with a clean-up (envs.sensors.MapCleanup); dropped without one
FOOT_METRICS = ("foot_scan_error", "foot_scan_coverage")       # likewise, of a sensor with foot rows (envs.sensors.FootScan); dropped without them


def _map_fusion_columns(env, cam):
    """{name: fn} of MAP_FUSION_METRICS for a sensor whose map has a fusion, else {}.  "map_variance": the mean of cam.map_variance()
    over the points the map knows; "map_z2": the mean over those points of (map scan - true height)^2 / variance, the truth being
    LSIM_BUF_MEASURED_HEIGHTS moved by the error of the base height the map was given (odometry) -- 1 when the variance is honest.
    An env whose map knows no point reports 0.  map_z2 needs the map's points to be the env's measured ones."""
    if getattr(getattr(cam, "map", None), "fusion", None) is None:
        return {}
    known = lambda: cam.map_known().to(torch.float32)
    over_known = lambda v: (v * known()).sum(dim=1) / known().sum(dim=1).clamp(min=1.0)
    out = {"map_variance": lambda a, a0, live, priv: over_known(cam.map_variance())}
    truth = env.buf.get("measured_heights") if hasattr(env, "buf") else None
    if truth is not None and truth.shape[1] == cam.map_scan().shape[1]:
        def z2(a, a0, live, priv):
            err = cam.map_scan() - (truth + (cam.map_pose()[:, 2:3] - env.root_states[:, 2:3]))
            return over_known(err.square() / cam.map_variance().clamp(min=1e-12))
        out["map_z2"] = z2
    return out


def _map_cleanup_columns(env, cam):
    """{name: fn} of MAP_CLEANUP_METRICS for a sensor whose map has a clean-up, else {}.  "map_cleared": the cells the clean-up forgot
    in this step, per env -- the growth of cam.map_cleared() since the step before (the counter starts again when an env's episode does:
    its value then is what was forgotten since)"""
    if getattr(getattr(cam, "map", None), "cleanup", None) is None:
        return {}
    last = [cam.map_cleared().clone()]

    def cleared(a, a0, live, priv):
        now = cam.map_cleared().clone()
        grown = torch.where(now >= last[0], now - last[0], now).to(torch.float32)
        last[0] = now
        return grown
    return {"map_cleared": cleared}


class FrameWriter:
    """evaluate(frames=...): a shaded chase camera (envs.sensors.chase_camera) on the evaluated env and one PPM per chosen env every
    `every` steps.  {"dir", "every" (default 10), "envs" (default (0,)), "size" (W, H) (default (128, 96)), "shading" (a Shading; None:
    the default one)}; "api": the library the camera launches through (default: the env's).  The camera renders only every g-th env,
    g the greatest common divisor of the chosen envs (one env: that env's multiples; env 0 alone: env 0 only), and is launched only on
    the steps that write: one device-to-host copy per written frame and none otherwise.  finish() also writes `e<env>.gif` per env
    when PIL can be imported."""

    def __init__(self, env, frames):
        unknown = set(frames) - {"dir", "every", "envs", "size", "shading", "api"}
        if unknown or "dir" not in frames:
            raise ValueError(f"evaluate: frames is a dict with 'dir' and optionally 'every', 'envs', 'size', 'shading'; got {sorted(frames)}")
        self.dir, self.every = str(frames["dir"]), int(frames.get("every", 10))
        self.envs = tuple(int(e) for e in frames.get("envs", (0,)))
        W, H = (int(v) for v in frames.get("size", (128, 96)))
        N = int(env.num_envs)
        if self.every < 1 or not self.envs or any(not 0 <= e < N for e in self.envs):
            raise ValueError(f"evaluate: frames needs every >= 1 and envs in [0, {N}), got every={self.every}, envs={self.envs}")
        shading = frames.get("shading")
        stride = math.gcd(*self.envs) or N
        self.cam = sensors.chase_camera(env, W, H, env_stride=stride, api=frames.get("api"), shading=sensors.Shading() if shading is None else shading)
        os.makedirs(self.dir, exist_ok=True)
        self.step, self.written = 0, []

    def after_step(self):
        """called behind env.step_device(): on every `every`-th step launch the camera and write the chosen envs' frames"""
        self.step += 1
        if self.step % self.every:
            return
        self.cam.update()
        rgb = self.cam.rgb_image()
        for e in self.envs:
            img = rgb[e].cpu().numpy()             # the one device-to-host copy of this frame
            path = os.path.join(self.dir, f"e{e}_s{self.step:05d}.ppm")
            sensors.write_ppm(path, img)
            self.written.append((e, path, img))

    def finish(self):
        """the GIFs, when PIL is there; returns what was written: {"frames": [...paths], "gifs": [...paths]}"""
        gifs = []
        try:
            from PIL import Image
        except ImportError:
            Image = None
        for e in (self.envs if Image is not None else ()):
            images = [Image.fromarray(img) for env_id, _, img in self.written if env_id == e]
            if images:
                path = os.path.join(self.dir, f"e{e}.gif")
                images[0].save(path, save_all=True, append_images=images[1:], duration=20 * self.every, loop=0)
                gifs.append(path)
        print(f"evaluate: {len(self.written)} frames (PPM) under {self.dir}" + (f", {len(gifs)} GIF" if gifs else "; no PIL, so no GIF"))
        return {"frames": [p for _, p, _ in self.written], "gifs": gifs}


def _run(env, ac, ev, steps, cmd, fused, packed_cls, rows=None, blind=False, metrics=(), frames=None):
    """evaluate()'s loop, for every kind of policy.  `packed_cls`: the fused launch's class (PackedHimPolicy; PackedVisionPolicy when the
    actor reads more rows), used when the topology allows and `fused` is not False, else act_inference.  `rows()`: the live [N, L] tensor
    the actor also reads (cam.latent, cam.memory_rows, cam.map_rows), zeros in its place when `blind`.  `metrics`: (name, fn) per
    evaluator column, fn(actions, zero_mean, live, priv) -> [N] from the observation the action came from (the step's reset flags decide
    what counts); zero_mean is the action mean over zero rows, one more policy forward per step, made only for a "depth_influence"
    column of a policy that is not blind (None otherwise).  `frames`: a FrameWriter, told of every step behind step_device()."""
    names = tuple(n for n, _ in metrics)
    if names and ev.column_names != names:
        ev.add_columns(names)
    entry = "lsim_policy_forward" if rows is None else "lsim_policy_forward_ext"
    use_fused = packed_cls.supported(ac) if fused is None else bool(fused)
    if use_fused and not packed_cls.supported(ac):
        raise ValueError(f"fused=True but {entry} does not support this policy's topology")
    if hasattr(env, "_external_call"):
        env._external_call()
    dev, N = env.buf["rew"].device, env.num_envs
    influence = "depth_influence" in names and not blind
    zeros = torch.zeros(N, ac.depth_latent_dim, device=dev) if rows is not None else None
    live = mean0 = None
    fed = ()
    if use_fused:
        packed = packed_cls(ac)
        mean, values = torch.empty(N, env.num_actions, device=dev), torch.empty(N, 1, device=dev)
        mean0 = torch.empty(N, env.num_actions, device=dev) if influence else None
    obs, priv = env.get_observations(), env.get_privileged_observations()
    for _ in range(int(steps)):
        if cmd is not None:
            env.commands[:, :3] = cmd
        if rows is not None:
            live = rows()
            fed = (zeros if blind else live,)
        if use_fused:
            packed.forward(obs, priv, mean, values, *fed)
            actions = mean
            if influence:
                packed.forward(obs, priv, mean0, values, zeros)
        else:
            actions = ac.act_inference(obs, *fed)
            if influence:
                mean0 = ac.act_inference(obs, zeros)
        for k, (_, fn) in enumerate(metrics):
            ev.columns[:, k] = fn(actions, mean0, live, priv)
        env.step_device(actions)
        ev.accumulate()
        if metrics:
            ev.accumulate_columns()
        if frames is not None:
            frames.after_step()
    if frames is not None:
        ev.frames_written = frames.finish()
    return ev


def _scan_block(env):
    """(offset, width) of the height scan in the env's privileged observation, or None when it holds none"""
    from .vision import height_scan_block
    try:
        return height_scan_block(env.cfg)
    except ValueError:
        return None


def _influence(blind):
    return lambda actions, zero_mean, live, priv: 0.0 if blind else torch.linalg.vector_norm(actions - zero_mean, dim=1)


def _evaluate_vision(env, ac, ev, steps, cmd, fused, cam, head, blind, metrics, memory=None, memory_head=None, frames=None):
    """evaluate() for a VisionActorCritic: the actor also reads the sensor's live latent rows -- with a memory [z | h] -- and the evaluator
    accumulates the `metrics` as columns (module docstring of learn/vision.py).  A metric whose inputs are
    missing -- its head, the map, a privileged observation that holds the scan, the scan's own points -- is dropped, not zero."""
    from .vision import PackedVisionPolicy
    metrics = list(metrics)
    for m in metrics:
        if m not in VISION_METRICS + MAP_METRICS + MAP_FUSION_METRICS + MAP_CLEANUP_METRICS + FOOT_METRICS:
            raise ValueError(f"unknown vision metric {m!r}: 'depth_influence' or 'scan_error' (with a depth memory also 'memory_scan_error', "
                             f"with an elevation map also 'map_scan_error' and 'map_coverage', with a fused one also 'map_variance' and 'map_z2', with a clean-up also 'map_cleared')")
    has_map = getattr(cam, "map", None) is not None
    scan = _scan_block(env)
    needs = {"map_coverage": has_map, "map_scan_error": has_map and scan is not None and cam.map_scan().shape[1] == scan[1],
             "scan_error": head is not None and scan is not None, "memory_scan_error": memory is not None and memory_head is not None and scan is not None}
    Lz = ac.depth_latent_dim - (memory.hidden if memory is not None else 0)       # the encoder's columns of the actor's depth segment
    target = lambda priv: priv[:, scan[0]:scan[0] + scan[1]]
    columns = {
        "depth_influence": _influence(blind),
        "scan_error": lambda a, a0, live, priv: (head(live[:, :Lz]) - target(priv)).square().mean(dim=1),
        "memory_scan_error": lambda a, a0, live, priv: (memory_head(live[:, Lz:]) - target(priv)).square().mean(dim=1),
        # the map's scan in observation units, exactly as ph_build_obs turns measured_heights into the block, from the height the map has
        "map_scan_error": lambda a, a0, live, priv: ((cam.map_pose()[:, 2:3] - 0.5 - cam.map_scan()).clamp(-1.0, 1.0) * float(env.lcfg.obs_scale_height) - target(priv)).square().mean(dim=1),
        "map_coverage": lambda a, a0, live, priv: cam.map_known().to(torch.float32).mean(dim=1)}
    columns.update(_map_fusion_columns(env, cam))
    columns.update(_map_cleanup_columns(env, cam))
    columns.update(_foot_columns(env, cam, metrics))
    return _run(env, ac, ev, steps, cmd, fused, PackedVisionPolicy, cam.latent if memory is None else cam.memory_rows, blind,
                [(m, columns[m]) for m in metrics if m in columns and needs.get(m, True)], frames=frames)


def _foot_columns(env, cam, metrics):
    """the columns of FOOT_METRICS for a sensor with foot rows ({} without them: the metrics are dropped).  "foot_scan_error": the mean
    square, over the 4K points, of the height block of cam.map_rows() minus the same block of a terrain-source twin (sensors.TerrainFootScan,
    same pattern, z_offset and scale) placed with the TRUE pose -- observation units, so with odometry the placement error of the feet
    and of the map is inside it.  The twin is created only when the metric is named and launched once per step from the column itself;
    it is no sensor of the env.  "foot_scan_coverage": the mean of cam.foot_known()."""
    feet = getattr(cam, "foot_scan", None)
    if feet is None:
        return {}
    columns = {"foot_scan_coverage": lambda a, a0, live, priv: cam.foot_known().to(torch.float32).mean(dim=(1, 2))}
    if "foot_scan_error" in metrics:
        twin, K4 = sensors.TerrainFootScan(env, feet, sensors.FOOT_CHANNELS[0], api=cam._api), 4 * feet.num_points
        columns["foot_scan_error"] = lambda a, a0, live, priv: (cam.map_rows()[:, :K4] - twin.update()[:, :K4]).square().mean(dim=1)
    return columns


def _evaluate_map(env, ac, ev, steps, cmd, fused, cam, blind, metrics, frames=None):
    """evaluate() for a map policy: the actor also reads the sensor's live map rows; of the `metrics` a map policy has "depth_influence"
    (the action distance against zero rows), "map_scan_error" (the rows' height block against the privileged observation's) and
    "map_coverage"; the encoder's and the memory's are dropped"""
    from .vision import PackedVisionPolicy
    P, scan = int(cam.map_scan().shape[1]), _scan_block(env)
    needs = {"map_scan_error": scan is not None and scan[1] == P and getattr(cam, "foot_scan", None) is None}        # foot rows are no scan block
    columns = {
        "depth_influence": _influence(blind),
        "map_scan_error": lambda a, a0, live, priv: (live[:, :P] - priv[:, scan[0]:scan[0] + scan[1]]).square().mean(dim=1),
        "map_coverage": lambda a, a0, live, priv: cam.map_known().to(torch.float32).mean(dim=1)}
    columns.update(_map_fusion_columns(env, cam))
    columns.update(_map_cleanup_columns(env, cam))
    columns.update(_foot_columns(env, cam, metrics))
    return _run(env, ac, ev, steps, cmd, fused, PackedVisionPolicy, cam.map_rows, blind,
                [(m, columns[m]) for m in metrics if m in columns and needs.get(m, True)], frames=frames)


def _evaluate_scan(env, ac, ev, steps, cmd, fused, record, blind, metrics, explicit, frames=None):
    """evaluate() for a scan policy (learn/scan_policy.py): the actor also reads the scan block of the live privileged observation --
    a column-slice view, so the fused launch takes it with ld = num_priv_obs and nothing is copied.  Only the base columns are reported:
    there is no sensor, encoder or map to measure, so vision metrics that were NAMED are refused."""
    from .vision import PackedVisionPolicy, height_scan_block
    if explicit and metrics:
        raise ValueError(f"evaluate: a scan policy reads the privileged height scan itself -- it has no sensor, encoder or map, so no vision "
                         f"metrics; got {tuple(metrics)} (pass vision_metrics=())")
    if record.get("foot_scan") is not None:         # the teacher on true foot scans: its rows are a TerrainFootScan's, rebuilt from the record
        feet, channels = sensors.FootScan(**record["foot_scan"]), tuple(record.get("channels") or sensors.FOOT_CHANNELS[0])
        have = env.sensors.get("foot_scan")
        if have is None:
            have = env.add_sensor("foot_scan", sensors.TerrainFootScan(env, feet, channels))
        elif not isinstance(have, sensors.TerrainFootScan) or have.foot_scan != feet or have.channels != channels:
            raise ValueError("evaluate: env.sensors['foot_scan'] is not the TerrainFootScan the scan policy's record names")
        if have.rows().shape[1] != ac.depth_latent_dim:
            raise ValueError(f"evaluate: the foot rows have {have.rows().shape[1]} columns, the actor reads {ac.depth_latent_dim}")
        return _run(env, ac, ev, steps, cmd, fused, PackedVisionPolicy, have.rows, blind, frames=frames)
    off, width = height_scan_block(env.cfg)
    if (int(record.get("offset", off)), int(record.get("width", width))) != (off, width) or width != ac.depth_latent_dim:
        raise ValueError(f"evaluate: the scan policy read the block {record}, the env's is offset {off}, width {width}; the actor reads {ac.depth_latent_dim}")
    priv = env.get_privileged_observations()
    return _run(env, ac, ev, steps, cmd, fused, PackedVisionPolicy, lambda: priv[:, off:off + width], blind, frames=frames)


@torch.no_grad()
def evaluate(env, policy, steps, commands=None, group_by=("robot", "type", "level"), trace_envs=(), trace_capacity=None, fused=None, evaluator=None,
             sensor=None, encoder=None, depth_head=None, blind=False, vision_metrics=VISION_METRICS, camera_jitter="trained",
             camera_instrument="trained", odometry="trained", camera_stereo="trained", frames=None):
    """The loop of play.py:124-133 on the device: per step write the commands (when given: (vx, vy, yaw) or a tensor [N, 3]), take the MEAN
    action (fused lsim_policy_forward when the topology allows and `fused` is not False, HIMActorCritic.act_inference otherwise), step, accumulate.
    No host synchronisation inside the loop.  Returns the Evaluator (`.result()`, `.trace()`).
    A vision policy (a VisionActorCritic, a VisionOnPolicyRunner, or a checkpoint of one) also reads the latent of `sensor` (default: the
    runner's, else env.sensors["depth"]) through `encoder` (default: the runner's, else rebuilt from the checkpoint's `vision` record);
    `blind=True` feeds zeros instead.  `vision_metrics` become columns of the result: "depth_influence" = the L2 distance of the action
    mean from the mean with a zero latent (one more policy forward per step), "scan_error" = the mean square error of `depth_head` (the
    encoder's auxiliary head) against the height scan of the privileged observation; a metric whose inputs are missing is dropped.
    A policy trained with a depth memory (the runner's alg.memory, or the memory record of the checkpoint) gets the memory rebuilt and
    attached behind the encoder and reads cam.memory_rows(), [z | h]; "memory_scan_error" is the memory head's error on h.
    With an elevation map on the sensor (envs.sensors.ElevationMap, cam.attach_map) two more metrics are accepted when NAMED (they are in
    no default): "map_scan_error" = the mean square, over the scan points, of the map's scan in observation units
    (clip(base z - 0.5 - h, -1, 1) * obs_scales.height_measurements, as csrc/ls_post.h builds the block) minus the height scan of the
    privileged observation -- the same units as scan_error and memory_scan_error -- and "map_coverage" = the mean of cam.map_known().
    `camera_jitter` (a vision policy only): the per-episode mount error of the camera (envs.sensors.MountJitter) -- "trained": what the
    checkpoint's record of the sensor says (a runner's camera stays as it is); None: the nominal mount; a MountJitter: that one, to
    measure robustness beyond the trained range.  The choice and the ranges in force are written to the result's conventions["camera_jitter"].
    `camera_instrument` (a vision policy only): the same choice for the per-episode error of the camera's own constants
    (envs.sensors.InstrumentError: latency, noise gain, depth-scale error, field of view), written to conventions["camera_instrument"].
    `camera_stereo` (likewise): the same choice for the stereo pair's artefacts -- occlusion shadows, minimum range, depth-edge holes and
    fattening (envs.sensors.StereoArtifacts) --, written to conventions["camera_stereo"].
    A map policy (a MapOnPolicyRunner, its checkpoint -- from whose record sensor, map and rows are rebuilt when the env has none -- or a
    bare module that learn/policy_io.py's policy_parts takes for one) reads cam.map_rows(); `blind=True` feeds zeros; "depth_influence" is
    the action distance against zero rows and "map_scan_error" the mean square of the rows' height block minus the privileged one.
    `odometry` (a sensor with an elevation map only): the dead-reckoning error of the pose the map is placed with
    (envs.sensors.OdometryError) -- "trained", None or an OdometryError, as camera_jitter; written to conventions["odometry"].  With
    odometry map_scan_error uses the ESTIMATED base height, the one the map has.
    With foot rows on the sensor (cam.attach_map_rows(("foot_height",), foot_scan=FootScan()); a map policy trained on them has them
    rebuilt from its record) two more metrics are accepted when NAMED: "foot_scan_error" = the mean square of the rows' height block minus
    the same block sampled from the true terrain at the true pose (_foot_columns), and "foot_scan_coverage" = the mean of cam.foot_known();
    "map_scan_error" is dropped for such a policy.  A scan policy trained on true foot scans (ScanOnPolicyRunner(foot_scan=...)) reads a
    sensors.TerrainFootScan rebuilt from its record.
    A scan policy (a ScanOnPolicyRunner or its checkpoint) reads the scan block of the live privileged observation; `blind=True` feeds
    zeros; only the base columns are reported and `vision_metrics` other than the default or an empty tuple are refused: no camera to measure.
    `frames` (None: nothing of this is allocated, launched or written): {"dir": ..., "every": K, "envs": (...), "size": (W, H), "shading":
    Shading | None} -- what a person watches (FrameWriter): a shaded chase camera (envs.sensors.chase_camera, lsim_sensor_shade) follows
    the chosen envs and `dir/e<env>_s<step>.ppm` is written every K steps, plus one `e<env>.gif` per env at the end when PIL can be
    imported; the Evaluator's `frames_written` lists the files.  The result is the one without frames."""
    from .fused_policy import PackedHimPolicy
    dev = env.buf["rew"].device
    parts = policy_parts(env, policy, dev, sensor=sensor, encoder=encoder, depth_head=depth_head)      # the caller's own parts come first
    ac, kind = parts.actor_critic.eval(), parts.kind
    if kind in ("vision", "map"):
        cam = _policy_sensor(env, parts, dev)
        # a checkpoint's record of the sensor; a runner's or a module's sensor carries what it was trained with, and stays as it is
        record = parts.sensor_record if parts.checkpoint is not None else None
        conventions = _sensor_options(cam, record, camera_jitter, camera_instrument, odometry, camera_stereo)
    ev = evaluator or Evaluator(env, group_by, trace_envs, trace_capacity if trace_capacity is not None else max(int(steps), 1))
    frames = None if frames is None else FrameWriter(env, frames)
    cmd = None
    if commands is not None:
        cmd = torch.as_tensor(commands, dtype=torch.float32, device=dev)
        cmd = cmd.expand(env.num_envs, 3).contiguous() if cmd.dim() == 1 else cmd.contiguous()
        if tuple(cmd.shape) != (env.num_envs, 3):
            raise ValueError(f"commands must be (vx, vy, yaw) or [num_envs, 3], got shape {tuple(cmd.shape)}")
    if kind == "him":
        return _run(env, ac, ev, steps, cmd, fused, PackedHimPolicy, frames=frames)
    if kind == "scan":
        return _evaluate_scan(env, ac, ev, steps, cmd, fused, parts.scan, bool(blind), tuple(vision_metrics or ()),
                              explicit=vision_metrics is not VISION_METRICS, frames=frames)
    ev.extra_conventions.update(conventions)
    if kind == "map":
        return _evaluate_map(env, ac, ev, steps, cmd, fused, cam, bool(blind), tuple(vision_metrics or ()), frames=frames)
    return _evaluate_vision(env, ac, ev, steps, cmd, fused, cam, parts.depth_head, bool(blind), tuple(vision_metrics or ()),
                            memory=parts.memory, memory_head=parts.memory_head, frames=frames)


def format_table(result):
    cols = ("samples", "episodes", "fall_rate", "lin_vel_error_rms", "yaw_rate_error_rms", "mechanical_power_mean", "torque_saturation_rate",
            "episode_return_mean", "episode_length_mean", "episode_distance_mean")
    extra = tuple(result["total"].get("columns", ()))          # the caller's columns (Evaluator.add_columns): their means, after the fixed ones
    lines = [" ".join([f"{'group':<28}"] + [f"{c[:14]:>14}" for c in cols + extra])]
    for g in result["groups"] + [{"key": {"all": ""}, **result["total"]}]:
        name = " ".join(f"{k}={v}" if v != "" else k for k, v in g["key"].items()) or "all"
        lines.append(" ".join([f"{name:<28}"] + [f"{g[c]:>14d}" if isinstance(g[c], int) else f"{g[c]:>14.4f}" for c in cols] +
                              [f"{g['columns'][c]['mean']:>14.6f}" for c in extra]))
    return "\n".join(lines)


def parse_args(argv=None):
    """the command line; argument errors raise SystemExit through argparse"""
    ap = argparse.ArgumentParser(prog="python -m isaacgymloco_amd.learn.evaluate", description=__doc__.split("\n")[0])
    ap.add_argument("--task", required=True, choices=sorted(C.TASKS))
    ap.add_argument("--robots", default=None, help="name=fraction,... (a mixed instance, config.mixed_cfg)")
    ap.add_argument("--checkpoint", required=True, help="file written by runner.save")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--commands", default="1.0,0,0", help="vx,vy,yaw written every step; 'env' keeps the env's own sampled commands")
    ap.add_argument("--group-by", default="robot,type,level")
    ap.add_argument("--no-terminations", action="store_true", help="empty terminate_after_contacts_on as the reference's play.py does")
    ap.add_argument("--out", required=True)
    ap.add_argument("--trace-envs", default="")
    ap.add_argument("--trace-out", default=None)
    ap.add_argument("--blind", action="store_true", help="a vision policy acts on a zero latent instead of its camera's")
    ap.add_argument("--vision-metrics", default="depth_influence,scan_error",
                    help="columns a vision policy adds to the result; empty: none.  A column whose inputs are missing is dropped, not zero: map_variance and "
                         "map_z2 need a map with a fusion, and map_z2 also a map sampled at the env's own measured points (LSIM_BUF_MEASURED_HEIGHTS is its truth)")
    ap.add_argument("--camera-jitter", default="trained", help="a vision policy's per-episode camera mount error: 'trained' (the checkpoint's record), "
                    "'off' (the nominal mount) or pos=METRES,rot_deg=DEGREES (one number, or x/y/z)")
    ap.add_argument("--camera-instrument", default="trained", help="a vision policy's per-episode error of the camera's own constants: 'trained' (the "
                    "checkpoint's record), 'off' or latency=LO:HI,noise_gain=LO:HI,depth_scale=S,depth_quad=Q,fov=F (any subset)")
    ap.add_argument("--camera-stereo", default="trained", help="a vision policy's stereo artefacts (occlusion shadows, depth-edge holes and fattening): "
                    "'trained' (the checkpoint's record), 'off' or baseline=B,max_disparity=D,window=W,max_range=R,edge_radius=N,edge_rel=E,edge_hole=P,edge_fatten=Q (any subset)")
    ap.add_argument("--odometry", default="trained", help="the dead-reckoning error of the pose an elevation map is placed with: 'trained' (the "
                    "checkpoint's record), 'off' or scale=S,yaw_per_m=Y,z_per_m=Z,noise=a:b:c (any subset)")
    ap.add_argument("--frames", default=None, metavar="DIR", help="write shaded chase-camera frames of the chosen envs here: e<env>_s<step>.ppm, and e<env>.gif when PIL is there")
    ap.add_argument("--frames-every", type=int, default=10, help="a frame every K steps")
    ap.add_argument("--frames-envs", default="0", help="the envs to follow, e.g. 0,7")
    ap.add_argument("--frames-size", default="128x96", help="WIDTHxHEIGHT, at most LSIM_RAYCAST_MAX_RAYS pixels")
    ap.add_argument("--frames-shading", default="default", help="sun=AZ:EL,ambient=A,shadows=0|1,checker=M,checker_gain=G,shadow_bias=B,shadow_far=F (any subset)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if a.frames is not None:
        try:
            size = tuple(int(v) for v in a.frames_size.lower().split("x"))
            if len(size) != 2:
                raise ValueError(f"--frames-size takes WIDTHxHEIGHT, got {a.frames_size!r}")
            a.frames = {"dir": a.frames, "every": a.frames_every, "envs": tuple(int(v) for v in a.frames_envs.split(",") if v), "size": size,
                        "shading": sensors.parse_shading(a.frames_shading)}
        except ValueError as exc:
            ap.error(f"--frames: {exc}")
    for name, parse in (("camera_instrument", parse_camera_instrument), ("odometry", parse_odometry), ("camera_jitter", parse_camera_jitter),
                        ("camera_stereo", parse_camera_stereo)):
        try:
            setattr(a, name, parse(getattr(a, name)))
        except ValueError as exc:
            ap.error(f"--{name.replace('_', '-')}: {exc}")
    if a.envs < 1 or a.steps < 1:
        ap.error("--envs and --steps must be positive")
    if a.commands == "env":
        a.commands = None
    else:
        try:
            a.commands = tuple(float(v) for v in a.commands.split(","))
        except ValueError:
            ap.error(f"--commands: not numbers: {a.commands!r}")
        if len(a.commands) != 3:
            ap.error("--commands takes vx,vy,yaw")
    a.group_by = tuple(g for g in a.group_by.split(",") if g)
    a.vision_metrics = tuple(m for m in a.vision_metrics.split(",") if m)
    if any(m not in VISION_METRICS + MAP_METRICS + MAP_FUSION_METRICS + MAP_CLEANUP_METRICS + FOOT_METRICS for m in a.vision_metrics):
        ap.error(f"--vision-metrics: 'depth_influence', 'scan_error', 'memory_scan_error', 'map_scan_error' and / or 'map_coverage', got {a.vision_metrics}"
                 " (a map with a fusion also has 'map_variance' and 'map_z2', one with a clean-up 'map_cleared', a sensor with foot rows 'foot_scan_error' and 'foot_scan_coverage')")
    try:
        group_mask(a.group_by)
    except ValueError as exc:
        ap.error(str(exc))
    try:
        a.trace_envs = tuple(int(v) for v in a.trace_envs.split(",") if v)
    except ValueError:
        ap.error(f"--trace-envs: not integers: {a.trace_envs!r}")
    if len(a.trace_envs) > MAX_TRACE_ENVS or any(not 0 <= i < a.envs for i in a.trace_envs):
        ap.error(f"--trace-envs: at most {MAX_TRACE_ENVS} envs, each in [0, --envs)")
    if bool(a.trace_envs) != bool(a.trace_out):
        ap.error("--trace-envs and --trace-out go together")
    if a.robots is not None:
        try:
            a.robots = {k: float(v) for k, v in (item.split("=") for item in a.robots.split(","))}
        except ValueError:
            ap.error(f"--robots: expected name=fraction,..., got {a.robots!r}")
    return a


def main(argv=None):
    a = parse_args(argv)
    from ..envs.legged_robot import LeggedRobot
    cfg = C.mixed_cfg(a.task, a.robots)[0] if a.robots else C.TASKS[a.task][0]()
    cfg = play_cfg(cfg, keep_terminations=not a.no_terminations)
    cfg.env.num_envs = a.envs
    env = LeggedRobot(cfg, sim_device=a.device, seed=a.seed)
    env.reset()
    kind, record = policy_record(torch.load(a.checkpoint, map_location="cpu", weights_only=False))
    if record.get("sensor") is not None:       # a vision or a map policy's checkpoint names the camera it was trained with
        env.add_sensor("depth", sensors.from_spec(env, record["sensor"]))
    named = any(str(v).startswith("--vision-metrics") for v in (sys.argv[1:] if argv is None else argv))
    if kind == "scan" and not named:       # a scan policy has no vision metrics: the option's default means none, a named one is refused
        a.vision_metrics = ()
    ev = evaluate(env, a.checkpoint, a.steps, commands=a.commands, group_by=a.group_by, trace_envs=a.trace_envs, blind=a.blind,
                  vision_metrics=a.vision_metrics, camera_jitter=a.camera_jitter, camera_instrument=a.camera_instrument, odometry=a.odometry,
                  camera_stereo=a.camera_stereo, frames=a.frames)
    res = ev.result()
    print(format_table(res))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    if a.trace_out:
        np.savez(a.trace_out, **ev.trace())
    return 0


if __name__ == "__main__":
    sys.exit(main())
