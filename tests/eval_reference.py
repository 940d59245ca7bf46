"""TEST INFRASTRUCTURE -- the evaluator's semantics (include/lsim.h, "policy evaluation on the device") restated in float64 / exact integers with
numpy, written from that text and not from the kernel.  `RefEvaluator.step(bufs)` consumes one env-step's buffers (numpy arrays named as in
lsim_eval); `.table` is the int64 table the device must reproduce: count words exactly, fixed-point words within `.bound()`.

Next to every fixed-point word the reference keeps what the error bound needs: the number of addends and the sum of their magnitudes.  A sample
is formed on the device in fp32 from at most 2 * 12 + 4 operations (12 products, 12 additions, a difference / square / root / quotient), each
with relative error <= 2^-24 of a partial result no larger than the final sum of the (non-negative) terms, and converted with error <= 2^-33:
    |device - reference| <= 32 * 2^-24 * sum|addends| + addends * 2^-32        (in units of the value; times 2^32 in units of the word)
"""
import numpy as np

W = {n: i for i, n in enumerate(
    ["samples", "lin_err", "lin_err_sq", "yaw_err", "yaw_err_sq", "power", "torque_sq", "action_rate", "feet_contact", "torque_sat",
     "peak_torque_ratio", "episodes", "time_outs", "falls", "return", "length", "distance", "nonfinite"])}
COUNT_WORDS = ("samples", "feet_contact", "torque_sat", "episodes", "time_outs", "falls", "length", "nonfinite")
EXACT_WORDS = COUNT_WORDS + ("return",)      # the return is an integer sum of exactly converted fp32 rewards
FIX_WORDS = tuple(n for n in W if n not in EXACT_WORDS)
BY_ROBOT, BY_TYPE, BY_LEVEL = 1, 2, 4
CLAMP = float(2 ** 20)
TRACE_COLS = {"dof_pos_target": (0, 12), "dof_pos": (12, 24), "dof_vel": (24, 36), "torques": (36, 48), "commands": (48, 51), "base_lin_vel": (51, 54),
              "base_ang_vel": (54, 57), "contact_forces_z": (57, 61), "root_pos": (61, 64), "root_quat": (64, 68), "rew": (68, 69), "reset": (69, 70)}


def fix(v):
    """float64 array -> int64 words: round-half-even(clamp(v, +-2^20) * 2^32); callers mask non-finite values out first"""
    return np.rint(np.clip(v, -CLAMP, CLAMP) * 2.0 ** 32).astype(np.int64)


class RefEvaluator:
    def __init__(self, num_envs, num_robots, num_types, num_levels, group_by, robot_ids=None):
        self.N, self.R, self.T, self.L, self.by = num_envs, num_robots, num_types, num_levels, group_by
        self.robot_ids = None if robot_ids is None else np.asarray(robot_ids).astype(np.int64)
        self.num_groups = (num_robots if group_by & BY_ROBOT else 1) * (num_types if group_by & BY_TYPE else 1) * (num_levels if group_by & BY_LEVEL else 1)
        self.table = np.zeros((self.num_groups, len(W)), np.int64)
        self.mag = np.zeros((self.num_groups, len(W)), np.float64)      # sum of |addend| per fixed-point word
        self.cnt = np.zeros((self.num_groups, len(W)), np.int64)        # number of addends per fixed-point word
        self.group = np.full(num_envs, -1, np.int64)
        self.ret = np.zeros(num_envs, np.int64)
        self.length = np.zeros(num_envs, np.int64)
        self.start = np.zeros((num_envs, 2)); self.last = np.zeros((num_envs, 2))

    def _groups_now(self, b):
        r = np.clip(self.robot_ids, 0, self.R - 1) if (self.by & BY_ROBOT and self.robot_ids is not None) else np.zeros(self.N, np.int64)
        nt, nl = (self.T if self.by & BY_TYPE else 1), (self.L if self.by & BY_LEVEL else 1)
        t = np.clip(b["terrain_types"].astype(np.int64), 0, nt - 1)
        l = np.clip(b["terrain_levels"].astype(np.int64), 0, nl - 1)
        return (r * nt + t) * nl + l

    def _add(self, word, env_mask, values):
        """values: float64 [N]; adds the finite ones of the masked envs to their groups, counts the others as non-finite"""
        k = W[word]
        ok = env_mask & np.isfinite(values)
        bad = env_mask & ~np.isfinite(values)
        v = np.where(ok, values, 0.0)
        if word == "peak_torque_ratio":
            np.maximum.at(self.table[:, k], self.group[ok], fix(v[ok]))
            np.maximum.at(self.mag[:, k], self.group[ok], np.minimum(np.abs(v[ok]), CLAMP))
            self.cnt[:, k] = 1
        else:
            np.add.at(self.table[:, k], self.group[ok], fix(v[ok]))
            np.add.at(self.mag[:, k], self.group[ok], np.minimum(np.abs(v[ok]), CLAMP))
            np.add.at(self.cnt[:, k], self.group[ok], 1)
        np.add.at(self.table[:, W["nonfinite"]], self.group[bad], 1)

    def _count(self, word, env_mask, values):
        np.add.at(self.table[:, W[word]], self.group[env_mask], np.asarray(values, np.int64)[env_mask])

    def step(self, b):
        f8 = lambda name: b[name].astype(np.float64)
        reset, tout = b["reset_buf"].astype(bool), b["time_out_buf"].astype(bool)
        xy = f8("root_states")[:, 0:2]
        new = self.group < 0
        now = self._groups_now(b)
        self.group[new] = now[new]
        self.start[new] = xy[new]; self.last[new] = xy[new]
        rew = f8("rew")
        okr = np.isfinite(rew)
        self.ret += np.where(okr, fix(np.where(okr, rew, 0.0)), 0)
        np.add.at(self.table[:, W["nonfinite"]], self.group[~okr], 1)
        self.length += 1
        live = ~reset
        ones = np.ones(self.N, np.int64)
        # ---- step sample
        cmd, blv, bav = f8("commands"), f8("base_lin_vel"), f8("base_ang_vel")
        tau, qd = f8("torques"), f8("dof_state").reshape(self.N, 12, 2)[:, :, 1]
        lim32 = b["torque_limits"].astype(np.float32)
        with np.errstate(all="ignore"):
            e2 = (cmd[:, 0] - blv[:, 0]) ** 2 + (cmd[:, 1] - blv[:, 1]) ** 2
            yaw = np.abs(cmd[:, 2] - bav[:, 2])
            power = np.abs(tau * qd).sum(1)
            tsq = (tau * tau).sum(1)
            rate = ((f8("actions") - f8("last_actions")) ** 2).sum(1)
            ratio = np.abs(tau) / lim32.astype(np.float64)
            peak = np.where(np.isnan(ratio).any(1), np.nan, np.nan_to_num(ratio, nan=0.0).max(1))
            sat = (np.abs(b["torques"].astype(np.float32)) >= np.float32(0.98) * lim32).sum(1)      # the threshold is an fp32 product by definition
        self._count("samples", live, ones)
        self._add("lin_err", live, np.sqrt(e2)); self._add("lin_err_sq", live, e2)
        self._add("yaw_err", live, yaw); self._add("yaw_err_sq", live, yaw * yaw)
        self._add("power", live, power); self._add("torque_sq", live, tsq); self._add("action_rate", live, rate)
        self._count("feet_contact", live, (b["contact_filt"].reshape(self.N, 4) != 0).sum(1))
        self._count("torque_sat", live, sat)
        self._add("peak_torque_ratio", live, peak)
        self.last[live] = xy[live]
        # ---- episode record
        self._count("episodes", reset, ones); self._count("time_outs", reset, tout); self._count("falls", reset, ~tout)
        self._count("return", reset, self.ret); self._count("length", reset, self.length)
        self._add("distance", reset, np.sqrt(((self.last - self.start) ** 2).sum(1)))
        self.ret[reset] = 0; self.length[reset] = 0
        self.group[reset] = now[reset]
        self.start[reset] = xy[reset]; self.last[reset] = xy[reset]

    def bound(self):
        """int64-word bound per (group, word) on |device - reference| (module docstring); 0 for the exact words"""
        bd = (32.0 * 2.0 ** -24 * self.mag + self.cnt * 2.0 ** -32) * 2.0 ** 32
        for n in EXACT_WORDS:
            bd[:, W[n]] = 0
        return np.ceil(bd)


def trace_row(b, env, feet_bodies, action_scale, default_dof_pos):
    """the LSIM_EVAL_TRACE_DIM columns of one env from one step's buffers; dof_pos_target in float64 (the device rounds it to fp32: <= 1 ulp)"""
    N = b["rew"].shape[0]
    d = b["dof_state"].reshape(N, 12, 2)
    cf = b["contact_forces"].reshape(N, 17, 3)
    return np.concatenate([
        b["actions"][env].astype(np.float64) * action_scale[env].astype(np.float64) + default_dof_pos[env].astype(np.float64),
        d[env, :, 0], d[env, :, 1], b["torques"][env], b["commands"][env, :3], b["base_lin_vel"][env], b["base_ang_vel"][env],
        cf[env, list(feet_bodies), 2], b["root_states"][env, 0:3], b["root_states"][env, 3:7], [b["rew"][env]], [1.0 if b["reset_buf"][env] else 0.0]]).astype(np.float64)
