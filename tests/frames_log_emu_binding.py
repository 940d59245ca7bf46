"""TEST INFRASTRUCTURE -- builds and binds tests/emu/emu_frames_log.cpp (the CPU shim of the two entry points of
isaacgymloco_amd/csrc/ls_frames_log.h compiled by g++ under LS_EMU), and their rigs: one struct with the arrays it points to, in host memory
for the shim or in device memory for the HIP library, driven call by call.  Every array a call writes has guard elements behind it,
pre-filled and checked.  The checks both tests/test_frames_log.py (shim) and tests/test_gpu_frames_log.py (device) run are here too."""
import numpy as np

import emu_binding
import frames_log_reference as R
from helpers import abi
from launch_rig import EditRig, LaunchRig

LOG_FILL, INT_FILL = np.float32(-7.25), -99
LsimFramesLog = abi.STRUCTS["lsim_frames_log_t"]
LsimLatentRowsGrad = abi.STRUCTS["lsim_latent_rows_grad_t"]
assert (R.FILL_ALL, R.RESETS_ONLY) == (abi.DEFINES["LSIM_SENSOR_FILL_ALL"], abi.DEFINES["LSIM_SENSOR_RESETS_ONLY"])
assert (R.COUNT, R.OVERFLOW, R.BASE, R.NEXT) == tuple(abi.DEFINES["LSIM_FRAMES_LOG_" + k] for k in ("COUNT", "OVERFLOW", "BASE", "NEXT"))


def lib():
    return emu_binding.shim("frames_log")


def EmuApi():
    """the sensor, encoder and memory shims plus this one, for envs.sensors.RaySensor(api=...)"""
    return emu_binding.api("raycast", "raycast_bodies", "sensor_model", "depth_encoder", "depth_memory", "frames_log")


class Rig(LaunchRig):
    """the arrays of one frame log for N envs: hist [N, slots, stride] and episode_length are inputs a call replaces; log, row_of, row_src
    and state are outputs, pre-filled as frames_log_reference.FramesLog pre-fills its own, each with guard elements behind it.
    `device`: None -- numpy arrays and the shim -- or a torch device and `entry` = the library's lsim_sensor_frames_log."""

    def __init__(self, N, capacity, pixels=R.PIXELS, env_stride=1, device=None, entry=None):
        super().__init__(device)
        self.N, self.capacity, self.pixels = int(N), int(capacity), int(pixels)
        self.add("hist", np.zeros((N, R.SLOTS, R.HIST_STRIDE), np.float32))
        self.add("episode_length", np.zeros(N, np.int64))
        self.add("log", np.full((capacity, R.FRAMES, R.ROW_STRIDE), LOG_FILL, np.float32), guard=LOG_FILL)
        self.add("row_of", np.full((R.STEPS, N), INT_FILL, np.int32), guard=INT_FILL)
        self.add("row_src", np.full(capacity, INT_FILL, np.int32), guard=INT_FILL)
        self.add("state", np.zeros(4, np.int32), guard=INT_FILL)
        fl = LsimFramesLog()
        self.point(fl, ("hist", "episode_length", "log", "row_of", "row_src", "state"))
        fl.hist_stride, fl.hist_slots, fl.num_envs, fl.env_stride = R.HIST_STRIDE, R.SLOTS, self.N, int(env_stride)
        fl.frames, fl.pixels, fl.row_stride, fl.num_steps, fl.capacity = R.FRAMES, self.pixels, R.ROW_STRIDE, R.STEPS, self.capacity
        fl.period, fl.stagger = R.PERIOD, 1
        self.fl = self.bind(fl, entry if device is not None else lib().emu_sensor_frames_log)

    def launch(self, hist, episode_length, tick, step, flags, edit=None, stream=None):
        """one call on new inputs; `edit(fl)` changes a copy of the struct first; returns the entry point's value"""
        self.put("hist", hist)
        self.put("episode_length", episode_length)

        def edits(fl):
            fl.step = int(step)
            if edit:
                edit(fl)
        return super().launch(int(tick), int(flags), edits, stream)

    def outputs_raw(self):
        """copies of the four outputs, guards included"""
        return {k: self.raw(k) for k in ("log", "row_of", "row_src", "state")}

    def read(self):
        """(log [capacity, frames, row_stride], row_of [T, N], row_src [capacity], state [4]); asserts the four guards intact"""
        self.assert_guards()
        return tuple(self.get(k) for k in ("log", "row_of", "row_src", "state"))


def check_scenario(make_rig, N, pixels=R.PIXELS):
    """the scenario of frames_log_reference on a rig against the state machine, all four outputs exactly equal after EVERY call"""
    capacity = R.scenario_capacity(N)
    rig = make_rig(N, capacity, pixels=pixels)
    ref = R.FramesLog(N, R.STEPS, capacity, R.FRAMES, pixels, R.ROW_STRIDE, R.PERIOD, 1, log_fill=LOG_FILL, int_fill=INT_FILL)
    calls = R.launches(N)
    assert sum(1 for c in calls if c[4] == R.RESETS_ONLY) == 1
    for i, call in enumerate(calls):
        before_last = int(ref.state[R.COUNT]), int(ref.state[R.OVERFLOW])
        ref.launch(*call)
        assert rig.launch(*call) == 0
        log, row_of, row_src, state = rig.read()
        what = f"N {N} call {i} (step {call[3]}, flags {call[4]})"
        assert np.array_equal(state, ref.state), (what, state, ref.state)
        assert np.array_equal(row_of, ref.row_of), what
        assert np.array_equal(row_src, ref.row_src), what
        assert np.array_equal(log.view(np.uint32), ref.log.view(np.uint32)), what
        count = int(state[R.COUNT])
        assert (log[count:] == LOG_FILL).all() and (row_src[count:] == INT_FILL).all(), what + ": a row at or above count was written"
    if N == 8:      # the capacity is three short, and only the last step found that out
        assert before_last == (capacity - (R.run_reference(N, 10 ** 6)[1][-1] - 3), 0) and tuple(ref.state[:2]) == (capacity, 3)
        assert (ref.row_of[-1] == -1).sum() == 3
    else:           # the default capacity is never reached
        assert capacity == R.default_capacity(N, R.STEPS, R.PERIOD) and ref.state[R.COUNT] < capacity and ref.state[R.OVERFLOW] == 0
        assert (ref.row_of >= 0).all()
    return rig, ref


def _bad_pointer(name, off):
    def edit(s):
        setattr(s, name, (getattr(s, name) or 0) + off if off else None)
    return edit


def _set(**kw):
    def edit(s):
        for k, v in kw.items():
            setattr(s, k, v)
    return edit


FRAMES_LOG_REFUSALS = {
    **{f"{n} NULL": _bad_pointer(n, 0) for n in ("hist", "episode_length", "log", "row_of", "row_src", "state")},
    "hist misaligned": _bad_pointer("hist", 4), "log misaligned": _bad_pointer("log", 4), "episode_length misaligned": _bad_pointer("episode_length", 4),
    "row_of misaligned": _bad_pointer("row_of", 2), "row_src misaligned": _bad_pointer("row_src", 2), "state misaligned": _bad_pointer("state", 2),
    "num_envs 0": _set(num_envs=0), "env_stride 0": _set(env_stride=0), "frames 0": _set(frames=0), "pixels 0": _set(pixels=0),
    "frames > hist_slots": _set(frames=R.SLOTS + 1), "hist_slots > MAX_HISTORY": _set(hist_slots=abi.DEFINES["LSIM_SENSOR_MAX_HISTORY"] + 1),
    "pixels > hist_stride": _set(pixels=R.HIST_STRIDE + 1, row_stride=R.HIST_STRIDE + 4), "hist_stride % 4": _set(hist_stride=R.HIST_STRIDE + 2),
    "row_stride < pixels": _set(row_stride=R.PIXELS - 4), "row_stride % 4": _set(row_stride=R.ROW_STRIDE + 2),
    "num_steps 0": _set(num_steps=0), "step < 0": _set(step=-1), "step == num_steps": _set(step=R.STEPS), "capacity 0": _set(capacity=0),
    "step 0 without FILL_ALL": _set(step=0, flags=0), "step 0 with RESETS_ONLY": _set(step=0, flags=R.RESETS_ONLY),
    "num_steps * num_envs >= 2^31": _set(num_steps=2 ** 30),
    "tick < 0": _set(tick=-1), "period 0": _set(period=0), "stagger 2": _set(stagger=2), "an unknown flag": _set(flags=4),
    "both flags": _set(flags=R.FILL_ALL | R.RESETS_ONLY)}


def check_refusals(make_rig, null_call):
    """every listed argument error returns LSIM_E_INVALID and leaves all four outputs, guards included, as they were"""
    N = 8
    rig = make_rig(N, 20)
    calls = R.launches(N)
    for call in calls[:2]:
        assert rig.launch(*call) == 0
    before = rig.outputs_raw()
    assert null_call() == abi.E_INVALID
    for name, edit in FRAMES_LOG_REFUSALS.items():
        assert rig.launch(*calls[2], edit=edit) == abi.E_INVALID, name
        after = rig.outputs_raw()
        for k in before:
            assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), f"{name}: {k} was written"
    assert rig.launch(*calls[2]) == 0


class GradRig(EditRig):
    """g [B, g_stride], mb_of, row_of, row_src and G [rows + 2, G_stride] (guarded), G pre-filled with LOG_FILL"""

    def __init__(self, g, mb_of, row_of, row_src, rows, latent_dim, G_stride, device=None, entry=None):
        super().__init__(device)
        self.rows, self.G_stride = int(rows), int(G_stride)
        T, N = row_of.shape
        self.add("g", np.asarray(g, np.float32))
        for k, v in (("mb_of", mb_of), ("row_of", row_of), ("row_src", row_src)):
            self.add(k, np.asarray(v, np.int32))
        self.add("G", np.full((self.rows + 2, self.G_stride), LOG_FILL, np.float32), guard=LOG_FILL)
        lg = LsimLatentRowsGrad()
        self.point(lg, ("g", "mb_of", "row_of", "row_src", "G"))
        lg.batch, lg.rows, lg.latent_dim, lg.g_stride, lg.G_stride, lg.num_steps, lg.num_envs = g.shape[0], self.rows, int(latent_dim), g.shape[1], self.G_stride, T, N
        self.lg = self.bind(lg, entry if device is not None else lib().emu_latent_rows_grad)

    def read(self):
        """G [rows + 2, G_stride] with the guard checked"""
        self.assert_guards()
        return self.get("G")


GRAD_REFUSALS = {
    **{f"{n} NULL": _bad_pointer(n, 0) for n in ("g", "mb_of", "row_of", "row_src", "G")},
    **{f"{n} misaligned": _bad_pointer(n, 2) for n in ("g", "mb_of", "row_of", "row_src", "G")},
    "batch 0": _set(batch=0), "rows < 0": _set(rows=-1), "latent_dim 0": _set(latent_dim=0), "g_stride < latent_dim": _set(g_stride=0),
    "G_stride < latent_dim": _set(G_stride=0), "num_steps 0": _set(num_steps=0), "num_envs 0": _set(num_envs=0),
    "num_steps * num_envs >= 2^31": _set(num_steps=2 ** 30, num_envs=4)}


def check_grad(make_rig, N, latent_dim, null_call=None):
    """lsim_latent_rows_grad on the scenario's row_of / row_src against the sequential fp32 sum, bit for bit; the minibatch is one
    quarter of a random permutation of T * N"""
    ref = R.run_reference(N, R.scenario_capacity(N))[0]
    T, rows = R.STEPS, int(ref.state[R.COUNT])
    rng = np.random.default_rng(100 * N + latent_dim)
    B = T * N // 4
    perm = rng.permutation(T * N)
    if N == 8:                                              # three transitions in 48 have no row: the permutation starts with one of them
        at = int(np.flatnonzero(ref.row_of.reshape(-1)[perm] < 0)[0])
        perm[[0, at]] = perm[[at, 0]]
    picked = perm[:B]
    mb_of = np.full(T * N, -1, dtype=np.int32)
    mb_of[picked] = np.arange(B, dtype=np.int32)
    g_stride, G_stride = latent_dim + 3, latent_dim + 5
    g = rng.standard_normal((B, g_stride)).astype(np.float32)
    flat_rows = ref.row_of.reshape(-1)
    unlogged = [k for k in picked if flat_rows[k] < 0]
    if N == 8:
        assert unlogged, "the overflowing scenario must put a transition without a frame row into the minibatch"
    g[mb_of[unlogged]] = np.nan                             # a transition with frame_row = -1 appears nowhere: its NaN would show
    want = R.rows_grad(g, mb_of, ref.row_of, ref.row_src, rows, latent_dim, np.full((rows + 2, G_stride), LOG_FILL, dtype=np.float32))
    assert np.isfinite(want).all()
    read_by = {int(r) for r in flat_rows[picked] if r >= 0}
    idle = [r for r in range(rows) if r not in read_by]
    assert idle and read_by, "the minibatch must leave some rows unread and read others"
    rig = make_rig(g, mb_of, ref.row_of, ref.row_src, rows, latent_dim, G_stride)
    assert rig.launch() == 0
    got = rig.read()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (N, latent_dim)
    assert (got[idle, :latent_dim].view(np.uint32) == 0).all()                 # exactly +0.0
    assert (got[rows:] == LOG_FILL).all() and (got[:, latent_dim:] == LOG_FILL).all()
    assert rig.launch() == 0                                # a second call: the same bits
    assert np.array_equal(rig.read().view(np.uint32), want.view(np.uint32))
    if null_call is not None:
        assert null_call() == abi.E_INVALID
        for name, edit in GRAD_REFUSALS.items():
            rig.put("G", LOG_FILL)
            assert rig.launch(edit=edit) == abi.E_INVALID, name
            assert (rig.raw("G") == LOG_FILL).all(), f"{name}: G was written"
        assert rig.launch(edit=_set(rows=0)) == 0 and (rig.raw("G") == LOG_FILL).all()
