"""TEST INFRASTRUCTURE -- the numpy references of the two launches of isaacgymloco_amd/csrc/ls_frames_log.h, written from the text of
include/lsim.h and from nothing else: FramesLog, the state machine of lsim_sensor_frames_log, and rows_grad, the sequential fp32 sum of
lsim_latent_rows_grad.  Plus the scenario both the CPU shim and the device run (tests/frames_log_scenes.py drives it)."""
import numpy as np

FILL_ALL, RESETS_ONLY = 1, 2        # LSIM_SENSOR_FILL_ALL, LSIM_SENSOR_RESETS_ONLY (asserted against the header by the tests)
COUNT, OVERFLOW, BASE, NEXT = 0, 1, 2, 3


def default_capacity(N, steps, period):
    """the stage's default: the start of the rollout, every tick-due capture, and room for two resets per env per rollout"""
    return N * (1 + -(-(steps - 1) // period) + 2)


def due(flags, episode_length, period, stagger, tick):
    """[N] bool: the rule of lsim_depth_encode, word for word"""
    e = np.arange(episode_length.shape[0], dtype=np.int64)
    fill = np.full(e.shape, bool(flags & FILL_ALL)) | (episode_length == 0)
    tick_due = ((tick + (e if stagger else 0)) % period == 0) & (not flags & RESETS_ONLY)
    return fill | tick_due


class FramesLog:
    """the four outputs as numpy arrays, each starting from the pre-fill the caller gives, advanced call by call"""

    def __init__(self, N, num_steps, capacity, frames, pixels, row_stride, period, stagger, env_stride=1, log_fill=np.float32(-7.25), int_fill=-99):
        self.N, self.T, self.capacity, self.frames, self.pixels, self.row_stride = N, num_steps, capacity, frames, pixels, row_stride
        self.period, self.stagger, self.env_stride = period, stagger, env_stride
        self.log = np.full((capacity, frames, row_stride), log_fill, dtype=np.float32)
        self.row_of = np.full((num_steps, N), int_fill, dtype=np.int32)
        self.row_src = np.full((capacity,), int_fill, dtype=np.int32)
        self.state = np.zeros(4, dtype=np.int32)

    def launch(self, hist, episode_length, tick, step, flags):
        """hist [N, slots, stride] fp32, episode_length [N] int64"""
        N = self.N
        assert 0 <= step < self.T and (step > 0 or flags & FILL_ALL)
        visited = np.arange(N) % self.env_stride == 0
        logged = visited & due(flags, episode_length, self.period, self.stagger, tick)
        before = 0 if flags & FILL_ALL else int(self.state[COUNT])
        row = before
        for e in range(N):
            if not visited[e]:
                self.row_of[step, e] = -1
            elif logged[e]:
                if row < self.capacity:
                    self.log[row, :, :self.pixels] = hist[e, :self.frames, :self.pixels]
                    self.log[row, :, self.pixels:] = 0.0
                    self.row_of[step, e] = row
                    self.row_src[row] = step * N + e
                else:
                    self.row_of[step, e] = -1
                    self.state[OVERFLOW] += 1
                row += 1
            elif not flags & RESETS_ONLY:
                self.row_of[step, e] = self.row_of[step - 1, e]
        self.state[BASE] = before
        self.state[COUNT] = self.state[NEXT] = min(row, self.capacity)
        return int(logged.sum())


def rows_grad(g, mb_of, row_of, row_src, R, latent_dim, G):
    """G[:R, :latent_dim] written in place: the fp32 sum in ascending t"""
    T, N = row_of.shape
    for r in range(R):
        acc = np.zeros(latent_dim, dtype=np.float32)
        s = int(row_src[r])
        if 0 <= s < T * N:
            t, e = divmod(s, N)
            while t < T and row_of[t, e] == r:
                m = int(mb_of[t * N + e])
                if m >= 0:
                    acc = (acc + g[m, :latent_dim]).astype(np.float32)
                t += 1
        G[r, :latent_dim] = acc
    return G


# ---- the scenario of the issue: pixels 12 in a stride of 16, 3 slots of which 2 are the image, period 3 staggered, 6 steps
PIXELS, HIST_STRIDE, SLOTS, FRAMES, PERIOD, STEPS, ROW_STRIDE, TICK0 = 12, 16, 3, 2, 3, 6, 16, 40
SIZES = (8, 70, 1030)               # one wave; across a wave boundary; across several workgroups of the rank launch


def reset_plan(N):
    """{step: envs whose episode starts there}: env 0, env N - 1 and, where they exist, the two neighbours on either side of index 64;
    `by_hand`: the envs of the one RESETS_ONLY call, made inside step 3"""
    near = [e for e in (62, 63, 64, 65) if e < N] or [N // 2 - 1, N // 2]
    plan = {1: [0, near[0]], 2: [N - 1] + near[1:3], 4: [0, N - 1] + near, 5: near[-2:] + [1, N - 1]}
    return plan, [2 % N, near[-1], N - 2]


def launches(N, seed=0):
    """the scenario as a list of (hist, episode_length, tick, step, flags): a FILL_ALL call at step 0, then one call per step with the
    planned resets, and a RESETS_ONLY call ahead of step 3's"""
    rng = np.random.default_rng(seed + N)
    plan, by_hand = reset_plan(N)
    out = []

    def one(step, flags, fresh):
        hist = rng.standard_normal((N, SLOTS, HIST_STRIDE)).astype(np.float32)
        el = np.full(N, 3 + step, dtype=np.int64)
        el[list(fresh)] = 0
        out.append((hist, el, TICK0 + max(step - 1, 0), step, flags))
    one(0, FILL_ALL, ())
    for step in range(1, STEPS):
        if step == 3:
            one(step, RESETS_ONLY, by_hand)
        one(step, 0, plan.get(step, ()))
    return out


def run_reference(N, capacity, seed=0, pixels=PIXELS):
    ref = FramesLog(N, STEPS, capacity, FRAMES, pixels, ROW_STRIDE, PERIOD, 1)
    logged = [ref.launch(*a) for a in launches(N, seed)]
    return ref, logged


def scenario_capacity(N, seed=0):
    """N = 8: three rows fewer than the reference itself needs, all of them missed at the last step; else the default"""
    if N != 8:
        return default_capacity(N, STEPS, PERIOD)
    ref, logged = run_reference(N, 10 ** 6, seed)
    need = int(ref.state[COUNT])
    assert logged[-1] > 3, "the last step must log more envs than the capacity is short of"
    return need - 3
