"""Timed training loop for bench.py --mode train: the reference's total_fps definition (HIMR:179), i.e.
env-steps/s over collection (policy inference + LeggedRobot.step + storage) PLUS compute_returns + update().

The unit of timing is one WHOLE PPO iteration (HIMR:105-157): T = num_steps_per_env rollout steps, then GAE, then
HIMPPO.update().  `--steps K` asks for K env-steps; ceil(K / T) iterations are timed, so K is exact whenever it is a multiple of T
(pass K >= 1000, ten iterations or 1 s at the BASELINE size, when one clock ramp or collector pause must not move the line by several
per cent: VERDICT r2, r4) -- and `--warmup W` runs ceil(W / T) untimed iterations (at least six: the first update carries lazy library
initialisation and creates the optimiser state).  `value` stays
whole-region throughput (all timed env-steps / barrier-to-barrier time); with `full` the per-iteration minimum / median / maximum, the
kernel profile, the shader clock and the per-rank diagnostics are reported beside it."""
import ctypes
import os
import time

import torch

from ..envs import config as C
from .runner import HIMOnPolicyRunner


MIN_WARMUP_ITERATIONS = 6      # (round 6: on one fresh lease the first two timed iterations after three warm-ups still ran 9-14 % long; cause not isolated -- the box's host is shared)


def train_cfg_dict(task):
    ppo = C.TASKS[task][1]().to_dict()
    return {"runner": ppo["runner"], "algorithm": ppo["algorithm"], "policy": ppo["policy"]}


def weights_digest(module):
    """(sum, sum of squares) of every parameter in fp64 -- ranks that took identical optimiser steps agree to the last bit"""
    flat = torch.cat([p.detach().reshape(-1) for p in module.parameters()]).double()
    return [float(flat.sum()), float((flat * flat).sum())]


def run_train_bench(env, cfg, args, dev, rank, world, barrier, clocks=None, full=True):
    """-> (elapsed seconds, extra fields of the line, workload text, outputs of the last timed iteration).  full=False (a plain bench run)
    times the same iterations and skips everything the headline does not need: kernel profile, shader clock, per-rank diagnostics."""
    task = args.task if args.task in C.TASKS else "aliengo"
    tc = train_cfg_dict(task)
    torch.manual_seed(1)   # identical initial policy on every rank (then broadcast anyway)
    if C.TASKS[task][1]().runner_class_name == "HybridPolicyRunner":      # AMP configuration (AGA:297, AGA:329)
        from .hybrid import HybridPolicyRunner
        import numpy as np
        np.random.seed(1 + rank)
        runner = HybridPolicyRunner(env, tc, log_dir=None, device=str(dev))
    else:
        runner = HIMOnPolicyRunner(env, tc, log_dir=None, device=str(dev))
    use_graphs = os.environ.get("LSIM_NO_GRAPHS") != "1" and runner.enable_graphs()
    T = runner.num_steps_per_env
    iters = max(1, -(-args.steps // T))
    warm_iters = max(MIN_WARMUP_ITERATIONS, -(-args.warmup // T))
    env.episode_length_buf = torch.randint_like(env.episode_length_buf, high=int(env.max_episode_length))   # HIMR:90-91
    state = dict(obs=env.get_observations().clone(), critic=env.get_privileged_observations().clone())
    runner.alg.actor_critic.train()

    spans = {"collection": [], "update": []}      # wall-clock intervals of the two halves of every iteration (the clock sampler splits its samples by them)

    enqueue = []       # host seconds the update took to ENQUEUE (HIMPPO.update: up to its first read-back), every iteration incl. warm-up
    last = {}          # what the last iteration's update returned (the losses a caller of the loop receives)

    def one_iteration():
        """HIMR:105-157 without the logging: returns (collection seconds, learn seconds), each closed by a device sync"""
        t0 = time.perf_counter()
        for _ in range(T):
            if use_graphs:
                runner.graphs.step()
                state["critic"] = env.privileged_obs_buf
            else:
                with torch.inference_mode():
                    state["obs"], state["critic"], _, _, _ = runner._rollout_step(state["obs"], state["critic"])
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        with torch.inference_mode():
            runner.alg.compute_returns(state["critic"])
        if use_graphs:
            runner.graphs.end_iteration()
        last["update"] = runner.alg.update()
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        enqueue.append(getattr(runner.alg, "update_enqueue_s", 0.0))
        spans["collection"].append((t0, t1)); spans["update"].append((t1, t2))
        return t1 - t0, t2 - t1

    # The shipped GEMM table is only valid on the build it was tuned with: TunableOp rejects the whole file when one Validator line differs,
    # every GEMM then runs the default heuristics and the update loses its second stream (him_ppo._two_streams_allowed).  The line and
    # stderr say so (VERDICT r4 task 1d); `LSIM_TUNE=1 python bench.py` tunes a table for the build at hand (~50 s).
    from . import him_ppo as _hp
    tuned_table = os.environ.get("LSIM_TUNABLEOP_TABLE") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "tunableop_gfx950.csv")
    for _ in range(warm_iters):
        one_iteration()
    # what the update really runs on (the line must explain its own learn_s_per_update): streams, TunableOp
    tun = _hp.tunableop_status(dev, tuned_table)
    alg = runner.alg
    mb_rows = env.num_envs * T // alg.num_mini_batches
    multi = alg.dist_ctx is not None and alg.dist_ctx.enabled and alg.dist_ctx.world > 1
    two_streams = bool(alg._lr_t is not None and hasattr(alg, "_two_streams") and alg._two_streams(alg.actor_critic.critic, mb_rows, multi))
    if tun["enabled"] and not tun["tuning"] and tun["validators_match"] is False and rank == 0:
        import sys
        print(f"[bench] TunableOp REJECTED the GEMM table {tuned_table} (tuned on another build: {tun['validator_mismatches']}); every GEMM "
              f"runs the library's default heuristics and the update runs on {'two streams' if two_streams else 'ONE stream'}.  "
              "LSIM_TUNE=1 python bench.py writes a table for this build (gpurun_out/tunableop_new.csv)", file=sys.stderr)
    # Python's cyclic collector: a full (generation 2) pass over the objects the set-up left behind -- modules, configs, the captured graphs --
    # stalls the launch-bound update for ~60 ms once every few iterations (measured: one iteration of 30 at 0.139 s instead of 0.078 s).
    # Collect once and move the survivors to the permanent generation, as the runner's learn() does after its first iteration.
    import gc
    gc.collect(); gc.freeze()
    n_prof = iters * T
    if full:
        env._L.lsim_set_profiling(env._h, n_prof)
    coll = learn = 0.0
    per_iter = []
    multi_diag = full and alg.dist_ctx is not None and alg.dist_ctx.enabled        # N > 1 (or the forced 1-rank group): how long this rank stands in the collectives
    if multi_diag:
        alg.dist_ctx.timing = True
        alg.dist_ctx.take_blocked_seconds()
    blocked = 0.0
    barrier()
    nf0 = int(env.nonfinite_envs)                # (a host read: outside the timed region)
    if clocks is not None and full:
        clocks.start()
    t0 = time.perf_counter()
    for _ in range(iters):
        c, l = one_iteration()
        coll += c
        learn += l
        per_iter.append([round(c, 5), round(l, 5)])
        if multi_diag:
            blocked += alg.dist_ctx.take_blocked_seconds()       # (one_iteration ended with a device synchronisation)
    barrier()
    elapsed = time.perf_counter() - t0
    nonfinite = int(env.nonfinite_envs) - nf0
    outputs = last_outputs(env, runner, last.get("update"))
    workload = (f"{task}: {type(runner).__name__} loop, {iters} whole PPO iteration(s) timed, each = {T} x (policy inference + LeggedRobot.step + "
                f"storage) + GAE + {type(alg).__name__}.update ({alg.num_learning_epochs} epochs x {alg.num_mini_batches} minibatches), "
                f"{env.num_envs} envs/GPU")
    extra = {"timed_env_steps": iters * T, "nonfinite_envs": nonfinite, "ppo_updates_timed": iters, "warmup_iterations": warm_iters,
             "ppo_iteration_wall_s": elapsed / iters, "collection_s_per_iteration": coll / iters, "learn_s_per_update": learn / iters}
    if not full:
        return elapsed, extra, workload, outputs
    sclk = clocks.stop(phases=spans) if clocks is not None else None
    ms_a, ms_b, n = (ctypes.c_float * n_prof)(), (ctypes.c_float * n_prof)(), ctypes.c_int(n_prof)
    env._L.lsim_read_profile(env._h, ms_a, ms_b, ctypes.byref(n))
    ka = sum(ms_a[i] for i in range(n.value)) / max(n.value, 1)
    kb = sum(ms_b[i] for i in range(n.value)) / max(n.value, 1)
    digest = weights_digest(runner.alg.actor_critic)
    # which robot this rank really simulated: total mass of the model table the simulator was created with (aliengo 24.9 kg, go1 11.3 kg)
    mass = float(sum(b.mass for b in env.model.bodies))
    import torch.distributed as dist
    walls_local = [c + l for c, l in per_iter]
    mine = [coll / iters, learn / iters, blocked / iters, min(walls_local), max(walls_local), 1.0 if two_streams else 0.0]
    if dist.is_initialized():               # N > 1, or the 1-rank RCCL group of LSIM_DEBUG_FORCE_COLLECTIVES
        d = torch.tensor(digest + [mass] + mine, device=dev, dtype=torch.float64)
        all_d = [torch.zeros_like(d) for _ in range(world)]
        dist.all_gather(all_d, d)
        digests = [x.tolist()[:2] for x in all_d]
        masses = [x.tolist()[2] for x in all_d]
        per_rank = [x.tolist()[3:] for x in all_d]
        # every rank's wall time of every timed iteration: max - min ACROSS ranks per iteration = how far the slowest rank trails the fastest
        w = torch.tensor(walls_local, device=dev, dtype=torch.float64)
        all_w = [torch.zeros_like(w) for _ in range(world)]
        dist.all_gather(all_w, w)
        wm = torch.stack(all_w)
        skew = (wm.max(dim=0).values - wm.min(dim=0).values).tolist()
    else:
        digests, masses, per_rank, skew = [digest], [mass], [mine], [0.0] * len(walls_local)
    walls = sorted(c + l for c, l in per_iter)
    med = walls[len(walls) // 2] if len(walls) % 2 else 0.5 * (walls[len(walls) // 2 - 1] + walls[len(walls) // 2])
    extra.update({"kernel_a_ms": ka, "kernel_b_ms": kb,
             "collection_env_steps_per_s": world * env.num_envs * iters * T / max(coll, 1e-9),
             "collection_learn_s_by_iteration": per_iter[:32], "rollout_hip_graphs": bool(use_graphs), "weights_digest_by_rank": digests,
             "ranks_in_lockstep": all(x == digests[0] for x in digests), "robot_mass_kg_by_rank": [round(m, 3) for m in masses],
             # this rank's iterations: spread of the timed sample, and the throughput the median iteration gives (whole job, weak scaling)
             "iteration_wall_s_min_median_max": [round(walls[0], 5), round(med, 5), round(walls[-1], 5)],
             "iteration_spread_frac": (walls[-1] - walls[0]) / med,
             "value_from_median_iteration": world * env.num_envs * T / med,
             "update_two_streams": two_streams, "tunableop": tun,
             # host time to enqueue one update (Python + launches, no read-back inside) against learn_s_per_update: close to it = the host's launch rate,
             # not the device, bounds the update on this box (the spread of the line between leases)
             "update_host_enqueue_s": sum(enqueue[-iters:]) / max(len(enqueue[-iters:]), 1),
             # where a multi-rank run's time goes, per rank (VERDICT r5 task 6: the first scaling curve must be able to say where lost efficiency went):
             # a rank's iteration = collection + learn; `collective_blocked_s` = the part of learn its compute stream stood still waiting for a gradient
             # all-reduce (expected ~1-2 ms of 84 on xGMI); `iteration_skew_s` = slowest minus fastest rank, per timed iteration
             "per_rank": {"collection_s": [round(r[0], 5) for r in per_rank], "learn_s": [round(r[1], 5) for r in per_rank],
                          "collective_blocked_s": [round(r[2], 5) for r in per_rank], "iteration_wall_s_min": [round(r[3], 5) for r in per_rank],
                          "iteration_wall_s_max": [round(r[4], 5) for r in per_rank], "update_two_streams": [bool(r[5] > 0.5) for r in per_rank],
                          "collective_timing": bool(multi_diag)},
             "iteration_skew_s_max_mean": [round(max(skew), 5), round(sum(skew) / max(len(skew), 1), 5)],
             # which form the hidden layers' forward ran in (learn/fused_linear.py: linear_elu_forward): "aligned" = the library's MFMA kernel with bias + ELU in
             # the epilogue on the layers with 16-byte-aligned rows, BLAS + torch ELU on the rest; "0" = BLAS + ELU everywhere; "all"
             "linear_elu_forward": os.environ.get("LSIM_ELU_FORWARD", "aligned"),
             "sclk_during_timed_region": sclk})
    return elapsed, extra, workload, outputs


def env_outputs(env):
    """what LeggedRobot.step_device hands its caller after the last step: observations, privileged observations, rewards, reset flags"""
    return {"obs": env.obs_buf, "privileged_obs": env.privileged_obs_buf, "rew": env.rew_buf, "reset": env.reset_buf}


def last_outputs(env, runner, update_ret):
    """what the timed loop computed in its last iteration, as device / host values: the environment's outputs of the last step, the actions
    of the last rollout step (fused rollout graphs only: the eager path keeps them in its storage), the update's returned losses and the
    parameters of the policy after that update"""
    out = env_outputs(env)
    if getattr(runner.graphs, "actions", None) is not None:
        out["actions"] = runner.graphs.actions
    if update_ret is not None:
        vals = update_ret if isinstance(update_ret, (tuple, list)) else (update_ret,)
        out["update_losses"] = torch.tensor([float(v) for v in vals], dtype=torch.float64)
    out["policy_params"] = torch.cat([p.detach().reshape(-1).float() for p in runner.alg.actor_critic.parameters()])
    return out
