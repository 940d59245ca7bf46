#!/usr/bin/env python3
"""HIP-event time of the range-sensor launch (lsim_raycast) next to kernel A's.

    python tools/raycast_time.py [--num-envs 4096] [--terrains flat,stairs] [--iters 100] [--warmup 10] [--out profiles/raycast_time.json]

Per terrain (Aliengo, zero actions for 20 steps so that the robots stand where they were put): `camera_us` = one launch of a 64 x 48 depth
camera (87 degrees, far 5 m, pitched down 30 degrees, 0.3 m ahead of the base), `lidar_us` = one launch of a 16 x 360 lidar (30 degrees
vertical, far 10 m), each with rays/s; `kernel_a_us` = kernel A from the library's own events (lsim_read_profile) in the same process;
`cells_per_ray` / `triangles_per_ray` = the walk's two debug counters, from one launch through a build of the library with
-DLS_RAYCAST_COUNTERS (isaacgymloco_amd/csrc/liblsim_rccount.so, built here when stale; the product build has no counters).
`--bodies`: each sensor is also timed with see_robot=True (lsim_raycast_bodies, all bodies seen) in the same process, next to lsim_raycast and
kernel A: `<sensor>_bodies_us`, its ratio to the terrain-only launch, the share of rays that end on a body, and from the counters build the
primitives that passed the bounding test per ray and the cells walked per ray (the walk stops at the body hit).
`--model period=5,stagger=1,latency=1,frames=2,noise=0.01:0.002,dropout=0.02` (implies --bodies): each see_robot sensor is also timed through
lsim_sensor_capture with that sensors.SensorModel, the tick advancing by one per launch so that a staggered period is averaged over whole
periods (`<sensor>_model_us`), and with SensorModel() -- period 1, everything else off: what the epilogue and the history traffic add to
lsim_raycast_bodies (`<sensor>_model_period1_us`); both with their ratio to `<sensor>_bodies_us` of the same process.
`--mount-jitter POS,ROT_DEG` (metres, degrees; needs --model; a measurement of its own: the camera only, no lidar, no counters): per terrain,
in one process, `jitter_all_fresh_us` / `jitter_none_fresh_us` = lsim_sensor_mount_jitter alone with LSIM_SENSOR_FILL_ALL and with no env at
episode_length 0; `camera_model_us` = lsim_sensor_capture exactly as --model times it, on the nominal mount, and `camera_model_jittered_us` =
the same launch on a sensor whose mounts were drawn once for every env (the jitter launch itself kept out of the timed loop), the two
alternating `--repeats` times, each with its median and its range over the repeats (the run-to-run spread of this process);
`camera_model_update_with_jitter_us` = update() as a jittered sensor runs it in a step: the jitter launch (nobody fresh) and the capture.
`--instrument latency=0:2,noise_gain=0.5:2,depth_scale=0.02,depth_quad=0.005,fov=0.02` (the text of evaluate's --camera-instrument; needs
--model; a measurement of its own, no counters): per terrain and for the camera and the lidar (the lidar without the field-of-view term,
which it cannot take), in one process and alternating `--repeats` times, each with its median and range: `<sensor>_capture_us` =
lsim_sensor_capture as --model times it; `<sensor>_inst_neutral_us` = lsim_sensor_capture_inst on the neutral rows; `<sensor>_inst_drawn_us` =
the same on rows drawn once for every env (the draw launch kept out of the timed loop); `draw_all_fresh_us` / `draw_none_fresh_us` =
lsim_sensor_instrument alone with LSIM_SENSOR_FILL_ALL and with no env at episode_length 0.
`--map size=32,resolution=0.0625,source=noisy` (any subset; needs --model; a measurement of its own, the camera only, no counters): per
terrain, in one process and alternating `--repeats` times, each with its median and range: `capture_us` = lsim_sensor_capture as --model
times it (the tick advancing, so a staggered period is averaged over whole periods); `map_us` = lsim_elevation_map alone over the same
ticks, reading the rows the captures left; `map_all_due_us` = the same launch with LSIM_SENSOR_FILL_ALL (every env cleared and inserted);
`update_with_map_us` = update() as a sensor with a map runs it in a step: the capture and the map's launch behind it.
`--map ...,fusion=default` (or `fusion=band:0.1/gate:3`, sensors.parse_map_fusion): the map's launch is lsim_elevation_map_fused, and
`plain_map_us` / `plain_map_all_due_us` time lsim_elevation_map of the same map on the same ticks, in the same repetition.
`--map ...,cleanup=default` (or `cleanup=margin:0.05/min_rays:2`, sensors.parse_map_cleanup): `cleanup_us` = lsim_elevation_map_cleanup alone
over the same ticks, `cleanup_all_due_us` = the same with period 1 (every env due; LSIM_SENSOR_FILL_ALL would only zero its counters),
`update_without_cleanup_us` = update() of a second camera whose map lacks the option; `update_with_map_us` then includes the clean-up.
`--model ... --stereo default` (or `--stereo baseline=0.05,edge_hole=0.25,...`, sensors.parse_stereo; a measurement of its own, written to
profiles/sensor_stereo_time.json unless --out names another file): per terrain, in one process and alternating `--repeats` times, each
with its median and range: `capture_us` / `capture_all_due_us` = the capture alone over whole periods and with LSIM_SENSOR_FILL_ALL;
`stereo_us` / `stereo_all_due_us` = lsim_sensor_stereo alone over the same ticks, on the rows the captures left; `update_us` and
`update_with_stereo_us` = update() of a camera without and with the option; `hole_share` / `fattened_share` = the share of one whole
capture's pixels the stage rewrites (stereo_counts()).
`--map ... --odometry scale=0.02,yaw_per_m=0.01,z_per_m=0.01,noise=0.005:0.002:0.002` and / or `--map-rows 1|2` (the map policy's two
launches; a measurement of its own, written to profiles/map_policy_time.json unless --out names another file): per terrain, in one process
and alternating `--repeats` times, each with its median and range: `capture_us` as above; `odometry_us` = lsim_odometry_step alone, the tick
advancing; `map_rows_us` = lsim_map_rows alone over the map's scan; `map_rows_torch_us` = the torch statement of the same rows into the same
buffer (two subtractions, clamp, product, and with two channels the copy of `known`: five elementwise launches, without the non-finite
rule); `update_us` = update() as the sensor of a map policy runs it in a step: odometry, capture, map, rows.
`--shade` (or `--shade sun=145:50,shadows=1,...`, sensors.parse_shading; a measurement of its own, written to
profiles/sensor_shade_time.json unless --out names another file): the 128 x 96 chase camera of sensors.chase_camera, per terrain, in one
process and alternating `--repeats` times, each with its median and range, once with every env drawn and once with env_stride = N (the
viewer's case: env 0 alone, 50 times the iterations): `rays_us` = lsim_raycast_bodies alone, `shade_us` = lsim_sensor_shade alone on the rows the rays left,
`shade_plain_us` = the same launch without LSIM_SHADE_SHADOWS, `update_us` = the pair as update() runs it; `shade_over_rays` their ratio;
`lit_share` / `shadowed_share` = the share of the drawn pixels that face the sun lit and dark.  `--parent-lib PATH` (a liblsim.so built from
the parent commit) also times that library's lsim_raycast_bodies on the same struct in the same loops: `rays_parent_us`.
`--foot-scan` (or `--foot-scan radii:0.06/0.12,counts:6/8`, sensors.parse_foot_scan; a measurement of its own, written to
profiles/foot_scan_time.json unless --out names another file; --model defaults to period=5,stagger=1 and --map to size=32): the 64 x 48
camera with a map, per terrain, in one process and alternating `--repeats` times, each with its median and range: `capture_us` and `map_us` =
the capture and the map's launch alone over whole periods; `map_rows_us` = lsim_map_rows (two channels, 187 points) of a second camera
that carries the parent's chain; `foot_scan_map_us` = lsim_foot_scan alone with the map as its source (two channels, 4 K points per env);
`foot_scan_terrain_us` = the same launch with the terrain as its source (sensors.TerrainFootScan); `update_us` / `update_parent_us` =
update() of the camera with foot rows and of the one with scan rows, as a step runs them.
The torch restatement of the same walk ("what a user had to do before") was not written: `torch_us` is null.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from isaacgymloco_amd import abi, lib  # noqa: E402
from isaacgymloco_amd.csrc import build as hip_build  # noqa: E402
from isaacgymloco_amd.envs import config as C, sensors  # noqa: E402
from isaacgymloco_amd.envs.legged_robot import LeggedRobot  # noqa: E402

COUNT_LIB = os.path.join(os.path.dirname(hip_build.LIB), "liblsim_rccount.so")


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def counters(sensor, count_lib):
    """(cells, triangles) per ray of one launch through the counters build, on the sensor's own struct"""
    sensor.state.zero_()
    lib.check(count_lib.lsim_raycast(ctypes.byref(sensor.ray_struct), sensor.env._stream()), what="lsim_raycast (counters build)")
    torch.cuda.synchronize()
    st = sensor.state.cpu().tolist()
    rays = sensor.num_rays * ((sensor.env.num_envs + sensor.env_stride - 1) // sensor.env_stride)
    sensor.state.zero_()
    return st[2] / rays, st[3] / rays, st[0]


def counters_bodies(sensor, count_lib):
    """(primitives past the bounding test, cells, triangles) per ray of one lsim_raycast_bodies launch through the counters build"""
    sensor.state.zero_()
    lib.check(count_lib.lsim_raycast_bodies(ctypes.byref(sensor.bodies_struct), sensor.env._stream()), what="lsim_raycast_bodies (counters build)")
    torch.cuda.synchronize()
    st = sensor.state.cpu().tolist()
    rays = sensor.num_rays * sensor.env.num_envs
    sensor.state.zero_()
    return st[1] / rays, st[2] / rays, st[3] / rays


def parse_model(text):
    """sensors.SensorModel from key=value pairs: period, stagger, latency, frames, noise=sigma0:sigma2, dropout, drop_value, clip=lo:hi, normalise"""
    return sensors.parse_option(sensors.SensorModel, text)


def timed_ticks(what, iters, warmup, flags=0):
    """`timed` over launches whose tick advances by one each: `what` is a sensor (its update()) or one stage of its chain (that launch alone)"""
    run = what.launch if isinstance(what, sensors.Stage) else lambda tick, flags: what.update(tick=tick, flags=flags)
    tick = [0]

    def fn():
        run(tick[0], flags)
        tick[0] += 1
    return timed(fn, iters, warmup)


def measure_mount_jitter(n, terrain, iters, warmup, model, jitter, repeats):
    """the --mount-jitter measurement (module docstring)"""
    cfg = C.aliengo_cfg()
    cfg.env.num_envs = n
    cfg.terrain.terrain_proportions = [1.0, 0.0, 0.0, 0.0, 0.0, 0.0] if terrain == "flat" else [0.0, 0.0, 0.0, 0.0, 0.5, 0.5]
    env = LeggedRobot(cfg, sim_device="cuda:0", seed=1)
    env.reset()
    zero = torch.zeros(n, 12, device="cuda:0")
    for _ in range(20):
        env.step_device(zero)
    torch.cuda.synchronize()
    make = lambda **kw: sensors.depth_camera(env, 64, 48, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, near=0.05, far=5.0, see_robot=True, labels=True,
                                             model=model, **kw)
    nominal, jittered = make(), make(mount_jitter=jitter)
    nominal.refresh(tick=0)
    jittered.refresh(tick=0)                    # draws every env's mount once
    out = {"num_envs": n, "terrain": terrain, "resetting_envs": int((env.episode_length_buf == 0).sum().item()),
           "mount_offset_max_m": float((jittered.mount[:, :3] - jittered.mount_nominal[:, :3]).abs().max().item())}
    launch = lambda flags: jittered.stage("mount_jitter").launch(0, flags)
    fill_all = abi.DEFINES["LSIM_SENSOR_FILL_ALL"]
    whole = max(model.period, iters // model.period * model.period)
    rows = {"jitter_all_fresh_us": [], "jitter_none_fresh_us": [], "camera_model_us": [], "camera_model_jittered_us": [], "camera_model_update_with_jitter_us": []}
    for _ in range(repeats):
        rows["jitter_all_fresh_us"].append(timed(lambda: launch(fill_all), iters, warmup))
        rows["jitter_none_fresh_us"].append(timed(lambda: launch(0), iters, warmup))
        rows["camera_model_us"].append(timed_ticks(nominal, whole, warmup))
        rows["camera_model_jittered_us"].append(timed_ticks(jittered.stage("capture"), whole, warmup))     # the capture alone, reading the mounts drawn above
        rows["camera_model_update_with_jitter_us"].append(timed_ticks(jittered, whole, warmup))
    for k, v in rows.items():
        out[k], out[k + "_range"], out[k + "_all"] = sorted(v)[len(v) // 2], [min(v), max(v)], v
    out["jittered_over_nominal"] = out["camera_model_jittered_us"] / out["camera_model_us"]
    out["nonfinite_rays"] = int(nominal.nonfinite_rays.item()) + int(jittered.nonfinite_rays.item())
    return out


def measure_map(n, terrain, iters, warmup, model, emap, repeats):
    """the --map measurement (module docstring)"""
    cfg = C.aliengo_cfg()
    cfg.env.num_envs = n
    cfg.terrain.terrain_proportions = [1.0, 0.0, 0.0, 0.0, 0.0, 0.0] if terrain == "flat" else [0.0, 0.0, 0.0, 0.0, 0.5, 0.5]
    env = LeggedRobot(cfg, sim_device="cuda:0", seed=1)
    env.reset()
    zero = torch.zeros(n, 12, device="cuda:0")
    for _ in range(20):
        env.step_device(zero)
    env.episode_length_buf[:] = 20               # nobody is fresh inside the timed loops: the period alone decides who is due
    torch.cuda.synchronize()
    cam = sensors.depth_camera(env, 64, 48, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, near=0.05, far=5.0, see_robot=True, labels=True, model=model)
    cam.refresh(tick=0)
    plain = None
    if emap.fusion is not None:                  # ...,fusion=...: lsim_elevation_map of the same map is timed next to the fused launch, on the same ticks
        cam.attach_map(sensors.ElevationMap(**{k: v for k, v in emap.record().items() if k not in ("fusion", "cleanup")}))
        plain = cam.stage("map")                 # a Stage owns its struct and its tensors (Stage.buffers): held here, they outlive its place in the chain
    cam.attach_map(emap)
    if plain is not None:
        held = plain.buffers
        assert all(getattr(plain.struct, k) == held[k].data_ptr() for k in ("height", "stamp", "cell", "scan", "known", "pts", "state")), "the plain map's stage lost its arrays"
    em = cam.stage("map").struct
    whole = max(model.period, iters // model.period * model.period)
    fill_all = abi.DEFINES["LSIM_SENSOR_FILL_ALL"]
    rows = {"capture_us": [], "map_us": [], "map_all_due_us": [], "update_with_map_us": []}
    if plain is not None:
        rows.update(plain_map_us=[], plain_map_all_due_us=[])
    clean = cam.stage("map_cleanup")             # ...,cleanup=...: the clean-up's launch alone, next to the map's on the same ticks
    if clean is not None:
        rows.update(cleanup_us=[], cleanup_all_due_us=[], update_without_cleanup_us=[])
        bare = sensors.depth_camera(env, 64, 48, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, near=0.05, far=5.0, see_robot=True, labels=True, model=model)
        bare.refresh(tick=0)
        bare.attach_map(sensors.ElevationMap(**{k: v for k, v in emap.record().items() if k != "cleanup"}))

    def every_env(stage):
        """the clean-up with period 1: every env due and none fresh (LSIM_SENSOR_FILL_ALL would only zero its counters)"""
        period, stage.struct.period = stage.struct.period, 1
        t = timed_ticks(stage, whole, warmup)
        stage.struct.period = period
        return t
    for _ in range(repeats):
        if clean is not None:
            rows["cleanup_us"].append(timed_ticks(clean, whole, warmup))
            rows["cleanup_all_due_us"].append(every_env(clean))
            rows["update_without_cleanup_us"].append(timed_ticks(bare, whole, warmup))
        if plain is not None:
            rows["plain_map_us"].append(timed_ticks(plain, whole, warmup))
            rows["plain_map_all_due_us"].append(timed_ticks(plain, whole, warmup, fill_all))
        rows["capture_us"].append(timed_ticks(cam.stage("capture"), whole, warmup))      # the capture alone
        rows["map_us"].append(timed_ticks(cam.stage("map"), whole, warmup))
        rows["map_all_due_us"].append(timed_ticks(cam.stage("map"), whole, warmup, fill_all))
        rows["update_with_map_us"].append(timed_ticks(cam, whole, warmup))
    out = {"num_envs": n, "terrain": terrain, "rays": cam.num_rays, "scan_points": int(em.num_points), "size": int(em.size),
           "coverage": float(cam.map_known().float().mean().item()), "cells_known": float((cam.map_state()[1] >= 0).float().mean().item())}
    for k, v in rows.items():
        out[k], out[k + "_range"], out[k + "_all"] = sorted(v)[len(v) // 2], [min(v), max(v)], v
    out["map_over_capture"] = out["map_us"] / out["capture_us"]
    if clean is not None:
        out["cleanup_over_map"], out["cells_forgotten"] = out["cleanup_us"] / out["map_us"], int(cam.map_cleared().sum().item())
    out["nonfinite"] = int(cam.nonfinite_rays.item()) + int(cam.map_nonfinite.item())
    return out


def measure_stereo(n, terrain, iters, warmup, model, stereo, repeats):
    """the --stereo measurement (module docstring)"""
    cfg = C.aliengo_cfg()
    cfg.env.num_envs = n
    cfg.terrain.terrain_proportions = [1.0, 0.0, 0.0, 0.0, 0.0, 0.0] if terrain == "flat" else [0.0, 0.0, 0.0, 0.0, 0.5, 0.5]
    env = LeggedRobot(cfg, sim_device="cuda:0", seed=1)
    env.reset()
    zero = torch.zeros(n, 12, device="cuda:0")
    for _ in range(20):
        env.step_device(zero)
    env.episode_length_buf[:] = 20               # nobody is fresh inside the timed loops: the period alone decides who is due
    torch.cuda.synchronize()
    make = lambda **kw: sensors.depth_camera(env, 64, 48, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, near=0.05, far=5.0, see_robot=True, labels=True,
                                             model=model, **kw)
    plain, cam = make(), make(stereo=stereo)
    plain.refresh(tick=0)
    cam.refresh(tick=0)
    st = cam.stage("stereo").struct
    whole = max(model.period, iters // model.period * model.period)
    fill_all = abi.DEFINES["LSIM_SENSOR_FILL_ALL"]
    rows = {"capture_us": [], "capture_all_due_us": [], "stereo_us": [], "stereo_all_due_us": [], "update_us": [], "update_with_stereo_us": []}
    for _ in range(repeats):
        rows["capture_us"].append(timed_ticks(cam.stage("capture"), whole, warmup))      # the capture alone
        rows["capture_all_due_us"].append(timed_ticks(cam.stage("capture"), whole, warmup, fill_all))
        rows["stereo_us"].append(timed_ticks(cam.stage("stereo"), whole, warmup))        # the stage alone, over the same ticks, on the rows the captures left
        rows["stereo_all_due_us"].append(timed_ticks(cam.stage("stereo"), whole, warmup, fill_all))
        rows["update_us"].append(timed_ticks(plain, whole, warmup))
        rows["update_with_stereo_us"].append(timed_ticks(cam, whole, warmup))
    counts = cam.stereo_counts().clone()
    cam.refresh(tick=0)                          # one capture of every env: the share of its pixels the stage rewrites
    torch.cuda.synchronize()
    holes, fat = ((cam.stereo_counts() - counts).double() / (n * cam.num_rays)).tolist()
    out = {"num_envs": n, "terrain": terrain, "rays": cam.num_rays, "fb": float(st.fb), "window": int(st.window), "hole_share": holes, "fattened_share": fat}
    for k, v in rows.items():
        out[k], out[k + "_range"], out[k + "_all"] = sorted(v)[len(v) // 2], [min(v), max(v)], v
    out["stereo_over_capture"] = out["stereo_us"] / out["capture_us"]
    out["nonfinite_rays"] = int(cam.nonfinite_rays.item())
    return out


def measure_shade(n, terrain, base_iters, warmup, shading, repeats, parent=None):
    """the --shade measurement (module docstring)"""
    cfg = C.aliengo_cfg()
    cfg.env.num_envs = n
    cfg.terrain.terrain_proportions = [1.0, 0.0, 0.0, 0.0, 0.0, 0.0] if terrain == "flat" else [0.0, 0.0, 0.0, 0.0, 0.5, 0.5]
    env = LeggedRobot(cfg, sim_device="cuda:0", seed=1)
    env.reset()
    zero = torch.zeros(n, 12, device="cuda:0")
    for _ in range(20):
        env.step_device(zero)
    torch.cuda.synchronize()
    shadows = abi.DEFINES["LSIM_SHADE_SHADOWS"]
    out = {"num_envs": n, "terrain": terrain, "camera": "128x96 chase, hfov 60, frame yaw, far 8 m"}
    for name, stride in (("all_envs", 1), ("one_env", n)):
        cam = sensors.chase_camera(env, 128, 96, env_stride=stride, shading=shading)
        iters = base_iters * (50 if stride > 1 else 1)        # one env is 1 / N of the work: the timed window stays a good fraction of a second
        rays, shade = cam.stage("rays"), cam.stage("shade")
        rows = {"rays_us": [], "shade_us": [], "shade_plain_us": [], "update_us": []}
        if parent is not None:
            rows["rays_parent_us"] = []
            stream = env._stream()
            old = lambda: lib.check(parent.lsim_raycast_bodies(ctypes.byref(cam.bodies_struct), stream), what="lsim_raycast_bodies (parent)")
        cam.update()
        for _ in range(repeats):
            rows["rays_us"].append(timed(lambda: rays.launch(0, 0), iters, warmup))
            if parent is not None:
                rows["rays_parent_us"].append(timed(old, iters, warmup))
            rows["shade_us"].append(timed(lambda: shade.launch(0, 0), iters, warmup))
            shade.struct.shade_flags = 0
            rows["shade_plain_us"].append(timed(lambda: shade.launch(0, 0), iters, warmup))
            shade.struct.shade_flags = shadows if shading.shadows else 0
            rows["update_us"].append(timed(cam.update, iters, warmup))
        cam.update()
        torch.cuda.synchronize()
        surf, lab = cam.surface()[::stride], cam.labels()[::stride]
        sun = torch.tensor(shading.sun_vector(), device=surf.device, dtype=torch.float32)
        facing = (lab > 0) & ((surf[..., :3] * sun).sum(-1) > 0)
        case = {"rays": cam.num_rays, "envs_drawn": int(lab.shape[0]), "lit_share": float(((surf[..., 3] > 0) & facing).float().mean()),
                "shadowed_share": float(((surf[..., 3] == 0) & facing).float().mean()), "body_share": float((lab >= 2).float().mean()),
                "nonfinite_rays": int(cam.nonfinite_rays.item()), "iters": iters}
        for k, v in rows.items():
            case[k], case[k + "_range"], case[k + "_all"] = sorted(v)[len(v) // 2], [min(v), max(v)], v
        case["shade_over_rays"] = case["shade_us"] / case["rays_us"]
        out[name] = case
        del cam, rays, shade, surf, lab
        torch.cuda.empty_cache()
    return out


def measure_map_policy(n, terrain, iters, warmup, model, emap, odometry, channels, repeats):
    """the --map --odometry / --map-rows measurement (module docstring)"""
    cfg = C.aliengo_cfg()
    cfg.env.num_envs = n
    cfg.terrain.terrain_proportions = [1.0, 0.0, 0.0, 0.0, 0.0, 0.0] if terrain == "flat" else [0.0, 0.0, 0.0, 0.0, 0.5, 0.5]
    env = LeggedRobot(cfg, sim_device="cuda:0", seed=1)
    env.reset()
    zero = torch.zeros(n, 12, device="cuda:0")
    for _ in range(20):
        env.step_device(zero)
    env.episode_length_buf[:] = 20               # nobody is fresh inside the timed loops
    torch.cuda.synchronize()
    cam = sensors.depth_camera(env, 64, 48, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, near=0.05, far=5.0, see_robot=True, labels=True, model=model)
    cam.refresh(tick=0)
    cam.attach_map(emap, odometry=odometry)
    cam.attach_map_rows(("height", "known")[:channels])
    P = int(cam.stage("map").struct.num_points)
    whole = max(model.period, iters // model.period * model.period)
    rows_buf, scan, known, scale = cam.map_rows(), cam.map_scan(), cam.map_known(), float(env.lcfg.obs_scale_height)
    pose_z = cam.map_pose()[:, 2:3]

    rows_launch = lambda: cam.stage("map_rows").launch(0, 0)

    def rows_torch():
        torch.mul(torch.clamp(pose_z - 0.5 - scan, -1.0, 1.0), scale, out=rows_buf[:, :P])
        if channels == 2:
            rows_buf[:, P:].copy_(known)
    rows_launch()
    want = rows_buf.clone()
    rows_torch()
    same = bool(torch.equal(want, rows_buf))    # every pose and scan value is finite here: the two statements agree to the bit
    rows = {"capture_us": [], "map_rows_us": [], "map_rows_torch_us": [], "update_us": []}
    if odometry is not None:
        rows["odometry_us"] = []
    for _ in range(repeats):
        rows["capture_us"].append(timed_ticks(cam.stage("capture"), whole, warmup))      # the capture alone
        if odometry is not None:
            rows["odometry_us"].append(timed_ticks(cam.stage("odometry"), whole, warmup))
        rows["map_rows_us"].append(timed(rows_launch, whole, warmup))
        rows["map_rows_torch_us"].append(timed(rows_torch, whole, warmup))
        rows["update_us"].append(timed_ticks(cam, whole, warmup))
    out = {"num_envs": n, "terrain": terrain, "rays": cam.num_rays, "scan_points": P, "channels": channels, "columns": int(rows_buf.shape[1]),
           "coverage": float(known.float().mean().item()), "rows_equal_torch_bit_for_bit": same}
    for k, v in rows.items():
        out[k], out[k + "_range"], out[k + "_all"] = sorted(v)[len(v) // 2], [min(v), max(v)], v
    out["map_rows_over_torch"] = out["map_rows_us"] / out["map_rows_torch_us"]
    out["nonfinite"] = int(cam.nonfinite_rays.item()) + int(cam.map_nonfinite.item())
    return out


def measure_foot_scan(n, terrain, iters, warmup, model, emap, feet, repeats):
    """the --foot-scan measurement (module docstring)"""
    cfg = C.aliengo_cfg()
    cfg.env.num_envs = n
    cfg.terrain.terrain_proportions = [1.0, 0.0, 0.0, 0.0, 0.0, 0.0] if terrain == "flat" else [0.0, 0.0, 0.0, 0.0, 0.5, 0.5]
    env = LeggedRobot(cfg, sim_device="cuda:0", seed=1)
    env.reset()
    zero = torch.zeros(n, 12, device="cuda:0")
    for _ in range(20):
        env.step_device(zero)
    env.episode_length_buf[:] = 20               # nobody is fresh inside the timed loops
    torch.cuda.synchronize()
    cams = []
    for channels, kw in ((("foot_height", "foot_known"), {"foot_scan": feet}), (("height", "known"), {})):       # this tree's chain, and the parent's
        cam = sensors.depth_camera(env, 64, 48, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, near=0.05, far=5.0, see_robot=True, labels=True, model=model)
        cam.refresh(tick=0)
        cam.attach_map(emap)
        cam.attach_map_rows(channels, **kw)
        cams.append(cam)
    cam, parent = cams
    truth = sensors.TerrainFootScan(env, feet, ("foot_height", "foot_known"))
    whole = max(model.period, iters // model.period * model.period)
    rows = {k: [] for k in ("capture_us", "map_us", "map_rows_us", "foot_scan_map_us", "foot_scan_terrain_us", "update_us", "update_parent_us")}
    for _ in range(repeats):
        rows["capture_us"].append(timed_ticks(cam.stage("capture"), whole, warmup))
        rows["map_us"].append(timed_ticks(cam.stage("map"), whole, warmup))
        rows["map_rows_us"].append(timed(lambda: parent.stage("map_rows").launch(0, 0), whole, warmup))
        rows["foot_scan_map_us"].append(timed(lambda: cam.stage("foot_rows").launch(0, 0), whole, warmup))
        rows["foot_scan_terrain_us"].append(timed(truth.update, whole, warmup))
        rows["update_parent_us"].append(timed_ticks(parent, whole, warmup))
        rows["update_us"].append(timed_ticks(cam, whole, warmup))
    K = feet.num_points
    out = {"num_envs": n, "terrain": terrain, "rays": cam.num_rays, "points_per_foot": K, "points": 4 * K * n, "columns": int(cam.map_rows().shape[1]),
           "scan_points": int(parent.stage("map").struct.num_points), "coverage": float(cam.foot_known().float().mean().item()),
           "error_ms": float((cam.map_rows()[:, :4 * K] - truth.rows()[:, :4 * K]).square().mean().item())}
    for k, v in rows.items():
        out[k], out[k + "_range"], out[k + "_all"] = sorted(v)[len(v) // 2], [min(v), max(v)], v
    out["foot_scan_over_map_rows"] = out["foot_scan_map_us"] / out["map_rows_us"]
    out["foot_scan_over_map"] = out["foot_scan_map_us"] / out["map_us"]
    out["nonfinite"] = int(cam.nonfinite_rays.item()) + int(cam.map_nonfinite.item()) + int(cam.foot_nonfinite.item()) + int(truth.nonfinite.item())
    return out


def measure_instrument(n, terrain, iters, warmup, model, instrument, repeats):
    """the --instrument measurement (module docstring)"""
    cfg = C.aliengo_cfg()
    cfg.env.num_envs = n
    cfg.terrain.terrain_proportions = [1.0, 0.0, 0.0, 0.0, 0.0, 0.0] if terrain == "flat" else [0.0, 0.0, 0.0, 0.0, 0.5, 0.5]
    env = LeggedRobot(cfg, sim_device="cuda:0", seed=1)
    env.reset()
    zero = torch.zeros(n, 12, device="cuda:0")
    for _ in range(20):
        env.step_device(zero)
    torch.cuda.synchronize()
    no_fov = sensors.InstrumentError(**dict(instrument.record(), fov=0.0))
    makers = {"camera": (lambda **kw: sensors.depth_camera(env, 64, 48, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, near=0.05, far=5.0, see_robot=True,
                                                           labels=True, model=model, **kw), instrument),
              "lidar": (lambda **kw: sensors.lidar(env, 16, 30.0, 360, mount_pos=(0.0, 0.0, 0.15), near=0.05, far=10.0, see_robot=True, labels=True,
                                                   model=model, **kw), no_fov)}
    out = {"num_envs": n, "terrain": terrain, "resetting_envs": int((env.episode_length_buf == 0).sum().item())}
    fill_all = abi.DEFINES["LSIM_SENSOR_FILL_ALL"]
    whole = max(model.period, iters // model.period * model.period)
    rows, nonfinite = {}, 0
    sensors_ = {}
    for name, (make, inst) in makers.items():
        plain, neutral, drawn = make(), make(instrument=inst), make(instrument=inst)
        for s_ in (plain, neutral, drawn):
            s_.refresh(tick=0)                  # `drawn`: draws every env's row once
        rows_ = neutral.instrument_rows().zero_()       # back to the neutral rows {latency, 1, 0, 0, 1, 0, 0, 0}
        rows_[:, 0], rows_[:, 1], rows_[:, 4] = float(model.latency), 1.0, 1.0
        sensors_[name] = (plain, neutral, drawn)
        for k in ("capture", "inst_neutral", "inst_drawn"):
            rows[f"{name}_{k}_us"] = []
    rows["draw_all_fresh_us"], rows["draw_none_fresh_us"] = [], []
    draw = lambda flags: sensors_["camera"][2].stage("instrument").launch(0, flags)
    capture_only = lambda sensor: timed_ticks(sensor.stage("capture"), whole, warmup)     # lsim_sensor_capture_inst on the rows as they are, no draw
    for _ in range(repeats):                    # the draw at tick 0 rewrites the rows refresh(tick=0) drew: the same bits
        for name, (plain, neutral, drawn) in sensors_.items():
            rows[f"{name}_capture_us"].append(timed_ticks(plain, whole, warmup))
            rows[f"{name}_inst_neutral_us"].append(capture_only(neutral))
            rows[f"{name}_inst_drawn_us"].append(capture_only(drawn))
        rows["draw_all_fresh_us"].append(timed(lambda: draw(fill_all), iters, warmup))
        rows["draw_none_fresh_us"].append(timed(lambda: draw(0), iters, warmup))
    for k, v in rows.items():
        out[k], out[k + "_range"], out[k + "_all"] = sorted(v)[len(v) // 2], [min(v), max(v)], v
    for name, (plain, neutral, drawn) in sensors_.items():
        out[f"{name}_neutral_over_capture"] = out[f"{name}_inst_neutral_us"] / out[f"{name}_capture_us"]
        out[f"{name}_drawn_over_capture"] = out[f"{name}_inst_drawn_us"] / out[f"{name}_capture_us"]
        nonfinite += sum(int(s_.nonfinite_rays.item()) for s_ in (plain, neutral, drawn))
    out["nonfinite_rays"] = nonfinite
    return out


def measure(n, terrain, iters, warmup, count_lib, bodies=False, model=None):
    cfg = C.aliengo_cfg()
    cfg.env.num_envs = n
    cfg.terrain.terrain_proportions = [1.0, 0.0, 0.0, 0.0, 0.0, 0.0] if terrain == "flat" else [0.0, 0.0, 0.0, 0.0, 0.5, 0.5]
    env = LeggedRobot(cfg, sim_device="cuda:0", seed=1)
    env.reset()
    zero = torch.zeros(n, 12, device="cuda:0")
    L = env._L
    steps = 20
    L.lsim_set_profiling(env._h, steps)
    for _ in range(steps):
        env.step_device(zero)
    torch.cuda.synchronize()
    ms_a, ms_b, cnt = (ctypes.c_float * steps)(), (ctypes.c_float * steps)(), ctypes.c_int(steps)
    L.lsim_read_profile(env._h, ms_a, ms_b, ctypes.byref(cnt))
    L.lsim_set_profiling(env._h, 0)
    out = {"num_envs": n, "terrain": terrain, "kernel_a_us": 1000.0 * sum(ms_a[:cnt.value]) / max(cnt.value, 1)}
    cam = sensors.depth_camera(env, 64, 48, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, near=0.05, far=5.0)
    lid = sensors.lidar(env, 16, 30.0, 360, mount_pos=(0.0, 0.0, 0.15), near=0.05, far=10.0)
    for name, s in (("camera", cam), ("lidar", lid)):
        us = timed(s.update, iters, warmup)
        rays = n * s.num_rays
        out[name + "_us"] = us
        out[name + "_rays"] = rays
        out[name + "_rays_per_s"] = rays / (us * 1e-6)
        out[name + "_over_kernel_a"] = us / out["kernel_a_us"]
        out[name + "_hit_share"] = float((s.out < s.far * (s.scale if s.scale is not None else 1.0) * 0.999).float().mean().item())
        if count_lib is not None:
            cells, tris, bad = counters(s, count_lib)
            out[name + "_cells_per_ray"], out[name + "_triangles_per_ray"] = cells, tris
        out[name + "_nonfinite_rays"] = int(s.nonfinite_rays.item())
    if bodies:
        camb = sensors.depth_camera(env, 64, 48, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, near=0.05, far=5.0, see_robot=True, labels=True)
        lidb = sensors.lidar(env, 16, 30.0, 360, mount_pos=(0.0, 0.0, 0.15), near=0.05, far=10.0, see_robot=True, labels=True)
        for name, s in (("camera", camb), ("lidar", lidb)):
            us = timed(s.update, iters, warmup)
            out[name + "_bodies_us"] = us
            out[name + "_bodies_over_terrain_only"] = us / out[name + "_us"]
            out[name + "_bodies_over_kernel_a"] = us / out["kernel_a_us"]
            out[name + "_body_share"] = float((s.labels() >= 2).float().mean().item())
            out[name + "_primitives"] = int(s._robots_host[0].num_prims)
            if count_lib is not None:
                prims, cells, tris = counters_bodies(s, count_lib)
                out[name + "_bodies_prims_tested_per_ray"], out[name + "_bodies_cells_per_ray"], out[name + "_bodies_triangles_per_ray"] = prims, cells, tris
            out[name + "_bodies_nonfinite_rays"] = int(s.nonfinite_rays.item())
    if model is not None:
        for name, make in (("camera", lambda m: sensors.depth_camera(env, 64, 48, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, near=0.05, far=5.0,
                                                                       see_robot=True, labels=True, model=m)),
                           ("lidar", lambda m: sensors.lidar(env, 16, 30.0, 360, mount_pos=(0.0, 0.0, 0.15), near=0.05, far=10.0, see_robot=True, labels=True, model=m))):
            for key, m in (("_model", model), ("_model_period1", sensors.SensorModel())):
                s = make(m)
                s.refresh(tick=0)
                whole = max(m.period, iters // m.period * m.period)          # whole periods: every env captures equally often
                us = timed_ticks(s, whole, warmup)
                out[name + key + "_us"] = us
                out[name + key + "_over_bodies"] = us / out[name + "_bodies_us"]
                out[name + key + "_over_kernel_a"] = us / out["kernel_a_us"]
                out[name + key + "_nonfinite_rays"] = int(s.nonfinite_rays.item())
        out["resetting_envs"] = int((env.episode_length_buf == 0).sum().item())      # envs with episode_length 0 are due on every tick: must be 0 here
    out["torch_us"] = None
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--terrains", default="flat,stairs")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-counters", action="store_true")
    ap.add_argument("--bodies", action="store_true", help="also time lsim_raycast_bodies (see_robot=True) on every workload")
    ap.add_argument("--model", default=None, help="also time lsim_sensor_capture with this sensor model, e.g. period=5,stagger=1,latency=1,frames=2,noise=0.01:0.002,dropout=0.02")
    ap.add_argument("--mount-jitter", default=None, help="POS,ROT_DEG: time lsim_sensor_mount_jitter and lsim_sensor_capture on jittered against nominal mounts (needs --model)")
    ap.add_argument("--instrument", default=None, help="latency=LO:HI,noise_gain=LO:HI,depth_scale=S,depth_quad=Q,fov=F: time lsim_sensor_instrument and "
                    "lsim_sensor_capture_inst against lsim_sensor_capture (needs --model)")
    ap.add_argument("--map", default=None, nargs="?", const="default", help="size=G,resolution=RES,source=noisy|clean (any subset): time lsim_elevation_map "
                    "next to lsim_sensor_capture (needs --model)")
    ap.add_argument("--odometry", default=None, nargs="?", const="default", help="scale=S,yaw_per_m=Y,z_per_m=Z,noise=a:b:c (any subset): with --map, time "
                    "lsim_odometry_step next to the capture")
    ap.add_argument("--map-rows", type=int, default=None, choices=(1, 2), help="with --map, time lsim_map_rows with this many channels against its torch statement")
    ap.add_argument("--stereo", default=None, nargs="?", const="default", help="baseline=B,max_disparity=D,window=W,edge_radius=N,edge_rel=E,edge_hole=P,edge_fatten=Q "
                    "(any subset; 'default'): time lsim_sensor_stereo next to the capture it follows (needs --model)")
    ap.add_argument("--shade", default=None, nargs="?", const="default", help="sun=AZ:EL,ambient=A,shadows=0|1,checker=M,... (any subset; 'default'): time "
                    "lsim_sensor_shade next to the lsim_raycast_bodies it follows, on the 128 x 96 chase camera")
    ap.add_argument("--foot-scan", default=None, nargs="?", const="default", help="radii:R/R,counts:C/C,centre:0|1,z_offset:Z (any subset; 'default'): time "
                    "lsim_foot_scan with the map and with the terrain as its source, next to lsim_map_rows and the map's launch")
    ap.add_argument("--parent-lib", default=None, help="with --shade: a liblsim.so of the parent commit, whose lsim_raycast_bodies is timed in the same loops")
    ap.add_argument("--repeats", type=int, default=5, help="--mount-jitter / --instrument / --map / --stereo / --shade: alternating repetitions of every timed loop")
    ap.add_argument("--build-only", action="store_true", help="build the counters variant of the library and exit (no GPU needed)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.mount_jitter:
        if not a.model:
            ap.error("--mount-jitter needs --model")
        pos, rot = (float(v) for v in a.mount_jitter.split(","))
        model, jitter = parse_model(a.model), sensors.MountJitter(pos=pos, rot_deg=rot)
        res = {"tool": "raycast_time --mount-jitter", "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
               "camera": "64x48, hfov 87, pitch 30 down, far 5 m, see_robot", "model": a.model, "mount_jitter": jitter.record(),
               "cases": [measure_mount_jitter(a.num_envs, t, a.iters, a.warmup, model, jitter, a.repeats) for t in a.terrains.split(",")]}
        line = json.dumps(res)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        print(line)
        return
    if a.shade is not None:
        shading = sensors.parse_shading(a.shade)
        # the parent's library has no lsim_sensor_shade: only the entry that is timed is bound
        parent = None if a.parent_lib is None else abi.bind(ctypes.CDLL(os.path.abspath(a.parent_lib)), names=["lsim_raycast_bodies"])
        res = {"tool": "raycast_time --shade", "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
               "shading": shading.record(), "parent_lib": a.parent_lib is not None,
               "cases": [measure_shade(a.num_envs, t, a.iters, a.warmup, shading, a.repeats, parent) for t in a.terrains.split(",")]}
        line = json.dumps(res)
        with open(a.out or os.path.join(ROOT, "profiles", "sensor_shade_time.json"), "w") as f:
            f.write(line + "\n")
        print(line)
        return
    if a.foot_scan is not None:
        model_text = a.model or "period=5,stagger=1"
        model, emap, feet = parse_model(model_text), sensors.parse_elevation_map(a.map or "size=32"), sensors.parse_foot_scan(a.foot_scan)
        res = {"tool": "raycast_time --foot-scan", "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
               "camera": "64x48, hfov 87, pitch 30 down, far 5 m, see_robot, labels", "model": model_text, "map": emap.record(), "foot_scan": feet.record(),
               "cases": [measure_foot_scan(a.num_envs, t, a.iters, a.warmup, model, emap, feet, a.repeats) for t in a.terrains.split(",")]}
        line = json.dumps(res)
        with open(a.out or os.path.join(ROOT, "profiles", "foot_scan_time.json"), "w") as f:
            f.write(line + "\n")
        print(line)
        return
    if a.stereo is not None:
        if not a.model:
            ap.error("--stereo needs --model")
        model, stereo = parse_model(a.model), sensors.parse_stereo(a.stereo)
        res = {"tool": "raycast_time --stereo", "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
               "camera": "64x48, hfov 87, pitch 30 down, far 5 m, see_robot, labels", "model": a.model, "stereo": stereo.record(),
               "cases": [measure_stereo(a.num_envs, t, a.iters, a.warmup, model, stereo, a.repeats) for t in a.terrains.split(",")]}
        line = json.dumps(res)
        with open(a.out or os.path.join(ROOT, "profiles", "sensor_stereo_time.json"), "w") as f:
            f.write(line + "\n")
        print(line)
        return
    if a.map:
        if not a.model:
            ap.error("--map needs --model")
        model, emap = parse_model(a.model), sensors.parse_elevation_map(a.map)
        if a.odometry is not None or a.map_rows is not None:
            odometry = None if a.odometry is None else sensors.parse_odometry(a.odometry)
            channels = a.map_rows or 1
            res = {"tool": "raycast_time --map --odometry --map-rows", "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats,
                   "device": torch.cuda.get_device_name(0), "camera": "64x48, hfov 87, pitch 30 down, far 5 m, see_robot, labels", "model": a.model,
                   "map": emap.record(), "odometry": None if odometry is None else odometry.record(), "channels": channels,
                   "cases": [measure_map_policy(a.num_envs, t, a.iters, a.warmup, model, emap, odometry, channels, a.repeats) for t in a.terrains.split(",")]}
            line = json.dumps(res)
            with open(a.out or os.path.join(ROOT, "profiles", "map_policy_time.json"), "w") as f:
                f.write(line + "\n")
            print(line)
            return
        res = {"tool": "raycast_time --map", "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
               "camera": "64x48, hfov 87, pitch 30 down, far 5 m, see_robot, labels", "model": a.model, "map": emap.record(),
               "cases": [measure_map(a.num_envs, t, a.iters, a.warmup, model, emap, a.repeats) for t in a.terrains.split(",")]}
        line = json.dumps(res)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        print(line)
        return
    if a.instrument:
        if not a.model:
            ap.error("--instrument needs --model")
        from isaacgymloco_amd.learn.evaluate import parse_camera_instrument
        model, instrument = parse_model(a.model), parse_camera_instrument(a.instrument)
        if not isinstance(instrument, sensors.InstrumentError):
            ap.error("--instrument takes ranges, not 'trained' or 'off'")
        res = {"tool": "raycast_time --instrument", "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
               "camera": "64x48, hfov 87, pitch 30 down, far 5 m, see_robot", "lidar": "16x360, vfov 30, far 10 m, see_robot, fov 0", "model": a.model,
               "instrument": instrument.record(),
               "cases": [measure_instrument(a.num_envs, t, a.iters, a.warmup, model, instrument, a.repeats) for t in a.terrains.split(",")]}
        line = json.dumps(res)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        print(line)
        return
    count_lib = None
    if not a.no_counters:
        if hip_build.variant_is_stale(COUNT_LIB):
            hip_build.build_variant(COUNT_LIB, ["-DLS_RAYCAST_COUNTERS"])
        if a.build_only:
            print(COUNT_LIB)
            return
        count_lib = lib.load_path(COUNT_LIB)
    model = parse_model(a.model) if a.model else None
    res = {"tool": "raycast_time", "iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "camera": "64x48, hfov 87, pitch 30 down, far 5 m", "lidar": "16x360, vfov 30, far 10 m", "model": a.model,
           "cases": [measure(a.num_envs, t, a.iters, a.warmup, count_lib, a.bodies or model is not None, model) for t in a.terrains.split(",")]}
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
