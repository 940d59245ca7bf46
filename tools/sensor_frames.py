#!/usr/bin/env python3
"""Third-person depth and label frames of robots on their terrain, without a viewer: a frame="yaw" chase camera (envs/sensors.py, see_robot=True).

    python tools/sensor_frames.py --out frames/ [--task aliengo] [--num-envs 64] [--envs 0,1,2] [--steps 50] [--every 10]
                                  [--checkpoint model.pt] [--width 128] [--height 96] [--terrain stairs]

Steps the env under a checkpoint's actor (learn/policy_io.py's loader) or zero actions; every `--every` steps writes, for each chosen env,
`depth_e<env>_s<step>.npy` (float32 [H, W] z-depth in metres), `labels_e<env>_s<step>.npy` (uint8: 0 nothing, 1 terrain, 2 + b body b) and the
same two as 8-bit PGM (depth: near = white, far = black; labels: spread over the grey range).  A PGM is a text header plus raw bytes.
`--map [size=32,resolution=0.0625,source=clean]`: the robot also carries the forward camera of the vision tasks (64 x 48, 0.3 m ahead, pitched
30 degrees down) with an elevation map (sensors.ElevationMap), and `map_e<env>_s<step>.npy` (float32 [G, G], window order, NaN = unknown)
and `.pgm` (unknown black, then low = dark to high = white over the map's own range) are written next to the frames.
`--stereo [baseline=0.05,edge_hole=0.25,...]` (sensors.parse_stereo): the robot carries that forward camera as a stereo pair
(sensors.StereoArtifacts, see_robot and labels on), and `stereo_e<env>_s<step>.npy` / `.pgm` hold what it reports -- the newest frame with
the occlusion shadows, the minimum range and the depth-edge artefacts, holes at the near end of the grey range -- next to the clean
`front_e<env>_s<step>.npy` / `.pgm`.
`--shade [sun=145:50,ambient=0.35,shadows=1,checker=0.5,...]` (sensors.parse_shading): the chase camera is also shaded (sensors.Shading,
lsim_sensor_shade: surface normals, sun shadows, a colour by label), and `rgb_e<env>_s<step>.ppm` (binary P6) and `.npy` (uint8 [H, W, 3])
are written next to the depth and label frames."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def write_pgm(path, img8):
    """binary PGM (P5) of a uint8 [H, W] array"""
    img8 = np.ascontiguousarray(img8, dtype=np.uint8)
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img8.shape[1], img8.shape[0]))
        f.write(img8.tobytes())


def write_ppm(path, rgb):
    """binary PPM (P6) of a uint8 [H, W, 3] array"""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (rgb.shape[1], rgb.shape[0]))
        f.write(rgb.tobytes())


def depth_to_gray(depth, near, far):
    d = np.clip((np.asarray(depth, np.float64) - near) / (far - near), 0.0, 1.0)
    return np.round(255.0 * (1.0 - d)).astype(np.uint8)


def labels_to_gray(labels):
    lab = np.asarray(labels, np.int64)
    return np.where(lab == 0, 0, np.where(lab == 1, 60, 80 + (lab - 2) * 10)).astype(np.uint8)


def map_to_gray(heights):
    h = np.asarray(heights, np.float64)
    known = ~np.isnan(h)
    if not known.any():
        return np.zeros(h.shape, np.uint8)
    lo, hi = h[known].min(), h[known].max()
    g = 40.0 + 215.0 * (np.where(known, h, lo) - lo) / max(hi - lo, 1e-6)
    return np.where(known, np.round(g), 0).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--task", default="aliengo")
    ap.add_argument("--num-envs", type=int, default=64)
    ap.add_argument("--envs", default="0")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--terrain", choices=("flat", "stairs"), default="stairs")
    ap.add_argument("--width", type=int, default=128)       # width * height <= LSIM_RAYCAST_MAX_RAYS (16384)
    ap.add_argument("--height", type=int, default=96)
    ap.add_argument("--hfov", type=float, default=60.0)
    ap.add_argument("--mount", default="-1.2,0.0,0.7", help="camera position in the yaw frame of the base (behind and above)")
    ap.add_argument("--pitch", type=float, default=28.0)
    ap.add_argument("--far", type=float, default=5.0)
    ap.add_argument("--map", default=None, nargs="?", const="source=clean", help="also write an elevation map: size=G,resolution=RES,source=noisy|clean")
    ap.add_argument("--stereo", default=None, nargs="?", const="default", help="also write the forward camera's frames with stereo artefacts: "
                    "baseline=B,max_disparity=D,window=W,edge_radius=N,edge_rel=E,edge_hole=P,edge_fatten=Q (any subset)")
    ap.add_argument("--shade", default=None, nargs="?", const="default", help="also write the chase camera's shaded colour frames: "
                    "sun=AZ:EL,ambient=A,shadows=0|1,checker=M,checker_gain=G,shadow_bias=B,shadow_far=F (any subset)")
    a = ap.parse_args()
    import torch
    from isaacgymloco_amd.envs import config as C, sensors
    from isaacgymloco_amd.envs.legged_robot import LeggedRobot
    cfg = C.aliengo_cfg() if a.task == "aliengo" else C.robot_cfg(C.mixed_cfg("aliengo", {"aliengo": 0.5, a.task: 0.5})[0], 1)
    cfg.env.num_envs = a.num_envs
    cfg.terrain.terrain_proportions = [1.0, 0.0, 0.0, 0.0, 0.0, 0.0] if a.terrain == "flat" else [0.0, 0.0, 0.0, 0.0, 0.5, 0.5]
    env = LeggedRobot(cfg, sim_device="cuda:0", seed=1)
    cam = env.add_sensor("chase", sensors.depth_camera(env, a.width, a.height, a.hfov, mount_pos=tuple(float(v) for v in a.mount.split(",")),
                                                       pitch_deg=a.pitch, near=0.05, far=a.far, see_robot=True, labels=True, frame="yaw",
                                                       shading=None if a.shade is None else sensors.parse_shading(a.shade)))
    front = None
    if a.map:
        front = env.add_sensor("front", sensors.depth_camera(env, 64, 48, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, near=0.05, far=a.far,
                                                             model=sensors.SensorModel()))
        front.attach_map(sensors.parse_elevation_map(a.map))
    pair = None
    if a.stereo is not None:
        pair = env.add_sensor("stereo", sensors.depth_camera(env, 64, 48, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, near=0.05, far=a.far, see_robot=True,
                                                             labels=True, model=sensors.SensorModel(), stereo=sensors.parse_stereo(a.stereo)))
    env.reset()
    policy = None
    if a.checkpoint:
        from isaacgymloco_amd.learn.policy_io import policy_parts
        policy = policy_parts(env, a.checkpoint, "cuda:0").actor_critic.act_inference
    ids = [int(v) for v in a.envs.split(",")]
    os.makedirs(a.out, exist_ok=True)
    zero = torch.zeros(a.num_envs, 12, device="cuda:0")
    for step in range(1, a.steps + 1):
        with torch.no_grad():
            actions = zero if policy is None else policy(env.get_observations())
        env.step_device(actions)
        if step % a.every == 0 or step == a.steps:
            depth, labels = cam.image().cpu().numpy(), cam.label_image().cpu().numpy()
            rgb = None if a.shade is None else cam.rgb_image().cpu().numpy()
            heights = None if front is None else front.map_heights().cpu().numpy()
            seen = None if pair is None else (pair.frame_images()[:, -1].cpu().numpy(), pair.image().cpu().numpy())
            for e in ids:
                stem = f"e{e}_s{step:04d}"
                for name, img in (() if seen is None else (("stereo", seen[0][e]), ("front", seen[1][e]))):
                    np.save(os.path.join(a.out, f"{name}_{stem}.npy"), img)
                    write_pgm(os.path.join(a.out, f"{name}_{stem}.pgm"), depth_to_gray(img, pair.near, pair.far))
                if heights is not None:
                    np.save(os.path.join(a.out, f"map_{stem}.npy"), heights[e])
                    write_pgm(os.path.join(a.out, f"map_{stem}.pgm"), map_to_gray(heights[e]))
                if rgb is not None:
                    np.save(os.path.join(a.out, f"rgb_{stem}.npy"), rgb[e])
                    write_ppm(os.path.join(a.out, f"rgb_{stem}.ppm"), rgb[e])
                np.save(os.path.join(a.out, f"depth_{stem}.npy"), depth[e])
                np.save(os.path.join(a.out, f"labels_{stem}.npy"), labels[e])
                write_pgm(os.path.join(a.out, f"depth_{stem}.pgm"), depth_to_gray(depth[e], cam.near, cam.far))
                write_pgm(os.path.join(a.out, f"labels_{stem}.pgm"), labels_to_gray(labels[e]))
    print(f"{len(ids)} env(s), frames under {a.out}; non-finite rays: {int(cam.nonfinite_rays)}")


if __name__ == "__main__":
    main()
