"""Range sensors on the terrain mesh and the robot's own collision shapes (include/lsim.h, lsim_raycast / lsim_raycast_bodies): depth cameras and lidar.

    cam = depth_camera(env, 64, 48, hfov_deg=87, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30, near=0.05, far=5.0, see_robot=True, labels=True)
    env.add_sensor("depth", cam)            # from now on every env.step_device() ends with one more launch
    img = env.sensors["depth"].image()      # [N, 48, 64] z-depth in metres, the live device tensor of the latest step
    seg = env.sensors["depth"].label_image()    # [N, 48, 64] uint8: 0 nothing, 1 terrain, 2 + b body b (env.sensors["depth"].body_names[b])

A sensor is one HIP launch over all envs and rays, on the current stream, without host synchronisation; it reads the post-step, post-reset
`root_states` (and `dof_state`), so it is consistent with the observations of the same step.  What is seen: by default (`see_robot=False`) the
terrain only, through lsim_raycast exactly as before.  `see_robot=True` adds the URDF collision primitives of the env's OWN robot (trunk box,
hip and rotor cylinders -- capsules under asset.replace_cylinder_with_capsule --, thigh and calf boxes, foot spheres), posed by forward kinematics
inside the launch (lsim_raycast_bodies); `ignore_bodies` hides bodies by name or index.  A ray that starts inside a shape passes out of it
freely, so a camera mounted inside the trunk box still sees the legs and the ground.  The robots of OTHER envs are never seen.  There is no torch
fall-back: without the library's entry point the constructor raises.

Frames: the sensor frame is the base frame moved by the mount -- x forward, y left, z up, as the reference's base frame; `frame="yaw"` keeps the
base's position and yaw but not its roll and pitch (a gimbal, or with a mount behind and above the robot a chase camera: a third-person depth
frame of the env's robot on its terrain, tools/sensor_frames.py).  A camera looks along its +x; image rows run top to bottom, columns left to
right (row-major, r = row * width + col).

Sensor model (`model=SensorModel(...)`, lsim_sensor_capture): the same launch renders only the envs that are due on the current tick (a
10-30 Hz camera under a 50 Hz policy: `period`, spread over the period by `stagger`), and turns each clean depth into what an instrument
reports -- depth-dependent noise, dropped pixels, clipping, normalisation -- kept as the env's last `frames` captures, `latency` captures
late, refilled inside the launch when the env resets:

    cam = depth_camera(env, 64, 48, 87, ..., model=SensorModel(period=5, stagger=True, latency=1, frames=2, noise=(0.01, 0.002), dropout=0.02, normalise=True))
    env.add_sensor("depth", cam)            # fills every env's history once, then one launch per step_device()
    obs = env.sensors["depth"].frame_images()    # [N, 2, 48, 64], oldest first, live; cam.image() stays the clean depth of the env's latest capture

Encoder (`cam.attach_encoder(learn.depth_encoder.DepthEncoder(48, 64, frames=2).to(device))`, lsim_depth_encode): every capture is followed,
on the same stream and with the same tick and flags, by one more launch that turns the frames of the envs just captured into a latent row;
`cam.latent()` is the live [N, latent_dim] tensor.  Without an attached encoder nothing of this is created or launched.

Mount jitter (`mount_jitter=MountJitter(pos=0.01, rot_deg=(1, 5, 1))`, lsim_sensor_mount_jitter; needs a model): a real camera is mounted with
millimetres and degrees of error, so every env draws its own mount pose when it starts an episode -- uniform offsets of up to `pos` metres
along and up to `rot_deg` degrees about the base x, y, z, around the nominal mount.  One small launch ahead of every capture rewrites the
rows of `cam.mount` of the envs just reset, on the device (nobody on the host learns who reset), so a reset env's frame history is
refilled from its new pose within the same step; `cam.mount_nominal` keeps the nominal poses.  spec() records the jitter and from_spec()
rebuilds it.  Without `mount_jitter` nothing of this is created or launched.

Instrument error (`instrument=InstrumentError(latency=(0, 2), noise_gain=(0.5, 2), depth_scale=0.02, depth_quad=0.005, fov=0.02)`,
lsim_sensor_instrument + lsim_sensor_capture_inst; needs a model): a real unit is not its data sheet, so every env that starts an episode also
draws the instrument's own constants -- how many captures late it is, a factor on the noise, a relative depth error that grows with depth, and
a field of view a little wider or narrower.  One small launch ahead of every capture rewrites the rows of `cam.instrument_rows()` of the envs
just reset, on the device, and the capture is lsim_sensor_capture_inst, which reads them.  spec() records the ranges and from_spec()
rebuilds them.  Without `instrument` nothing of this is created or launched and the capture is lsim_sensor_capture.

Stereo artefacts (`stereo=StereoArtifacts(baseline=0.05)`, lsim_sensor_stereo; a pinhole camera with a model): a stereo pair reports no
depth for what only one of its imagers sees, none below a minimum range, and its matcher loses or smears depth edges.  One launch directly
behind every capture, same stream, tick and flags, rewrites those pixels of the frame history the capture just wrote -- holes read the
model's drop_value, a fattened pixel its foreground's captured value -- so frames(), the encoder, the frame log and a "noisy" map all
see them; `out` / image() stay clean and `cam.stereo_counts()` counts holes and fattened pixels.  spec() records the option and
from_spec() rebuilds it.  Without `stereo` nothing of this is created or launched.

Shaded frames (`shading=Shading(sun=(145, 50))`, lsim_sensor_shade; a camera with see_robot=True, labels=True and no model): what a
person watches -- one launch directly behind the rays finds the surface normal at every hit, casts one shadow ray towards the sun against
the terrain and the env's own robot, and writes a colour per pixel from a palette by label, with a world-anchored checker on the ground.
`cam.rgb_image()` is the live uint8 [N, H, W, 3] frame, `cam.surface()` the normals and the light term.  `chase_camera(env)` is the
viewer's camera: behind and above the robot in the yaw frame, shaded (tools/sensor_frames.py --shade, learn/evaluate.py frames=...).
spec() records the option and from_spec() rebuilds it.  Without `shading` nothing of this is created or launched.

Elevation map (`cam.attach_map(ElevationMap(size=32, resolution=0.0625, source="noisy"))`, lsim_elevation_map; needs a model): what a robot
runs next to, or instead of, a learned terrain memory -- per env a robot-centred grid of heights, filled from the depth points of every
capture with the robot's own pose, which remembers the ground under the trunk after the camera has moved on.  One launch behind every
capture, same stream, tick and flags, inserts the envs just captured and resamples every env's map at the points of the height scan:
`cam.map_scan()` is the live [N, P] tensor in the layout of LSIM_BUF_MEASURED_HEIGHTS, `cam.map_known()` says which points the map
knows.  The map believes in the NOMINAL mount, so a jittered camera bends it as it would on a robot.  Without an attached map nothing of
this is created or launched.

Map fusion (`ElevationMap(..., fusion=MapFusion())`, lsim_elevation_map_fused in lsim_elevation_map's place): a cell is the mean of a
capture's points near its top instead of their biased maximum, the captures are fused by a variance the map keeps per cell, and cells the
camera has left age; `cam.map_variance()` is the live [N, P] variance of map_scan(), `attach_map_rows(("height", "confidence"))`
(lsim_map_rows_fused) the actor's rows with var_ref / (var_ref + variance) as the second block.  Without `fusion` nothing of this exists.
Map clean-up (`ElevationMap(..., cleanup=MapCleanup())`, lsim_elevation_map_cleanup between the capture and the map's launch): a cell the
newest capture's rays pass over, well below the height the map holds, is forgotten; `map_cleared()` counts them per env and episode.
Without `cleanup` nothing of this exists.

Odometry (`cam.attach_map(m, odometry=OdometryError(scale=0.02, yaw_per_m=0.01, z_per_m=0.01, noise=(0.005, 0.002, 0.002)))`,
lsim_odometry_step): a robot does not know where it is, it integrates its steps -- so the map is placed with an ESTIMATED pose that drifts
with the distance travelled, in scale, yaw and height, by biases every env draws when it starts an episode plus a per-step noise.  One
small launch ahead of every capture integrates the step each env took since the last one; the map's launch reads `cam.odometry_pose()`
where it read root_states, and the capture itself goes on reading the true pose: the camera is where the robot is.  Without `odometry`
nothing of this is created or launched and the map reads root_states.

Frame log (`cam.attach_frames_log(steps)`, lsim_sensor_frames_log; needs an encoder): what a PPO gradient into the encoder trains on
(learn/vision.py, end_to_end=True) -- every image a rollout's captures showed the encoder, kept ONCE: one launch behind the capture copies
the frames of the envs just captured into `frames_log()` and writes, per rollout step and env, which row of the log holds the image its
latent came from (`frame_rows()`).  It launches only while a rollout drives it (begin_rollout(), set_frames_log_step()); an evaluation
rollout or an env.reset() between two rollouts finds it idle.  Without it nothing of this is created or launched.

Map rows (`cam.attach_map_rows(channels=("height", "known"))`, lsim_map_rows; needs a map): one launch behind the map's turns its scan into
the rows an actor reads -- the heights relative to the pose the map was given, clipped and scaled exactly as the privileged height scan
is, and optionally which of them the map knows; `cam.map_rows()` is the live [N, channels * P] tensor (learn/map_policy.py).
"""
import ctypes
import math

import numpy as np
import torch

from .. import abi, lib
from . import config


def write_ppm(path, rgb):
    """binary PPM (P6) of a uint8 [H, W, 3] array: a text header plus raw bytes, what every image tool opens"""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError(f"write_ppm: expected [H, W, 3], got {rgb.shape}")
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (rgb.shape[1], rgb.shape[0]))
        f.write(rgb.tobytes())


def quat_from_pitch(pitch_deg):
    """xyzw of a rotation about the base y axis; positive pitch looks DOWN (x forward, z up: a positive rotation about y turns +x towards -z)"""
    h = math.radians(pitch_deg) / 2.0
    return (0.0, math.sin(h), 0.0, math.cos(h))


def pinhole_dirs(width, height, hfov_deg):
    """(dirs [H*W, 3] unit, scale [H*W] = cos to the optical axis) of a pinhole camera with square pixels looking along +x: pixel centres, the
    horizontal field of view spanning the image's full width (edge to edge); the vertical one follows from the aspect ratio"""
    tx = math.tan(math.radians(hfov_deg) / 2.0)
    ys = (1.0 - (2.0 * np.arange(width) + 1.0) / width) * tx                      # left (+y) to right
    zs = (1.0 - (2.0 * np.arange(height) + 1.0) / height) * tx * height / width   # top (+z) to bottom
    v = np.stack((np.ones((height, width)), np.broadcast_to(ys[None, :], (height, width)), np.broadcast_to(zs[:, None], (height, width))), axis=-1)
    n = np.linalg.norm(v, axis=-1, keepdims=True)
    return (v / n).reshape(-1, 3).astype(np.float32), (1.0 / n).reshape(-1).astype(np.float32)


def ring_dirs(channels, vfov_deg, points_per_rev):
    """dirs [channels * points_per_rev, 3] of a spinning lidar: channel c at elevation vfov[0] + c * (vfov[1] - vfov[0]) / (channels - 1) (degrees, up
    positive; one channel: the mean), azimuth k * 360 / points_per_rev counter-clockwise from +x; r = c * points_per_rev + k"""
    lo, hi = (-vfov_deg / 2.0, vfov_deg / 2.0) if np.isscalar(vfov_deg) else vfov_deg
    el = np.radians(np.linspace(lo, hi, channels) if channels > 1 else np.array([(lo + hi) / 2.0]))
    az = 2.0 * np.pi * np.arange(points_per_rev) / points_per_rev
    v = np.stack((np.cos(el)[:, None] * np.cos(az)[None, :], np.cos(el)[:, None] * np.sin(az)[None, :], np.broadcast_to(np.sin(el)[:, None], (channels, points_per_rev))), axis=-1)
    return v.reshape(-1, 3).astype(np.float32)


class _Option:
    """What the options of a range sensor share, from two tables of the class.  FIELDS: the constructor's keywords, each kept as the
    attribute of its name -- the record spec() stores (tuples as lists) and cls(**record) reads, equality (same class, equal records) and
    a one-line repr.  TEXT: the grammar of parse_option -- field -> the converter of a scalar, or (converter, separator, accepted lengths)
    of a list."""
    FIELDS, TEXT = (), {}

    def record(self):
        """the plain dict spec() stores and cls(**record) reads"""
        plain = lambda v: [plain(x) for x in v] if isinstance(v, (tuple, list)) else v
        return {k: plain(getattr(self, k)) for k in self.FIELDS}

    def __eq__(self, other):
        return type(other) is type(self) and self.record() == other.record()

    __hash__ = None

    def _shown(self, k):
        return repr(getattr(self, k))

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(f'{k}={self._shown(k)}' for k in self.FIELDS)})"


def parse_option(cls, text):
    """cls(...) of 'key=value,key=value' (any subset of cls.TEXT, each key once; '' or 'default': the defaults), a list as its numbers
    joined by the field's separator: the text every tool and learn/evaluate.py's command line takes for an option"""
    kw = {}
    for item in ([] if text in ("", "default") else text.split(",")):
        k, eq, v = item.partition("=")
        if not eq or k not in cls.TEXT or k in kw:
            raise ValueError(f"{cls.__name__}: {item!r} is no key=value with a key of {', '.join(cls.TEXT)}, each at most once (got {text!r})")
        how = cls.TEXT[k]
        if callable(how):
            kw[k] = how(v)
            continue
        conv, sep, lengths = how
        vals = tuple(conv(x) for x in v.split(sep))
        if len(vals) not in lengths:
            raise ValueError(f"{cls.__name__}: {k} takes {' or '.join(str(n) for n in lengths)} numbers joined by {sep!r}, got {v!r}")
        kw[k] = vals[0] if len(vals) == 1 else vals
    return cls(**kw)


_flag = lambda v: bool(int(v))
_or_none = lambda conv: lambda v: None if v.lower() == "none" else conv(v)       # a field whose default is "derived": the text 'none' asks for it


class SensorModel(_Option):
    """What lsim_sensor_capture adds to a ray cast (include/lsim.h states every formula).  `period`: an env captures on every period-th
    tick; `stagger`: env e captures when (tick + e) % period == 0 instead of tick % period == 0, so that every launch renders 1 env in
    `period`; `frames`: the captures a policy reads, oldest first; `latency`: how many captures old the newest of them is; `noise` =
    (sigma0, sigma2): standard deviation sigma0 + sigma2 * depth^2 on a hit; `dropout`: probability that a hit reads `drop_value`; `clip` =
    (lo, hi), None: the sensor's (near, far); `normalise`: (v - (lo + hi) / 2) / (hi - lo), in [-0.5, 0.5], instead of v.
    An env that was reset (episode_length 0) captures at once and all its frames are that capture."""
    FIELDS = ("period", "stagger", "latency", "frames", "noise", "dropout", "drop_value", "clip", "normalise")
    TEXT = {"period": int, "stagger": _flag, "latency": int, "frames": int, "noise": (float, ":", (2,)), "dropout": float, "drop_value": float,
            "clip": (float, ":", (2,)), "normalise": _flag}

    def __init__(self, period=1, stagger=False, latency=0, frames=1, noise=(0.0, 0.0), dropout=0.0, drop_value=0.0, clip=None, normalise=False):
        self.period, self.stagger, self.latency, self.frames = int(period), bool(stagger), int(latency), int(frames)
        self.noise = (float(noise[0]), float(noise[1]))
        self.dropout, self.drop_value = float(dropout), float(drop_value)
        self.clip = None if clip is None else (float(clip[0]), float(clip[1]))
        self.normalise = bool(normalise)
        kmax = abi.DEFINES["LSIM_SENSOR_MAX_HISTORY"]
        if self.period < 1 or self.latency < 0 or self.frames < 1 or self.latency + self.frames > kmax:
            raise ValueError(f"SensorModel: period >= 1, latency >= 0, frames >= 1 and latency + frames <= {kmax}")
        if min(self.noise) < 0.0 or not 0.0 <= self.dropout <= 1.0 or (self.clip is not None and not self.clip[0] <= self.clip[1]):
            raise ValueError("SensorModel: noise >= 0, 0 <= dropout <= 1, clip[0] <= clip[1]")

    def offset_gain(self, near, far):
        """((lo, hi), offset, gain) for a sensor with this [near, far]"""
        lo, hi = (near, far) if self.clip is None else self.clip
        if not self.normalise:
            return (lo, hi), 0.0, 1.0
        if not hi > lo:
            raise ValueError("SensorModel: normalise needs clip[0] < clip[1]")
        return (lo, hi), (lo + hi) / 2.0, 1.0 / (hi - lo)


class MountJitter(_Option):
    """Per-episode error of a sensor's mount pose (lsim_sensor_mount_jitter; include/lsim.h states every formula): when an env starts an
    episode its mount is the nominal one moved by uniform offsets in [-pos[k], pos[k]] metres along the base x, y, z and turned by about
    [-rot_deg[k], rot_deg[k]] degrees about the base x, y, z (rot_deg[1] is the pitch error of a forward camera).  A scalar is the same
    half-width on all three axes."""
    FIELDS = ("pos", "rot_deg")
    TEXT = {"pos": (float, "/", (1, 3)), "rot_deg": (float, "/", (1, 3))}

    def __init__(self, pos=(0.0, 0.0, 0.0), rot_deg=(0.0, 0.0, 0.0)):
        self.pos, self.rot_deg = self._three(pos, "pos"), self._three(rot_deg, "rot_deg")

    @staticmethod
    def _three(v, name):
        v = (float(v),) * 3 if np.isscalar(v) else tuple(float(x) for x in v)
        if len(v) != 3 or any(not math.isfinite(x) or x < 0.0 for x in v):
            raise ValueError(f"MountJitter: {name} takes one or three finite half-widths >= 0, got {v}")
        return v


class InstrumentError(_Option):
    """Per-episode error of a sensor's own constants (lsim_sensor_instrument; include/lsim.h states every formula): when an env starts an
    episode it draws `latency` = (lo, hi): its latency in captures, uniform on the integers lo .. hi (None: the model's, for every env;
    hi <= the model's latency, which sizes the history); `noise_gain` = (lo, hi): a uniform factor on the model's noise; `depth_scale` and
    `depth_quad` (1 / m): half-widths of the relative depth error depth_scale + depth_quad * d of a hit at depth d; `fov`: half-width of the
    relative error of the tangent of every ray's angle to the optical axis (0.02: the image is up to 2 % wider or narrower), which needs
    rays that all look forward (a camera, not a lidar)."""
    FIELDS = ("latency", "noise_gain", "depth_scale", "depth_quad", "fov")
    TEXT = {"latency": (int, ":", (2,)), "noise_gain": (float, ":", (2,)), "depth_scale": float, "depth_quad": float, "fov": float}

    def __init__(self, latency=None, noise_gain=(1.0, 1.0), depth_scale=0.0, depth_quad=0.0, fov=0.0):
        self.latency = None if latency is None else (int(latency[0]), int(latency[1]))
        if self.latency is not None and (len(latency) != 2 or self.latency != tuple(latency) or not 0 <= self.latency[0] <= self.latency[1] < abi.DEFINES["LSIM_SENSOR_MAX_HISTORY"]):
            raise ValueError(f"InstrumentError: latency is None or integers 0 <= lo <= hi < {abi.DEFINES['LSIM_SENSOR_MAX_HISTORY']}, got {latency}")
        self.noise_gain = (float(noise_gain[0]), float(noise_gain[1]))
        self.depth_scale, self.depth_quad, self.fov = float(depth_scale), float(depth_quad), float(fov)
        values = self.noise_gain + (self.depth_scale, self.depth_quad, self.fov)
        if len(noise_gain) != 2 or any(not math.isfinite(x) or x < 0.0 for x in values) or self.noise_gain[0] > self.noise_gain[1] or self.fov >= 1.0:
            raise ValueError(f"InstrumentError: finite 0 <= noise_gain[0] <= noise_gain[1], depth_scale >= 0, depth_quad >= 0 and 0 <= fov < 1, got {values}")


class StereoArtifacts(_Option):
    """What a stereo pair does to the image (lsim_sensor_stereo behind the capture; include/lsim.h states every formula).  The image is the
    LEFT imager's; the second one sits `baseline` metres to its right, and a pixel only one of them sees has no depth: to the left of every
    near object lies a band of holes as wide as the disparity difference between foreground and background.  `max_disparity` (pixels;
    None: no limit): a nearer pixel has no match and is a hole too; `window` (columns; None: what the nearest range can shadow, at most
    128): how far an occluder is searched; `max_range` (None: 0.98 far): the largest range that carries a depth; a pixel within
    `edge_radius` (0..3, Chebyshev) of a valid pixel nearer than (1 - `edge_rel`) times its own depth loses its depth with probability
    `edge_hole` and takes that foreground's value with probability `edge_fatten` (the matcher's window smearing the foreground over the edge).
    The defaults are STATED GUESSES: 0.05 m is the baseline of a D435-class camera, and the edge figures are fitted to nothing -- no
    recorded frames of a real camera were at hand."""
    FIELDS = ("baseline", "max_disparity", "window", "max_range", "edge_radius", "edge_rel", "edge_hole", "edge_fatten")
    TEXT = {"baseline": float, "max_disparity": _or_none(float), "window": _or_none(int), "max_range": _or_none(float), "edge_radius": int,
            "edge_rel": float, "edge_hole": float, "edge_fatten": float}

    def __init__(self, baseline=0.05, max_disparity=None, window=None, max_range=None, edge_radius=1, edge_rel=0.05, edge_hole=0.25, edge_fatten=0.25):
        self.baseline, self.edge_rel, self.edge_hole, self.edge_fatten = float(baseline), float(edge_rel), float(edge_hole), float(edge_fatten)
        self.max_disparity = None if max_disparity is None else float(max_disparity)
        self.max_range = None if max_range is None else float(max_range)
        self.window, self.edge_radius = None if window is None else int(window), int(edge_radius)
        wmax = abi.DEFINES["LSIM_STEREO_MAX_WINDOW"]
        values = (self.baseline, self.edge_rel, self.edge_hole, self.edge_fatten)
        if any(not math.isfinite(x) or x < 0.0 for x in values) or self.edge_rel >= 1.0 or self.edge_hole + self.edge_fatten > 1.0:
            raise ValueError(f"StereoArtifacts: finite baseline >= 0, 0 <= edge_rel < 1, edge_hole >= 0, edge_fatten >= 0 and edge_hole + edge_fatten <= 1, got {values}")
        if self.max_disparity is not None and not self.max_disparity > 0.0:
            raise ValueError(f"StereoArtifacts: max_disparity is None or > 0, got {max_disparity}")
        if self.max_range is not None and not (math.isfinite(self.max_range) and self.max_range > 0.0):
            raise ValueError(f"StereoArtifacts: max_range is None or finite and > 0, got {max_range}")
        if (self.window is not None and not 1 <= self.window <= wmax) or not 0 <= self.edge_radius <= 3:
            raise ValueError(f"StereoArtifacts: window is None or 1 .. {wmax} and edge_radius 0 .. 3, got {window}, {edge_radius}")


def parse_stereo(text):
    """a StereoArtifacts of 'baseline=0.05,edge_hole=0.25,window=none,...' ('' or 'default': the defaults): the text the tools take"""
    return parse_option(StereoArtifacts, text)


def _rgb(r, g, b):
    return r | g << 8 | b << 16


def _default_palette():
    """sky, terrain, trunk, then per leg hip / thigh / calf / foot: one hue per kind of body, a little darker from leg to leg"""
    kinds = ((235, 130, 40), (60, 110, 210), (70, 175, 90), (225, 50, 50))          # hip orange, thigh blue, calf green, foot red
    legs = [_rgb(*(int(c * (1.0 - 0.08 * leg)) for c in kinds[k])) for leg in range(4) for k in range(4)]
    return (_rgb(135, 206, 235), _rgb(150, 140, 120), _rgb(205, 205, 210)) + tuple(legs)


def _palette_text(v):
    return None if v.lower() == "none" else tuple(int(x, 16) for x in v.split(":"))


class Shading(_Option):
    """What lsim_sensor_shade adds behind the rays of a camera that sees the robot and labels its pixels (include/lsim.h states every
    formula): a colour per pixel.  `sun` = (azimuth_deg, elevation_deg): where the sun stands, azimuth counter-clockwise from the world
    +x, elevation above the horizon in (0, 90]; `ambient`: the light a surface turned away from the sun, or shadowed, still gets;
    `shadows`: one shadow ray per lit pixel, against the terrain and the env's own robot, over `shadow_far` metres from `shadow_bias`
    metres off the surface; `checker` (metres, 0: none): a world-anchored checker on the terrain whose darker squares are
    `checker_gain` as bright -- what shows motion over flat ground; `palette`: 2 + 17 words r | g << 8 | b << 16 by label (sky,
    terrain, body 0..16), None: one hue each for trunk, hips, thighs, calves and feet.
    The defaults are STATED GUESSES: a mid-afternoon sun behind the robot's left shoulder at spawn yaw 0, and figures chosen for
    frames that read well, fitted to nothing."""
    FIELDS = ("sun", "ambient", "shadows", "checker", "checker_gain", "palette", "shadow_bias", "shadow_far")
    TEXT = {"sun": (float, ":", (2,)), "ambient": float, "shadows": _flag, "checker": float, "checker_gain": float, "palette": _palette_text,
            "shadow_bias": float, "shadow_far": float}

    def __init__(self, sun=(145.0, 50.0), ambient=0.35, shadows=True, checker=0.5, checker_gain=0.8, palette=None, shadow_bias=2e-3, shadow_far=4.0):
        self.sun = (float(sun[0]), float(sun[1]))
        self.ambient, self.shadows, self.checker, self.checker_gain = float(ambient), bool(shadows), float(checker), float(checker_gain)
        self.shadow_bias, self.shadow_far = float(shadow_bias), float(shadow_far)
        self.palette = None if palette is None else tuple(int(w) for w in palette)
        words = 2 + abi.DEFINES["LSIM_NUM_BODIES"]
        if len(sun) != 2 or not all(math.isfinite(x) for x in self.sun) or not 0.0 < self.sun[1] <= 90.0:
            raise ValueError(f"Shading: sun is (azimuth_deg, elevation_deg) with 0 < elevation <= 90, got {sun}")
        values = (self.checker, self.checker_gain, self.shadow_bias, self.shadow_far)
        if not 0.0 <= self.ambient <= 1.0 or any(not math.isfinite(x) or x < 0.0 for x in values):
            raise ValueError(f"Shading: 0 <= ambient <= 1 and finite checker, checker_gain, shadow_bias, shadow_far >= 0, got {(self.ambient,) + values}")
        if self.palette is not None and (len(self.palette) != words or any(not 0 <= w <= 0xFFFFFF for w in self.palette)):
            raise ValueError(f"Shading: palette is None or {words} words r | g << 8 | b << 16 (sky, terrain, body 0..16)")

    def sun_vector(self):
        """the unit vector towards the sun, world frame"""
        az, el = math.radians(self.sun[0]), math.radians(self.sun[1])
        return (math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el))

    def palette_words(self):
        return _default_palette() if self.palette is None else self.palette


def parse_shading(text):
    """a Shading of 'sun=145:50,ambient=0.35,shadows=1,checker=0.5,...' ('' or 'default': the defaults): the text the tools take"""
    return parse_option(Shading, text)


class MapFusion(_Option):
    """A variance per cell of an ElevationMap and the fusion by it (lsim_elevation_map_fused; include/lsim.h states every formula).  Within
    a capture a cell takes the MEAN of the points that lie at most `band` metres below its highest one -- the maximum of k noisy points
    lies about 1.5 sigma above the surface for k = 10, the mean does not -- and over the captures a scalar Kalman filter fuses the means
    by their variances.  `band` (None: 5 sigma at 1.5 m, clipped to [0.02, 0.25]; at most 0.5): a band under about 5 sigma cuts the lower
    tail of the noise off and brings the bias back (one cell, 10 points, sigma 0.02 m, 8 captures: RMS error 0.002 m at 5 sigma, 0.009 m
    at 2.5 sigma, 0.033 m for the plain map).  `noise` = (sigma0, sigma2) (None: the sensor model's): a capture's standard deviation at
    range r is sigma0 + sigma2 * r^2, r^2 = the cell's horizontal distance squared + `camera_height`^2 (None: the nominal mount's z plus
    rewards.base_height_target); its variance is that squared over min(points, `count_cap`) plus `var_floor`.  `var_growth`: what a
    cell's variance gains per tick it is not seen, up to `var_max`.  `gate`: a mean further than this many standard deviations from the
    stored height replaces it instead of being fused (the surface changed; 0: every capture replaces)."""
    FIELDS = ("band", "noise", "var_floor", "var_growth", "gate", "count_cap", "var_max", "camera_height")
    TEXT = {"band": float, "noise": (float, ":", (2,)), "var_floor": float, "var_growth": float, "gate": float, "count_cap": int, "var_max": float,
            "camera_height": float}

    def __init__(self, band=None, noise=None, var_floor=2.5e-5, var_growth=1e-6, gate=3.0, count_cap=4, var_max=0.25, camera_height=None):
        self.band = None if band is None else float(band)
        self.noise = None if noise is None else (float(noise[0]), float(noise[1]))
        self.var_floor, self.var_growth, self.gate, self.var_max = float(var_floor), float(var_growth), float(gate), float(var_max)
        self.count_cap = int(count_cap)
        self.camera_height = None if camera_height is None else float(camera_height)
        values = (self.var_floor, self.var_growth, self.gate, self.var_max) + (() if self.noise is None else self.noise) + \
            (() if self.camera_height is None else (self.camera_height,))
        if any(not math.isfinite(v) or v < 0.0 for v in values) or self.var_floor > self.var_max or self.count_cap < 1:
            raise ValueError(f"MapFusion: noise, var_floor <= var_max, var_growth, gate and camera_height are finite and >= 0 and count_cap >= 1, got {values}, {count_cap}")
        if self.band is not None and not 0.0 <= self.band <= 0.5:
            raise ValueError(f"MapFusion: band is None or in [0, 0.5] metres, got {band}")

    def resolve(self, model_noise, camera_height):
        """the by-value fields of lsim_elevation_map_fused_t, in its order, with the defaults taken from the sensor: (sigma0, sigma2,
        range_z2, band, var_floor, var_growth, var_max, gate2, count_cap)"""
        s0, s2 = model_noise if self.noise is None else self.noise
        h = camera_height if self.camera_height is None else self.camera_height
        z2 = h * h
        band = min(max(5.0 * (s0 + s2 * (1.5 ** 2 + z2)), 0.02), 0.25) if self.band is None else self.band
        return (s0, s2, z2, band, self.var_floor, self.var_growth, self.var_max, self.gate * self.gate, self.count_cap)


def parse_map_fusion(text):
    """MapFusion of 'band:0.1/gate:3/noise:0.01:0.002' (any subset of its fields, key:value joined by '/'; '1', '' or 'default': the
    defaults): the form a fusion takes INSIDE the text of an elevation map, whose own separators are ',' and '='"""
    if text in ("1", "", "default"):
        return MapFusion()
    return parse_option(MapFusion, ",".join(item.replace(":", "=", 1) for item in text.split("/")))


class MapCleanup(_Option):
    """The visibility clean-up of an ElevationMap (lsim_elevation_map_cleanup, one launch between the capture and the map's; include/lsim.h
    states every formula): a cell that at least `min_rays` rays of the newest capture pass over, on their way to ground further away, more
    than `margin` metres below the height the map holds for it is forgotten -- a maximum lifted by noise, a stereo-fattened depth edge or a
    stretch placed with a pose that has since drifted does not stay for the whole episode.  `slope`: metres of allowance per metre of
    horizontal distance from the camera (the pose's pitch and roll error grows with it); `sigma`: standard deviations of a fused map's own
    variance that protect a cell (ignored by a plain map); `end_gap` (metres, None: 1.5 times the map's resolution): how much of a ray's
    end is left out, so that a ray never clears the cells around its own point.
    The defaults are STATED GUESSES, fitted to nothing: 0.05 m is about 2.5 sigma of the default noise at 1.5 m and exceeds what a ray
    gains across one cell of stairs-steep ground (sqrt(2) * resolution * slope)."""
    FIELDS = ("margin", "slope", "sigma", "min_rays", "end_gap")
    TEXT = {"margin": float, "slope": float, "sigma": float, "min_rays": int, "end_gap": _or_none(float)}

    def __init__(self, margin=0.05, slope=0.05, sigma=3.0, min_rays=2, end_gap=None):
        self.margin, self.slope, self.sigma, self.min_rays = float(margin), float(slope), float(sigma), int(min_rays)
        self.end_gap = None if end_gap is None else float(end_gap)
        values = (self.margin, self.slope, self.sigma) + (() if self.end_gap is None else (self.end_gap,))
        if any(not math.isfinite(v) or v < 0.0 for v in values) or self.min_rays < 1:
            raise ValueError(f"MapCleanup: margin, slope, sigma and end_gap are finite and >= 0 and min_rays >= 1, got {values}, {min_rays}")

    def resolve(self, resolution):
        """the by-value fields of lsim_elevation_map_cleanup_t, in its order: (clear_margin, clear_slope, clear_sigma, end_gap, min_rays)"""
        return (self.margin, self.slope, self.sigma, 1.5 * resolution if self.end_gap is None else self.end_gap, self.min_rays)


def parse_map_cleanup(text):
    """MapCleanup of 'margin:0.05/min_rays:2' (any subset of its fields, key:value joined by '/'; '1', '' or 'default': the defaults): the
    form a clean-up takes INSIDE the text of an elevation map, as a fusion does"""
    if text in ("1", "", "default"):
        return MapCleanup()
    return parse_option(MapCleanup, ",".join(item.replace(":", "=", 1) for item in text.split("/")))


class ElevationMap(_Option):
    """A robot-centred height grid per env, fused on the device from a sensor's captures (lsim_elevation_map; include/lsim.h states every
    formula).  `size`: cells per side, 16, 32 or 64; `resolution`: metres per cell (a power of two keeps the cell of a coordinate exact);
    `source`: "noisy" -- the newest capture as the instrument reports it (the newest slot of the frame history, noise, holes and
    calibration error included; with an InstrumentError too: lsim_sensor_capture_inst keeps the newest capture in the history's last slot
    whatever the env's latency, so the combination is supported) -- or "clean" -- the sensor's `out` rows; `max_range`: rays that report
    this range or more are not inserted (None: 0.98 * far, which drops the misses); `points` [P, 2], P <= 256: where the map is sampled,
    in the base-yaw frame (None: the env's measured_points_x x measured_points_y in the order of LSIM_BUF_MEASURED_HEIGHTS);
    `unknown_drop`: a point the map does not know reads the base height minus this (None: the robot's nominal base height,
    rewards.base_height_target of the env's config -- flat ground under a standing robot; on a mixed-robot instance that is ONE height
    for every robot, the first config's: pass the value wanted).
    What attach_map refuses, because the launch cannot be right with it: a sensor with frame="yaw" (the launch places the points with the
    base's full orientation); a see_robot sensor without labels=True (the robot's own legs would be inserted as ground); with "noisy", a
    model whose dropped pixels cannot be told from a range (dropout > 0 with drop_value strictly inside the clip range).
    `fusion` (a MapFusion, or its record): the launch is lsim_elevation_map_fused -- a cell is the mean of a capture's points near its
    top, fused over the captures by a variance the map keeps per cell; None: the plain map, and nothing of that exists.  The record
    carries the key "fusion" only when one is set.
    `cleanup` (a MapCleanup, or its record): lsim_elevation_map_cleanup runs between every capture and the map's launch and forgets the
    cells the camera sees through; None: nothing of that is allocated or launched.  The record carries the key "cleanup" only when one is set."""
    FIELDS = ("size", "resolution", "source", "max_range", "points", "unknown_drop")
    TEXT = {"size": int, "resolution": float, "source": str, "max_range": float, "unknown_drop": float, "fusion": parse_map_fusion,
            "cleanup": parse_map_cleanup}

    def __init__(self, size=32, resolution=0.0625, source="noisy", max_range=None, points=None, unknown_drop=None, fusion=None, cleanup=None):
        self.fusion = MapFusion(**fusion) if isinstance(fusion, dict) else fusion
        if self.fusion is not None and not isinstance(self.fusion, MapFusion):
            raise TypeError(f"ElevationMap: fusion is a MapFusion, its record or None, got {type(fusion).__name__}")
        self.cleanup = MapCleanup(**cleanup) if isinstance(cleanup, dict) else cleanup
        if self.cleanup is not None and not isinstance(self.cleanup, MapCleanup):
            raise TypeError(f"ElevationMap: cleanup is a MapCleanup, its record or None, got {type(cleanup).__name__}")
        self.size, self.resolution, self.source = int(size), float(resolution), str(source)
        self.max_range = None if max_range is None else float(max_range)
        self.unknown_drop = None if unknown_drop is None else float(unknown_drop)
        self.points = None if points is None else [[float(x), float(y)] for x, y in np.asarray(points, dtype=np.float64).reshape(-1, 2)]
        if self.size not in (16, 32, 64) or not (math.isfinite(self.resolution) and self.resolution > 0.0):
            raise ValueError(f"ElevationMap: size is 16, 32 or 64 and resolution finite and > 0, got {size}, {resolution}")
        if self.source not in ("noisy", "clean"):
            raise ValueError(f"ElevationMap: source is 'noisy' or 'clean', got {source!r}")
        if self.max_range is not None and not (math.isfinite(self.max_range) and self.max_range > 0.0):
            raise ValueError(f"ElevationMap: max_range is None or finite and > 0, got {max_range}")
        if self.unknown_drop is not None and not math.isfinite(self.unknown_drop):
            raise ValueError(f"ElevationMap: unknown_drop is None or finite, got {unknown_drop}")
        if self.points is not None and not 1 <= len(self.points) <= abi.DEFINES["LSIM_ELEVATION_MAP_MAX_POINTS"]:
            raise ValueError(f"ElevationMap: 1 to {abi.DEFINES['LSIM_ELEVATION_MAP_MAX_POINTS']} points, got {len(self.points)}")

    def record(self):
        out = super().record()
        if self.fusion is not None:
            out["fusion"] = self.fusion.record()
        if self.cleanup is not None:
            out["cleanup"] = self.cleanup.record()
        return out

    def _shown(self, k):
        return repr(getattr(self, k) if k != "points" or self.points is None else len(self.points))     # the number of points, not the points

    def __repr__(self):
        extra = "".join(f", {k}={v!r}" for k, v in (("fusion", self.fusion), ("cleanup", self.cleanup)) if v is not None)
        return f"{super().__repr__()[:-1]}{extra})"


class OdometryError(_Option):
    """Dead-reckoning error of the pose an elevation map is placed with (lsim_odometry_step; include/lsim.h states every formula).  When an
    env starts an episode it draws three biases, uniform in [-v, v]: `scale`, the relative error of every distance travelled; `yaw_per_m`,
    radians of heading error per metre travelled; `z_per_m`, metres of height error per metre travelled.  `noise` = (pos, yaw, z): the
    half-widths of a uniform error of the same three kinds drawn anew at every step.  All-zero values give the true pose bit for bit."""
    FIELDS = ("scale", "yaw_per_m", "z_per_m", "noise")
    TEXT = {"scale": float, "yaw_per_m": float, "z_per_m": float, "noise": (float, ":", (3,))}

    def __init__(self, scale=0.0, yaw_per_m=0.0, z_per_m=0.0, noise=(0.0, 0.0, 0.0)):
        self.scale, self.yaw_per_m, self.z_per_m = float(scale), float(yaw_per_m), float(z_per_m)
        self.noise = tuple(float(v) for v in noise)
        values = (self.scale, self.yaw_per_m, self.z_per_m) + self.noise
        if len(self.noise) != 3 or any(not math.isfinite(v) or v < 0.0 for v in values):
            raise ValueError(f"OdometryError: scale, yaw_per_m, z_per_m and the three of noise are finite half-widths >= 0, got {values}")

    def ranges(self):
        """the six ranges in the order of lsim_odometry_t"""
        return (self.scale, self.yaw_per_m, self.z_per_m) + self.noise


def parse_odometry(text):
    """OdometryError of 'scale=0.02,yaw_per_m=0.01,z_per_m=0.01,noise=0.005:0.002:0.002' (any subset): the text the tools take"""
    return parse_option(OdometryError, text)


class FootScan(_Option):
    """Where lsim_foot_scan samples around each of the four feet (include/lsim.h states every formula): rings of `counts[i]` points at
    `radii[i]` metres, the first point of every ring on the base-yaw frame's x axis and every other ring turned by half a step, plus the
    foot's own centre when `centre` -- K = sum(counts) + centre points per foot, at most LSIM_FOOT_SCAN_MAX_POINTS, the same pattern for
    every foot, turned with the base's yaw only.  `pattern` (a list of [x, y] offsets in metres) takes the place of the rings; radii,
    counts and centre are then recorded as None.  `z_offset`: subtracted from the foot's height before the terrain's is (a foot's
    centre stands its own radius above the ground it touches).  The feet are placed by forward kinematics from the pose the source is
    given and the joint positions, so a map placed by odometry is sampled where the robot believes its feet to be.
    The defaults are STATED GUESSES, fitted to nothing: three rings of 6, 8 and 10 points at 6, 12 and 20 cm (one, two and three cells of
    the default 6.25 cm map) and the centre, K = 25.  No training run long enough to show that foot scans help on stairs has been made."""
    FIELDS = ("radii", "counts", "centre", "z_offset", "pattern")
    TEXT = {"radii": (float, "/", range(1, 9)), "counts": (int, "/", range(1, 9)), "centre": _flag, "z_offset": float}

    def __init__(self, radii=(0.06, 0.12, 0.20), counts=(6, 8, 10), centre=True, z_offset=0.0, pattern=None):
        self.z_offset = float(z_offset)
        if not math.isfinite(self.z_offset):
            raise ValueError(f"FootScan: z_offset is finite, got {z_offset}")
        if pattern is not None:
            self.radii = self.counts = self.centre = None
            self._pattern = [[float(x), float(y)] for x, y in np.asarray(pattern, dtype=np.float64).reshape(-1, 2)]
        else:
            as_tuple = lambda v, conv: tuple(conv(x) for x in (v if isinstance(v, (tuple, list)) else (v,)))
            self.radii, self.counts, self.centre = as_tuple(radii, float), as_tuple(counts, int), bool(centre)
            if len(self.radii) != len(self.counts) or any(not (math.isfinite(r) and r > 0.0) for r in self.radii) or any(c < 1 for c in self.counts):
                raise ValueError(f"FootScan: as many radii (finite, > 0) as counts (>= 1), got {radii}, {counts}")
            pts = [[0.0, 0.0]] if self.centre else []
            for i, (r, c) in enumerate(zip(self.radii, self.counts)):
                pts += [[r * math.cos(2.0 * math.pi * (k + 0.5 * (i % 2)) / c), r * math.sin(2.0 * math.pi * (k + 0.5 * (i % 2)) / c)] for k in range(c)]
            self._pattern = pts
        if not 1 <= len(self._pattern) <= abi.DEFINES["LSIM_FOOT_SCAN_MAX_POINTS"] or not np.isfinite(np.asarray(self._pattern)).all():
            raise ValueError(f"FootScan: 1 to {abi.DEFINES['LSIM_FOOT_SCAN_MAX_POINTS']} finite points per foot, got {len(self._pattern)}")

    def pattern(self):
        """the [K, 2] table of offsets in the base-yaw frame, metres"""
        return [list(p) for p in self._pattern]

    @property
    def num_points(self):
        return len(self._pattern)

    def record(self):
        out = super().record()
        out["pattern"] = self.pattern() if self.radii is None else None
        return out

    def _shown(self, k):
        return repr(getattr(self, k)) if k != "pattern" else ("None" if self.radii is not None else f"<{self.num_points} points>")


def parse_foot_scan(text):
    """FootScan of 'radii=0.06/0.12,counts=6/8,centre=1,z_offset=0.02' (any subset; '' or 'default': the defaults), or the same with ':'
    for '=' and no other ',' -- 'radii:0.06/0.12,counts:6/8' -- the form it takes behind 'foot_scan=' in a tool's option text"""
    if text in ("1", "", "default"):
        return FootScan()
    return parse_option(FootScan, ",".join(item.replace(":", "=", 1) if "=" not in item else item for item in text.split(",")))


FOOT_CHANNELS = (("foot_height",), ("foot_height", "foot_known"))


def _robot_tables(env):
    """([lsim_raycast_robot per robot of the instance], body names): given by the env (the test doubles), else built from its config"""
    from ..robots.model import build_sensor_table
    tables = getattr(env, "sensor_tables", None)
    if tables is None:
        robots = getattr(env, "robots", None)
        assets = [env.cfg.asset] if robots is None else [config.robot_cfg(env.cfg, k).asset for k in range(len(robots))]
        built = [build_sensor_table(a) for a in assets]
        tables = ([t for t, _ in built], built[0][1])
    return list(tables[0]), list(tables[1])


def _foot_scan_struct(env, api, fs_opt, channels, pose, dev, held):
    """an lsim_foot_scan_t with everything but its source filled -- the robot tables on the device and the host, the pattern, rows [N, C * 4K],
    heights [N, 4K], known [N, 4K] and state, all kept in `held` -- for the sensor's stage "foot_rows" and for TerrainFootScan"""
    if not isinstance(fs_opt, FootScan):
        raise TypeError(f"foot_scan is a FootScan, got {type(fs_opt).__name__}")
    lib.entry(api, "lsim_foot_scan", "the foot scans")
    N, K, C = int(env.num_envs), fs_opt.num_points, len(channels)
    tabs, _ = _robot_tables(env)
    host = (abi.LsimRaycastRobot * len(tabs))(*tabs)
    zeros = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=dev)
    held.update(robots_host=host, robots=torch.from_numpy(np.frombuffer(host, dtype=np.uint8).copy()).to(dev),
                pattern=torch.tensor(fs_opt.pattern(), dtype=torch.float32, device=dev).reshape(K, 2).contiguous(),
                rows=zeros(N, C * 4 * K), heights=zeros(N, 4 * K), known=zeros(N, 4 * K, dtype=torch.uint8), state=zeros(1, dtype=torch.int64))
    fs = abi.LsimFootScan()
    fs.pose, fs.dof_state = pose.data_ptr(), env.dof_state.data_ptr()
    fs.robots, fs.robots_host, fs.num_robots = held["robots"].data_ptr(), ctypes.addressof(host), len(tabs)
    if len(tabs) > 1:
        held["env_robot"] = env.robot_ids.to(device=dev, dtype=torch.uint8).contiguous()
        fs.env_robot = held["env_robot"].data_ptr()
    fs.pattern, fs.rows, fs.heights, fs.known, fs.state = (held[k].data_ptr() for k in ("pattern", "rows", "heights", "known", "state"))
    fs.num_envs, fs.env_stride, fs.num_points, fs.channels = N, 1, K, C
    fs.ld, fs.heights_stride, fs.known_stride = C * 4 * K, 4 * K, 4 * K
    fs.z_offset, fs.scale = fs_opt.z_offset, float(env.lcfg.obs_scale_height)
    return fs


class TerrainFootScan:
    """The TRUE foot scan: lsim_foot_scan with the terrain as its source -- the reference's own height sampler at FootScan's pattern around
    every foot, the feet placed by forward kinematics from env.root_states and env.dof_state.  The input of a privileged teacher
    (learn/scan_policy.py) and the truth an evaluation measures a map's foot rows against.  `channels`: ("foot_height",) or
    ("foot_height", "foot_known") -- the terrain knows every point, the second block is all ones and exists so that the rows have the
    layout of a map's.  Add it with env.add_sensor(name, TerrainFootScan(env, FootScan())): every step then ends with its one launch;
    it launches once when created, so the rows exist before the first step.  `rows()` is the live [N, channels * 4K] tensor in observation
    units (clip(foot z - z_offset - h, -1, 1) * obs_scales.height_measurements), `heights()` the live [N, 4, K] terrain heights,
    `known()` the live uint8 [N, 4, K]."""
    model = None            # env.add_sensor: nothing to refresh, no noise stream

    def __init__(self, env, foot_scan=None, channels=("foot_height",), api=None):
        self.env, self._api = env, api if api is not None else env._L
        self.foot_scan, self.channels = FootScan() if foot_scan is None else foot_scan, tuple(channels)
        if self.channels not in FOOT_CHANNELS:
            raise ValueError(f"TerrainFootScan: channels is ('foot_height',) or ('foot_height', 'foot_known'), got {self.channels}")
        dev = env.root_states.device
        self._held = {}
        fs = self.struct = _foot_scan_struct(env, self._api, self.foot_scan, self.channels, env.root_states, dev, self._held)
        lc = env.lcfg
        fs.source, fs.mesh_type = abi.DEFINES["LSIM_FOOT_SCAN_TERRAIN"], int(lc.mesh_type)
        if fs.mesh_type != 0:
            fs.height_grid, fs.grid_rows, fs.grid_cols = env.height_samples.data_ptr(), int(lc.grid_rows), int(lc.grid_cols)
            fs.horizontal_scale, fs.vertical_scale, fs.border_size = lc.horizontal_scale, lc.vertical_scale, lc.border_size
        self._cuda = bool(env.root_states.is_cuda)
        self.update()

    def update(self, stream=None, tick=None, flags=0):
        """the one launch, on `stream` (default: the env's); tick and flags are a modelled sensor's and mean nothing here.  Returns rows()"""
        stream = stream if stream is not None else (self.env._stream() if self._cuda else None)
        lib.check(self._api.lsim_foot_scan(ctypes.byref(self.struct), stream), what="lsim_foot_scan")
        return self._held["rows"]

    def rows(self):
        return self._held["rows"]

    def heights(self):
        return self._held["heights"].unflatten(1, (4, self.foot_scan.num_points))

    def known(self):
        return self._held["known"].unflatten(1, (4, self.foot_scan.num_points))

    @property
    def nonfinite(self):
        """0-d device tensor: visits of envs whose pose or joints were not finite (their rows are zeros); must stay 0"""
        return self._held["state"][0]


def parse_elevation_map(text):
    """ElevationMap of 'size=32,resolution=0.0625,source=noisy,max_range=3,unknown_drop=0.4' (any subset; '' or 'default': the defaults):
    the text the tools take"""
    return parse_option(ElevationMap, text)


_ORDER = ("rays", "odometry", "mount_jitter", "instrument", "capture", "map", "map_rows", "encoder", "memory")      # a chain's launch order
# launched directly behind the stage named, in this order: the stereo artefacts rewrite what the capture wrote before anybody reads it
# (_ORDER keeps the tuple a test pins); a training buffer's stage is no part of the instrument; the shading reads what the rays just wrote;
# the map's clean-up tests the capture as the artefacts left it against the map of the earlier captures, ahead of the map's own launch
# the foot rows read the map its launch just wrote
_BEHIND = {"shade": "rays", "stereo": "capture", "frames_log": "capture", "map_cleanup": "capture", "foot_rows": "map"}
_LAUNCH_ORDER = tuple(n for o in _ORDER for n in (o,) + tuple(k for k, v in _BEHIND.items() if v == o))
_DEPENDENTS = {"map": ("odometry", "map_rows", "map_cleanup", "foot_rows"), "encoder": ("memory", "frames_log")}                                # who goes with whom
_ABSENT = {"instrument": "instrument error (instrument=InstrumentError(...))", "odometry": "odometry (attach_map(m, odometry=OdometryError(...)))",
           "stereo": "stereo artefacts (stereo=StereoArtifacts(...))", "shade": "shading (shading=Shading(...))", "map": "elevation map (attach_map)", "map_rows": "map rows (attach_map_rows)", "foot_rows": "foot rows (attach_map_rows(('foot_height',), foot_scan=FootScan()))",
           "map_cleanup": "map clean-up (ElevationMap(cleanup=MapCleanup(...)))", "encoder": "encoder (attach_encoder)",
           "memory": "memory (attach_memory)", "frames_log": "frame log (attach_frames_log)"}
_FILL_ALL = abi.DEFINES["LSIM_SENSOR_FILL_ALL"]


class Stage:
    """One launch of a sensor's chain.  `entry`: the name of the entry point it launches; `struct`: its ctypes struct (None: `run`, the
    launch of an encoder or a memory, builds its own); `buffers`: the tensors the stage allocated and nobody else owns, by name;
    `option`: what it was attached with (the MountJitter, the ElevationMap, the encoder ...).  Dropping the stage drops all of them.
    `outer`: the struct the entry point takes when `struct` is a view of its first member (a fused map's lsim_elevation_map_fused_t
    around the lsim_elevation_map_t everybody reads and writes the fields of)."""

    def __init__(self, sensor, name, entry, struct, buffers=None, option=None, run=None, outer=None):
        self.name, self.entry, self.struct, self.option, self.args, self.outer = name, entry, struct, option, (), outer
        self.buffers = {} if buffers is None else buffers
        self._sensor, self._run, self._ticks = sensor, run, hasattr(struct, "tick")
        self._ref = None if struct is None else ctypes.byref(struct if outer is None else outer)

    def launch(self, tick, flags, stream=None):
        """the launch on `stream` (default: the sensor's), with `tick` and `flags` where the entry point takes them"""
        if self._run is not None:
            return self._run(tick, flags, stream)
        if self._ticks:
            self.struct.tick, self.struct.flags = tick, flags
        sensor = self._sensor
        lib.check(getattr(sensor._api, self.entry)(self._ref, *self.args, sensor._stream(stream)), what=self.entry)


def _option(name):
    return property(lambda self: getattr(self._stages.get(name), "option", None), doc=f"what the stage {name!r} was attached with; None without it")


class RaySensor:
    """R rays per env against the terrain.  `dirs` [R, 3] unit vectors in the sensor frame; `mount_pos` (3) / `mount_quat` (4, xyzw): one pose, a
    dict {robot name: pose} for a mixed-robot instance, or one per env ([N, 3] / [N, 4]); `scale` [R] or None; every `env_stride`-th env is
    rendered (the other rows of the output keep their initial value, `far`).  `update()` launches once and returns the live [N, R] tensor.
    `see_robot=True`: the env's own robot is seen too (lsim_raycast_bodies), except the bodies of `ignore_bodies` (names or indices);
    `labels=True` (needs see_robot): `labels()` is the live uint8 [N, R] tensor of what each ray met; `frame`: "base" or "yaw" (module docstring).
    With the defaults nothing of this is allocated and the launch is lsim_raycast.
    `model` (a SensorModel): the launch is lsim_sensor_capture -- `update(tick=...)` renders the envs due on that tick, `frames()` is the live
    [N, frames, R] history, `out` the clean value of each env's latest capture, `refresh()` fills every env's history from the present state,
    `tick` the tick of the last launch and `stream_id` (set by env.add_sensor) what separates the noise of the sensors of one env;
    `attach_encoder(enc)` adds the encoder's launch behind every capture and `latent()` is its live [N, latent_dim] output.
    With `model=None` nothing of this is allocated and the launch is the one above.
    `mount_jitter` (a MountJitter; needs a model): `mount_nominal` keeps the [N, 7] poses given here, `mount` becomes a buffer of its own
    that lsim_sensor_mount_jitter rewrites, ahead of every capture and with its stream, tick and flags, for the envs that start an episode.
    With `mount_jitter=None` `mount` is `mount_nominal` and no such launch is made.
    `instrument` (an InstrumentError; needs a model): `instrument_rows()` is the live [N, 8] tensor of each env's own latency, noise gain,
    depth-scale error and field-of-view factor, which lsim_sensor_instrument rewrites ahead of every capture for the envs that start an
    episode, and the capture is lsim_sensor_capture_inst.  With `instrument=None` there is no such tensor and no such launch.
    `stereo` (a StereoArtifacts; a pinhole camera with a model): lsim_sensor_stereo directly behind every capture rewrites the pixels of the
    frame history a stereo pair has no or a wrong depth for; `set_stereo(opt | None)`, `stereo_counts()` the live [2] int64 of holes and
    fattened pixels.  With `stereo=None` nothing of this is allocated or launched.
    `shading` (a Shading; see_robot and labels, no model): lsim_sensor_shade directly behind the rays writes a colour per pixel and the
    surface normal and light term of every hit; `set_shading(opt | None)`, `rgba()` the live uint8 [N, R, 4] colours (a camera:
    `rgba_image()` / `rgb_image()`), `surface()` the live [N, R, 4].  With `shading=None` nothing of this is allocated or launched.
    `attach_map(m)` (an ElevationMap; needs a model): lsim_elevation_map behind every capture; `map_scan()` / `map_known()` are the live
    [N, P] samples, `map_heights()` a window-ordered copy for people and tools, `map_state()` the three raw arrays.  Without it nothing
    of this is allocated or launched.  `attach_map(m, odometry=OdometryError(...))`: lsim_odometry_step ahead of every capture, and the map
    reads `odometry_pose()` [N, 13] (its state: `odometry_state()` [N, 12]) where it read root_states.  `attach_map_rows(channels)`:
    lsim_map_rows behind the map's launch, `map_rows()` the live [N, channels * P] rows an actor reads.
    `attach_frames_log(steps)` (needs an encoder): lsim_sensor_frames_log directly behind the capture while a rollout drives it
    (begin_rollout(), set_frames_log_step()) -- `frames_log()` keeps every image the rollout's captures showed the encoder once,
    `frame_rows()` [steps, N] says which row each storage row's latent came from.  A training buffer: no part of spec().
    `kind`: the record spec() opens with -- {"kind": "camera", "width", "height"}, {"kind": "lidar", "channels", "points_per_rev"}, None:
    {"kind": "rays"} -- whose numbers are also attributes of the sensor.

    The chain: every launch behind update() is a Stage, kept by name and launched in the order of _ORDER; `chain()` names
    the entry points, `stage(name)` hands one out (None: not attached); without a model it is the one stage "rays".  ONE ray struct, the
    outermost that is launched: `ray_struct` and `bodies_struct` (None in the terrain-only form) are views into it.  `out_rows` /
    `label_rows`: the padded tensors `out` / `labels()` are views of; `history()`: the raw frame history."""

    mount_jitter, instrument, map, odometry, foot_scan = (_option(n) for n in ("mount_jitter", "instrument", "map", "odometry", "foot_rows"))
    map_channels = property(lambda self: self._stages["foot_rows"].channels if "foot_rows" in self._stages else getattr(self._stages.get("map_rows"), "option", None),
                            doc="the channels of the attached map rows or foot rows (only one of the two is attached at a time); None without either")
    encoder, memory, stereo, shading, map_cleanup = _option("encoder"), _option("memory"), _option("stereo"), _option("shade"), _option("map_cleanup")

    def __init__(self, env, dirs, mount_pos=(0.0, 0.0, 0.0), mount_quat=(0.0, 0.0, 0.0, 1.0), near=0.0, far=10.0, scale=None, env_stride=1, api=None,
                 see_robot=False, ignore_bodies=(), labels=False, frame="base", model=None, mount_jitter=None, instrument=None, kind=None, stereo=None, shading=None):
        self.env = env
        self.model = model
        self._api = api if api is not None else env._L
        self.kind = {"kind": "rays"} if kind is None else {k: v if k == "kind" else int(v) for k, v in kind.items()}
        vars(self).update({k: v for k, v in self.kind.items() if k != "kind"})
        if frame not in ("base", "yaw"):
            raise ValueError(f"frame: expected 'base' or 'yaw', got {frame!r}")
        self.see_robot, self.frame = bool(see_robot), frame
        self.body_mask, self.body_names = None, []
        bodies = self.see_robot or frame == "yaw"             # the yaw frame is the new entry point's, with or without bodies
        if (labels or len(tuple(ignore_bodies))) and not self.see_robot:
            raise ValueError("labels / ignore_bodies need see_robot=True")
        rays = "lsim_raycast_bodies" if bodies else "lsim_raycast"
        lib.entry(self._api, rays, "the range sensors")
        if model is not None:
            lib.entry(self._api, "lsim_sensor_capture", "the sensor model")
        dev = env.root_states.device
        N = int(env.num_envs)
        self.dirs = torch.as_tensor(np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3), device=dev).contiguous()
        R = self.num_rays = int(self.dirs.shape[0])
        self.near, self.far, self.env_stride = float(near), float(far), int(env_stride)
        self.scale = None if scale is None else torch.as_tensor(np.ascontiguousarray(scale, dtype=np.float32).reshape(R), device=dev).contiguous()
        self.mount = self.mount_nominal = torch.cat((self._per_env(mount_pos, 3, dev), self._per_env(mount_quat, 4, dev)), dim=1).contiguous()
        stride = (R + 3) // 4 * 4
        self.out_rows = torch.full((N, stride), self.far, dtype=torch.float32, device=dev)
        if self.scale is not None:
            self.out_rows[:, :R] *= self.scale
        self.out, self.label_rows = self.out_rows[:, :R], None
        nbytes, rbytes = ctypes.c_size_t(), ctypes.c_size_t()
        if bodies:
            lib.check(self._api.lsim_raycast_bodies_sizes(ctypes.byref(nbytes), ctypes.byref(rbytes)), what="lsim_raycast_bodies_sizes")
            if rbytes.value != ctypes.sizeof(abi.LsimRaycastRobot):
                raise lib.LsimError("lsim_raycast_robot: the library's layout differs from include/lsim.h; rebuild")
        else:
            lib.check(self._api.lsim_raycast_sizes(ctypes.byref(nbytes)), what="lsim_raycast_sizes")
        self.state = torch.zeros(nbytes.value // 8, dtype=torch.int64, device=dev)
        # the one struct that is launched; the inner ones are views into its memory (with a model and no bodies, sm.rb keeps robots NULL,
        # num_robots 0, flags 0: the terrain-only form)
        top = abi.LsimSensorModel() if model is not None else abi.LsimRaycastBodies() if bodies else abi.LsimRaycast()
        self.bodies_struct = None if not bodies else top.rb if model is not None else top
        rc = self.ray_struct = top.rb.rc if model is not None else top.rc if bodies else top
        lc = env.lcfg
        rc.root_states, rc.mount, rc.dirs = env.root_states.data_ptr(), self.mount.data_ptr(), self.dirs.data_ptr()
        rc.scale = None if self.scale is None else self.scale.data_ptr()
        rc.out, rc.state = self.out_rows.data_ptr(), self.state.data_ptr()
        rc.mesh_type = int(lc.mesh_type)
        if rc.mesh_type != 0:
            rc.mesh = env.buf["terrain_mesh"].data_ptr()
            rc.grid_rows, rc.grid_cols = int(lc.grid_rows), int(lc.grid_cols)
        rc.horizontal_scale, rc.vertical_scale, rc.border_size = lc.horizontal_scale, lc.vertical_scale, lc.border_size
        rc.num_envs, rc.num_rays, rc.env_stride, rc.out_stride = N, R, self.env_stride, stride
        rc.near, rc.far = self.near, self.far
        self._stages, self._chain, self._spare = {}, (), {}
        if bodies:
            self._setup_bodies(self.bodies_struct, ignore_bodies, labels, dev)
        if model is None:
            self._attach(Stage(self, "rays", rays, top))
        else:
            self._setup_model(top, model, dev)
        if mount_jitter is not None:
            self.set_mount_jitter(mount_jitter)
        if instrument is not None:
            self.set_instrument(instrument)
        if stereo is not None:
            self.set_stereo(stereo)
        if shading is not None:
            self.set_shading(shading)

    # ---- the chain
    def chain(self):
        """the entry points update() launches, in launch order"""
        return tuple(s.entry for s in self._chain)

    def stage(self, name):
        """the Stage `name` (one of _ORDER), or None when it is not attached"""
        return self._stages.get(name)

    def _need(self, name):
        if name not in self._stages:
            raise ValueError(f"the sensor has no {_ABSENT[name]}")
        return self._stages[name]

    # the private names of before the chain, read-only, for scripts outside the repository that reached them (nothing inside does, DESIGN.md
    # 7.17): name -> (stage, what of it); None while the stage is not attached, as the fields were
    _BEFORE = {"_mj": ("mount_jitter", "struct"), "_si": ("instrument", "struct"), "_inst": ("instrument", "inst"), "_em": ("map", "struct"),
               "_map": ("map", "buffers"), "_od": ("odometry", "struct"), "_odo": ("odometry", "buffers"), "_mr": ("map_rows", "struct"),
               "_rows": ("map_rows", "rows"), "_encoder": ("encoder", "option"), "_memory": ("memory", "option"), "_memory_h": ("memory", "h"),
               "_memory_rows": ("memory", "rows"), "_sm": ("capture", "struct"), "_hist": ("capture", "hist")}
    _BEFORE_FIXED = {"_rc": "ray_struct", "_rb": "bodies_struct", "_out": "out_rows", "_labels": "label_rows"}

    def __getattr__(self, name):            # reached only for a name the object does not have
        stages = self.__dict__.get("_stages")
        if stages is not None and name in self._BEFORE:
            owner, what = self._BEFORE[name]
            if owner in stages:
                return getattr(stages[owner], what) if hasattr(stages[owner], what) else stages[owner].buffers[what]
            if owner != "capture":          # _sm and _hist did not exist without a model, _rb not without bodies
                return None
        elif stages is not None and name == "_latent":
            return self._latent_held().get("latent")
        elif name in self._BEFORE_FIXED and (name != "_rb" or self.__dict__.get("bodies_struct") is not None):
            return getattr(self, self._BEFORE_FIXED[name])
        raise AttributeError(f"{type(self).__name__!r} object has no attribute {name!r}")

    def _attach(self, stage):
        """`stage` joins the chain, in place of the one of its name.  What every stage has in common with the capture -- who starts an
        episode, the noise stream, the envs visited -- is written here, into the fields its struct has"""
        if stage.struct is not None and stage.name not in ("rays", "capture"):
            cap = self._stages.get("capture")           # none behind plain rays: the shading, which has none of its fields
            for src, fields in ((getattr(cap, "struct", None), ("episode_length", "seed", "rank", "stream_id")), (self.ray_struct, ("num_envs", "env_stride"))):
                for f in fields:
                    if src is not None and hasattr(stage.struct, f):
                        setattr(stage.struct, f, getattr(src, f))
        self._stages[stage.name] = stage
        self._rebuild()
        return stage

    def _drop(self, name):
        """the stage `name` leaves the chain and with it its struct, its buffers and the stages that need it"""
        for n in (name,) + _DEPENDENTS.get(name, ()):
            self._stages.pop(n, None)
        self._rebuild()

    def _rebuild(self):
        cap, inst = self._stages.get("capture"), self._stages.get("instrument")
        if cap is not None:                 # the capture that reads the instrument's rows, or the plain one
            cap.entry, cap.args = ("lsim_sensor_capture", ()) if inst is None else ("lsim_sensor_capture_inst", (inst.buffers["inst"].data_ptr(),))
        if "stereo" in self._stages:        # the artefacts follow the instrument's focal length and latency, or the model's own
            self._stages["stereo"].struct.inst = None if inst is None else inst.buffers["inst"].data_ptr()
        self._chain = tuple(self._stages[n] for n in _LAUNCH_ORDER if n in self._stages)

    def _kept(self, name, make):
        """the buffers the stage `name` holds already (set again: what was drawn so far stays), else make()"""
        return self._stages[name].buffers if name in self._stages else make()

    def _zeros(self, *shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype, device=self.out_rows.device)

    def set_instrument(self, instrument):
        """`instrument` (an InstrumentError) from now on, or None: back to lsim_sensor_capture, no launch and no rows.  Until the next
        refresh() (every env) or, env by env, until episodes start, the rows are the neutral ones: the model's own constants"""
        if instrument is None:
            return self._drop("instrument")
        if not isinstance(instrument, InstrumentError):
            raise TypeError(f"instrument: expected an InstrumentError or None, got {type(instrument).__name__}")
        if self.model is None:
            raise ValueError("instrument needs a model (SensorModel): the latency, the noise and the history it varies are the model's")
        lat = (self.model.latency, self.model.latency) if instrument.latency is None else instrument.latency
        if lat[1] > self.model.latency:
            raise ValueError(f"instrument: latency {instrument.latency} exceeds the model's latency {self.model.latency}, which sizes the history")
        if instrument.fov > 0.0 and bool((self.dirs[:, 0] <= 0.0).any()):
            raise ValueError("instrument: fov > 0 needs rays that all look forward (dirs[:, 0] > 0): a ray at or behind the image plane has no tangent to scale")
        for need in ("lsim_sensor_instrument", "lsim_sensor_capture_inst"):
            lib.entry(self._api, need, "the instrument error")

        def neutral():
            rows = self._zeros(int(self.env.num_envs), 8)
            rows[:, 0], rows[:, 1], rows[:, 4] = float(self.model.latency), 1.0, 1.0
            return {"inst": rows}
        buffers = self._kept("instrument", neutral)
        si = abi.LsimSensorInstrument()
        si.inst = buffers["inst"].data_ptr()
        si.lat_lo, si.lat_hi = lat
        si.gain_lo, si.gain_hi = instrument.noise_gain
        si.scale_range, si.quad_range, si.fov_range = instrument.depth_scale, instrument.depth_quad, instrument.fov
        self._attach(Stage(self, "instrument", "lsim_sensor_instrument", si, buffers, instrument))

    def instrument_rows(self):
        """live [N, 8] tensor: row e = {latency, noise gain, depth_scale, depth_quad, tan_scale, 0, 0, 0} of env e (instrument=...)"""
        return self._need("instrument").buffers["inst"]

    def _holes_tellable(self, who, source, stereo):
        """the map's rule for source="noisy": a hole -- a dropped pixel or a stereo artefact -- must read as a clamped value, never as a range"""
        sm = self._stages["capture"].struct
        clip_lo, clip_hi = float(sm.clip_lo), float(sm.clip_hi)
        drop = min(max(float(sm.drop_value), clip_lo), clip_hi)
        if source == "noisy" and (float(sm.p_drop) > 0.0 or stereo is not None) and clip_lo < drop < clip_hi:
            raise ValueError(f"{who}: source='noisy' with dropout or stereo artefacts needs a drop_value at or beyond a clip limit; {drop} lies inside "
                             f"({clip_lo}, {clip_hi}) and a dropped pixel could not be told from a range")

    def _tan_half_hfov(self):
        """the tangent of half the horizontal field of view of a pinhole camera: from hfov_deg, or from the recorded rays (pinhole_dirs' layout)"""
        if getattr(self, "hfov_deg", None) is not None:
            return math.tan(math.radians(self.hfov_deg) / 2.0)
        d = self.dirs[0].cpu().double()
        return float(d[1] / d[0]) / (1.0 - 1.0 / self.width)

    def set_stereo(self, stereo):
        """`stereo` (a StereoArtifacts) from now on, or None: no launch and no buffers.  It applies from the next capture: nothing is
        launched here, whatever the sensor has captured before"""
        if stereo is None:
            return self._drop("stereo")
        if not isinstance(stereo, StereoArtifacts):
            raise TypeError(f"stereo: expected a StereoArtifacts or None, got {type(stereo).__name__}")
        if self.model is None:
            raise ValueError("stereo needs a model (SensorModel): the artefacts are written into the model's frame history")
        if self.kind["kind"] != "camera" or self.scale is None or self.width < 2:
            raise ValueError("stereo needs a pinhole depth camera at least two columns wide (depth_camera): a lidar has no second imager")
        for need in ("lsim_sensor_stereo", "lsim_sensor_stereo_sizes"):
            lib.entry(self._api, need, "the stereo artefacts")
        W, H, lds = self.width, self.height, ctypes.c_size_t()
        if self._api.lsim_sensor_stereo_sizes(W, H, ctypes.byref(lds)) != 0:
            raise ValueError(f"stereo: a {W} x {H} image needs more LDS than lsim_sensor_stereo has ({abi.DEFINES['LSIM_STEREO_MAX_LDS_BYTES']} bytes)")
        if "map" in self._stages:
            self._holes_tellable("set_stereo", self.map.source, stereo)
        buffers = self._kept("stereo", lambda: {"state": self._zeros(2, dtype=torch.int64), "inv_scale": (1.0 / self.scale).contiguous()})
        sm, inv = self._stages["capture"].struct, buffers["inv_scale"]
        st = abi.LsimSensorStereo()
        st.depth, st.depth_stride, st.inv_scale, st.state = self.out_rows.data_ptr(), self.out_rows.shape[1], inv.data_ptr(), buffers["state"].data_ptr()
        if self.label_rows is not None:
            st.labels, st.label_stride = self.label_rows.data_ptr(), self.label_rows.shape[1]
        for f in ("hist", "hist_stride", "latency", "frames", "period", "stagger", "drop_value", "clip_lo", "clip_hi", "offset", "gain"):
            setattr(st, f, getattr(sm, f))
        st.width, st.height = W, H
        fb = (W / 2.0) / self._tan_half_hfov() * stereo.baseline
        nearest = self.near * float(self.scale.min())               # the smallest z-depth the camera reports
        widest = math.ceil(fb / nearest) + 1 if nearest > 0.0 and math.isfinite(fb / nearest) else abi.DEFINES["LSIM_STEREO_MAX_WINDOW"]
        st.fb = fb
        st.window = max(1, min(W - 1, abi.DEFINES["LSIM_STEREO_MAX_WINDOW"], widest) if stereo.window is None else min(stereo.window, W - 1))
        st.max_disparity = float(np.finfo(np.float32).max) if stereo.max_disparity is None else stereo.max_disparity
        st.t_lo = self.near * float(inv.max())
        st.t_hi = (0.98 * self.far if stereo.max_range is None else stereo.max_range) * float(inv.min())
        if not st.t_lo < st.t_hi:
            raise ValueError(f"stereo: no range is left between near ({st.t_lo}) and max_range ({st.t_hi})")
        st.edge_radius, st.edge_rel, st.p_edge_hole = stereo.edge_radius, stereo.edge_rel, stereo.edge_hole
        st.p_edge_cum = min(float(np.float32(stereo.edge_hole) + np.float32(stereo.edge_fatten)), 1.0)
        self._attach(Stage(self, "stereo", "lsim_sensor_stereo", st, buffers, stereo))

    def stereo_counts(self):
        """live [2] int64 tensor: the holes written and the pixels fattened so far (stereo=...)"""
        return self._need("stereo").buffers["state"]

    def set_shading(self, shading):
        """`shading` (a Shading) from now on, or None: no launch and no buffers.  One launch directly behind the rays, which reads the
        range and the label they just wrote; it applies from the next update()"""
        if shading is None:
            return self._drop("shade")
        if not isinstance(shading, Shading):
            raise TypeError(f"shading: expected a Shading or None, got {type(shading).__name__}")
        if self.label_rows is None:
            raise ValueError("shading needs see_robot=True and labels=True: the colour of a pixel is the colour of what its label names")
        if self.model is not None:
            raise ValueError("shading takes no model (SensorModel): an env that is not due would be shaded from a stale range under a fresh pose")
        for need in ("lsim_sensor_shade", "lsim_sensor_shade_sizes"):
            if not hasattr(self._api, need):
                raise ValueError(f"shading: the loaded library has no {need}; rebuild it (there is no torch fall-back for the shaded frames)")
        nbytes, pbytes = ctypes.c_size_t(), ctypes.c_size_t()
        lib.check(self._api.lsim_sensor_shade_sizes(ctypes.byref(nbytes), ctypes.byref(pbytes)), what="lsim_sensor_shade_sizes")
        words = shading.palette_words()
        if pbytes.value != 4 * len(words):
            raise lib.LsimError("lsim_sensor_shade: the library's palette differs from include/lsim.h; rebuild")
        N, R = int(self.env.num_envs), self.num_rays
        stride = (R + 3) // 4 * 4
        buffers = self._kept("shade", lambda: {"rgba": self._zeros(N, 4 * stride, dtype=torch.uint8), "surface": self._zeros(N, R, 4)})
        buffers["palette"] = torch.tensor(words, dtype=torch.int32, device=self.out_rows.device)
        ss = abi.LsimSensorShade()
        ctypes.memmove(ctypes.addressof(ss.rb), ctypes.addressof(self.bodies_struct), ctypes.sizeof(abi.LsimRaycastBodies))
        ss.rgba, ss.surface, ss.palette, ss.rgba_stride = buffers["rgba"].data_ptr(), buffers["surface"].data_ptr(), buffers["palette"].data_ptr(), stride
        sun = np.asarray(shading.sun_vector(), np.float32)
        for k in range(3):
            ss.sun[k] = float(sun[k])
        ss.ambient, ss.checker, ss.checker_gain = shading.ambient, shading.checker, shading.checker_gain
        ss.shadow_bias, ss.shadow_far = shading.shadow_bias, shading.shadow_far
        ss.shade_flags = abi.DEFINES["LSIM_SHADE_SHADOWS"] if shading.shadows else 0
        self._attach(Stage(self, "shade", "lsim_sensor_shade", ss, buffers, shading))

    def rgba(self):
        """live uint8 [N, R, 4] view of the colour words of the latest launch: red, green, blue, 255 (shading=...)"""
        return self._need("shade").buffers["rgba"][:, :4 * self.num_rays].unflatten(1, (self.num_rays, 4))

    def surface(self):
        """live [N, R, 4] tensor of the latest launch: the unit surface normal at every hit, world frame, and the light term 0 / 1; zeros
        where nothing is hit (shading=...)"""
        return self._need("shade").buffers["surface"]

    def set_mount_jitter(self, jitter):
        """`jitter` (a MountJitter) from now on, or None: back to the nominal mount and no launch.  The new poses are drawn by the next
        refresh() (every env) or, env by env, as episodes start"""
        if jitter is None:
            self._drop("mount_jitter")
            return self._point_mount(self.mount_nominal)
        if not isinstance(jitter, MountJitter):
            raise TypeError(f"mount_jitter: expected a MountJitter or None, got {type(jitter).__name__}")
        if self.model is None:
            raise ValueError("mount_jitter needs a model (SensorModel): the tick and the episode lengths that say who starts an episode are the model's")
        lib.entry(self._api, "lsim_sensor_mount_jitter", "the mount jitter")
        buffers = self._kept("mount_jitter", lambda: {"mount": self.mount_nominal.clone()})
        self._point_mount(buffers["mount"])
        mj = abi.LsimSensorMountJitter()
        mj.nominal, mj.mount = self.mount_nominal.data_ptr(), self.mount.data_ptr()
        for k in range(3):
            mj.pos_range[k], mj.rot_range[k] = jitter.pos[k], math.radians(jitter.rot_deg[k])
        self._attach(Stage(self, "mount_jitter", "lsim_sensor_mount_jitter", mj, buffers, jitter))

    def _point_mount(self, mount):
        """`mount` is what every launch of this sensor reads from now on"""
        self.mount = mount
        self.ray_struct.mount = mount.data_ptr()

    def _setup_model(self, sm, model, dev):
        """the lsim_sensor_model fields around the ray struct, and the history: the stage "capture" """
        env = self.env
        self._episode_length = env.episode_length_buf
        sm.episode_length = self._episode_length.data_ptr()
        K, stride = model.latency + model.frames, self.out_rows.shape[1]
        hist = self._zeros(int(env.num_envs), K, stride)
        sm.hist, sm.hist_stride = hist.data_ptr(), stride
        sm.seed, sm.rank, sm.stream_id = int(env.lcfg.seed), int(env.lcfg.rank), 0
        sm.period, sm.stagger, sm.latency, sm.frames = model.period, int(model.stagger), model.latency, model.frames
        sm.sigma0, sm.sigma2 = model.noise
        sm.p_drop, sm.drop_value = model.dropout, model.drop_value
        (sm.clip_lo, sm.clip_hi), sm.offset, sm.gain = model.offset_gain(self.near, self.far)
        self._attach(Stage(self, "capture", "lsim_sensor_capture", sm, {"hist": hist}, model))
        self.tick = -1

    @property
    def stream_id(self):
        return int(self._stages["capture"].struct.stream_id) if self.model is not None else 0

    @stream_id.setter
    def stream_id(self, value):
        for s in self._chain:
            if hasattr(s.struct, "stream_id"):
                s.struct.stream_id = int(value)

    @property
    def episode_length_ptr(self):
        """the address of the env's episode lengths, as the capture reads them (a model only)"""
        return self._stages["capture"].struct.episode_length

    def _setup_bodies(self, rb, ignore_bodies, labels, dev):
        """the lsim_raycast_bodies fields around the ray struct: one sensor table per robot of the instance, on the device and (for the argument check) on the host"""
        env = self.env
        tabs, self.body_names = _robot_tables(env)
        if not self.see_robot:
            tabs = [abi.LsimRaycastRobot.from_buffer_copy(t) for t in tabs]
            for t in tabs:
                t.num_prims = 0
        self._robots_host = (abi.LsimRaycastRobot * len(tabs))(*tabs)
        raw = np.frombuffer(self._robots_host, dtype=np.uint8).copy()
        self._robots_dev = torch.from_numpy(raw).to(dev)
        mask = (1 << abi.DEFINES["LSIM_NUM_BODIES"]) - 1
        for b in ignore_bodies:
            if isinstance(b, str):
                hit = [i for i, n in enumerate(self.body_names) if n == b] or [i for i, n in enumerate(self.body_names) if b in n]
                if not hit:
                    raise ValueError(f"ignore_bodies: no body named {b!r} (bodies: {self.body_names})")
            else:
                hit = [int(b)]
                if not 0 <= hit[0] < abi.DEFINES["LSIM_NUM_BODIES"]:
                    raise ValueError(f"ignore_bodies: body index {b} out of range")
            for i in hit:
                mask &= ~(1 << i)
        self.body_mask = mask
        rb.dof_state = env.dof_state.data_ptr()
        rb.robots = self._robots_dev.data_ptr()
        rb.robots_host = ctypes.addressof(self._robots_host)
        rb.num_robots = len(tabs)
        if len(tabs) > 1:
            self._env_robot = env.robot_ids.to(device=dev, dtype=torch.uint8).contiguous()
            rb.env_robot = self._env_robot.data_ptr()
        rb.body_mask = mask
        rb.flags = abi.RAYCAST_FRAME_YAW if self.frame == "yaw" else 0
        if labels:
            self.label_rows = self._zeros(int(env.num_envs), (self.num_rays + 3) // 4 * 4, dtype=torch.uint8)
            rb.labels, rb.label_stride = self.label_rows.data_ptr(), self.label_rows.shape[1]

    def _per_env(self, pose, width, dev):
        N = int(self.env.num_envs)
        if isinstance(pose, dict):
            names = getattr(self.env, "robot_names", None)
            if names is None:
                raise ValueError("a {robot name: pose} mount needs a mixed-robot instance (config.mixed_cfg)")
            missing = [n for n in names if n not in pose]
            if missing:
                raise ValueError(f"no mount for robots {missing}")
            table = torch.tensor([list(pose[n]) for n in names], dtype=torch.float32, device=dev).reshape(len(names), width)
            return table[self.env.robot_ids.to(dev)]
        p = torch.as_tensor(pose, dtype=torch.float32, device=dev)
        if p.shape == (width,):
            return p.unsqueeze(0).expand(N, width)
        if p.shape == (N, width):
            return p
        raise ValueError(f"mount: expected ({width},), ({N}, {width}) or a dict by robot name, got {tuple(p.shape)}")

    def _stream(self, stream):
        if stream is not None:
            return stream
        return self.env._stream() if self.out_rows.is_cuda else None

    def update(self, stream=None, tick=None, flags=0):
        """the chain's launches on `stream` (default: the current one), no host synchronisation; returns the live [N, R] tensor.  With a
        model: the envs due on `tick` (default: the env's common_step_counter), `flags` = 0 or one of LSIM_SENSOR_FILL_ALL /
        LSIM_SENSOR_RESETS_ONLY, the same for every stage; without one both are ignored"""
        if self.model is not None:
            tick = self.tick = int(getattr(self.env, "common_step_counter", 0)) if tick is None else int(tick)
        tick, flags = tick or 0, int(flags)
        for s in self._chain:
            s.launch(tick, flags, stream)
        return self.out

    def refresh(self, stream=None, tick=None):
        """capture every env now and fill its whole history with that capture (a model only)"""
        if self.model is None:
            raise ValueError("the sensor was created without a model")
        return self.update(stream, tick, _FILL_ALL)

    def history(self):
        """live raw [N, latency + frames, stride] tensor: the frame history as the capture keeps it, padded rows and all (a model only)"""
        if self.model is None:
            raise ValueError("the sensor was created without a model")
        return self._stages["capture"].buffers["hist"]

    def frames(self):
        """live [N, frames, R] view of the history: what the model reports, oldest first; the last one is `latency` captures old"""
        return self.history()[:, :self.model.frames, :self.num_rays]

    def attach_encoder(self, enc):
        """from now on every update() / refresh() is followed by `enc`'s launch (learn.depth_encoder.DepthEncoder.encode_device) on the same
        stream with the same tick and flags; encodes every env once now, from the present history, when the sensor has captured before.
        None: detach, the latent and an attached memory with it"""
        if enc is None:
            return self._drop("encoder")
        if self.model is None:
            raise ValueError("attach_encoder: the sensor was created without a model, so it has no frame history to encode")
        buffers, self._spare = self._kept("encoder", lambda: self._spare), {}       # the latent of an encoder launched by hand, if any
        stage = self._attach(Stage(self, "encoder", "lsim_depth_encode", None, buffers, enc, run=lambda tick, flags, stream: enc.encode_device(self, tick, flags, stream)))
        if self.tick >= 0:
            stage.launch(self.tick, _FILL_ALL)
        return enc

    def attach_map(self, m, odometry=None):
        """from now on every update() / refresh() is followed by lsim_elevation_map on the same stream with the same tick and flags (`m`: an
        ElevationMap, or None: detach and free, odometry and map rows included).  Inserts every env once now, from the present rows, when
        the sensor has captured before.  `odometry` (an OdometryError): the map is placed with the estimated pose of lsim_odometry_step,
        enqueued ahead of every capture for every visited env (and once now, every env fresh, when the sensor has captured before); None:
        the map reads root_states and no such launch is made.
        "noisy" reads the newest slot of the frame history with (a, b) = (1 / gain, offset), "clean" the `out` rows with (1, 0); the
        labels are passed when the sensor has them (only terrain is ground); the assumed mount is `mount_nominal`.
        Which ranges are points: above `near` and below max_range (None: 0.98 far) -- and for "noisy", whose values the model clamps to
        [clip_lo, clip_hi], misses and dropped pixels included, also strictly inside that range for every ray: a value AT a clip limit is
        a clamped one and never a point (so a hit beyond clip_hi is dropped, not inserted at clip_hi).
        Refused (ElevationMap's docstring): frame="yaw", see_robot without labels, a drop_value inside the clip range with dropout or
        with stereo artefacts (set_stereo() checks the same on a sensor that has its map already)."""
        if m is None:
            return self._drop("map")
        if not isinstance(m, ElevationMap):
            raise TypeError(f"attach_map: expected an ElevationMap or None, got {type(m).__name__}")
        if odometry is not None and not isinstance(odometry, OdometryError):
            raise TypeError(f"attach_map: odometry is an OdometryError or None, got {type(odometry).__name__}")
        if odometry is not None:
            lib.entry(self._api, "lsim_odometry_step", "the odometry")
        if self.model is None:
            raise ValueError("attach_map needs a model (SensorModel): the tick, the period and the episode lengths that say who captured are the model's")
        entry = "lsim_elevation_map" if m.fusion is None else "lsim_elevation_map_fused"
        lib.entry(self._api, entry, "the elevation map")
        if m.cleanup is not None:
            lib.entry(self._api, "lsim_elevation_map_cleanup", "the map's clean-up")
        if self.frame != "base":
            raise ValueError(f"attach_map: the sensor's frame is {self.frame!r}; lsim_elevation_map places the points with the base's full orientation, "
                             "so only a frame='base' sensor can feed a map")
        if self.see_robot and self.label_rows is None:
            raise ValueError("attach_map: a see_robot sensor needs labels=True, or the robot's own legs are inserted as ground")
        env, N, G = self.env, int(self.env.num_envs), m.size
        if m.points is None:
            t = env.cfg.terrain
            pts = [[float(x), float(y)] for x in t.measured_points_x for y in t.measured_points_y]
        else:
            pts = m.points
        if not 1 <= len(pts) <= abi.DEFINES["LSIM_ELEVATION_MAP_MAX_POINTS"]:
            raise ValueError(f"attach_map: 1 to {abi.DEFINES['LSIM_ELEVATION_MAP_MAX_POINTS']} scan points, got {len(pts)}")
        P = len(pts)
        mp = {"pts": torch.tensor(pts, dtype=torch.float32, device=self.out_rows.device).reshape(P, 2).contiguous(),
              "height": self._zeros(N, G, G), "stamp": self._zeros(N, G, G, dtype=torch.int32).fill_(-1), "cell": self._zeros(N, G, G, dtype=torch.int32),
              "scan": self._zeros(N, P), "known": self._zeros(N, P, dtype=torch.uint8), "state": self._zeros(1, dtype=torch.int64)}
        ef = None if m.fusion is None else abi.LsimElevationMapFused()
        em = abi.LsimElevationMap() if ef is None else ef.em           # a view: the fused launch's struct opens with the plain one's
        if ef is not None:
            mp["var"], mp["scan_var"] = self._zeros(N, G, G), self._zeros(N, P)
            ef.var, ef.scan_var, ef.var_stride = mp["var"].data_ptr(), mp["scan_var"].data_ptr(), P
            height = float(self.mount_nominal[0, 2]) + float(env.cfg.rewards.base_height_target)
            (ef.sigma0, ef.sigma2, ef.range_z2, ef.band, ef.var_floor, ef.var_growth, ef.var_max, ef.gate2,
             ef.count_cap) = m.fusion.resolve(self.model.noise, height)
            mp["scan_var"].fill_(float(ef.var_max))
        em.root_states, em.assumed_mount, em.dirs = env.root_states.data_ptr(), self.mount_nominal.data_ptr(), self.dirs.data_ptr()
        widest = narrowest = 1.0
        if self.scale is not None:
            inv = mp["inv_scale"] = (1.0 / self.scale).contiguous()
            em.inv_scale, widest, narrowest = inv.data_ptr(), float(inv.max()), float(inv.min())
        sm, stride = self._stages["capture"].struct, self.out_rows.shape[1]
        if m.source == "clean":
            em.depth, em.depth_stride, em.a, em.b = self.out_rows.data_ptr(), stride, 1.0, 0.0
        else:
            K = self.model.latency + self.model.frames
            em.depth, em.depth_stride = self.history().data_ptr() + (K - 1) * stride * 4, K * stride
            em.a, em.b = 1.0 / float(sm.gain), float(sm.offset)
        if self.label_rows is not None:
            em.labels, em.label_stride = self.label_rows.data_ptr(), self.label_rows.shape[1]
        em.pts = mp["pts"].data_ptr()
        em.height, em.stamp, em.cell = mp["height"].data_ptr(), mp["stamp"].data_ptr(), mp["cell"].data_ptr()
        em.scan, em.known, em.state = mp["scan"].data_ptr(), mp["known"].data_ptr(), mp["state"].data_ptr()
        em.num_rays, em.num_points, em.scan_stride, em.known_stride, em.size = self.num_rays, P, P, P, G
        em.period, em.stagger = sm.period, sm.stagger
        em.res = m.resolution
        # the window of ranges t = d * inv_scale[r] that are points.  d_lo, d_hi bound the stored value d; a ray's t then lies strictly
        # inside for EVERY ray when t_lo = d_lo * max(inv_scale) and t_hi = d_hi * min(inv_scale)
        d_lo, d_hi = self.near, float("inf")
        if m.source == "noisy":
            # the model clamps every value -- misses, hits beyond the range and dropped pixels alike -- to [clip_lo, clip_hi], and "noisy"
            # reads it back through (1 / gain, offset) with a rounding of 2-3 ulp of offset and far: 2^-20 of that magnitude lies well
            # above it.  A value within that margin of a clip limit is a clamped one, never a point
            clip_lo, clip_hi = float(sm.clip_lo), float(sm.clip_hi)
            self._holes_tellable("attach_map", m.source, self.stereo)
            margin = 2.0 ** -20 * max(self.far, abs(float(sm.offset)), abs(clip_hi))
            d_lo, d_hi = max(self.near, clip_lo) + margin, clip_hi - margin
        em.t_lo = d_lo * widest
        em.t_hi = min(0.98 * self.far if m.max_range is None else m.max_range, d_hi * narrowest)
        em.unknown_drop = float(env.cfg.rewards.base_height_target) if m.unknown_drop is None else m.unknown_drop
        if not em.t_lo < em.t_hi:
            raise ValueError(f"attach_map: no range is left between the nearest the sensor reports ({em.t_lo}) and max_range / the clip limit ({em.t_hi})")
        self._drop("map")                   # a new map: the odometry and the rows of the old one go with it
        launches = []
        if odometry is not None:
            od = abi.LsimOdometry()
            held = {"est": env.root_states.detach().clone().contiguous(), "odo": self._zeros(N, 12)}
            od.root_states, od.est, od.odo = env.root_states.data_ptr(), held["est"].data_ptr(), held["odo"].data_ptr()
            od.scale_range, od.yaw_range, od.z_range, od.pos_noise, od.yaw_noise, od.z_noise = odometry.ranges()
            em.root_states = od.est
            launches.append(self._attach(Stage(self, "odometry", "lsim_odometry_step", od, held, odometry)))
        stage = self._attach(Stage(self, "map", entry, em, mp, m, outer=ef))
        if m.cleanup is not None:           # ahead of the map's launch: the same struct, and the fused map's variance when there is one
            ec = abi.LsimElevationMapCleanup()
            ctypes.memmove(ctypes.addressof(ec.em), ctypes.addressof(em), ctypes.sizeof(em))
            held = {"cleared": self._zeros(N, dtype=torch.int32)}
            ec.cleared, ec.var = held["cleared"].data_ptr(), mp["var"].data_ptr() if "var" in mp else None
            ec.clear_margin, ec.clear_slope, ec.clear_sigma, ec.end_gap, ec.min_rays = m.cleanup.resolve(m.resolution)
            launches.append(self._attach(Stage(self, "map_cleanup", "lsim_elevation_map_cleanup", ec.em, held, m.cleanup, outer=ec)))
        launches.append(stage)
        if self.tick >= 0:
            for s in launches:
                s.launch(self.tick, _FILL_ALL)
        return m

    def map_pose(self):
        """live [N, 13] tensor: the pose the map is given -- odometry_pose() with odometry, else the env's root_states"""
        self._need("map")
        return self._stages["odometry"].buffers["est"] if "odometry" in self._stages else self.env.root_states

    def odometry_pose(self):
        """live [N, 13] tensor: the estimated root states (attach_map(m, odometry=...)); columns 7.. are root_states' own"""
        return self._need("odometry").buffers["est"]

    def odometry_state(self):
        """live [N, 12] tensor: row e = {dx, dy, dz, h, scale, yaw_bias, z_bias, 0, prev_x, prev_y, 0, 0} of env e (lsim.h)"""
        return self._need("odometry").buffers["odo"]

    def attach_map_rows(self, channels=("height",), var_ref=None, foot_scan=None):
        """from now on the map's launch of every update() / refresh() is followed by lsim_map_rows on the same stream: `map_rows()` is the
        live [N, len(channels) * P] tensor of the map's scan as an actor reads it -- ("height",): clip(map_pose z - 0.5 - scan, -1, 1) *
        obs_scales.height_measurements, the privileged height scan's expression; ("height", "known"): then map_known() as 0 / 1.  Needs
        an attached map; builds the rows once now when the sensor has captured before.  None: detach and free.
        ("height", "confidence") (lsim_map_rows_fused; needs a map with a fusion): then var_ref / (var_ref + map_variance()) where the
        map knows the point and 0 where it does not -- 1/2 at a variance of `var_ref` (None: 16 times the fusion's var_floor).
        ("foot_height",) and ("foot_height", "foot_known") with `foot_scan` (a FootScan; None: its defaults): the stage "foot_rows",
        lsim_foot_scan directly behind the map's launch -- the map read at FootScan's pattern around each foot, the feet placed by forward
        kinematics from map_pose() and the joint positions; map_rows() then is the live [N, channels * 4K] tensor of
        clip(foot z - z_offset - height, -1, 1) * obs_scales.height_measurements, foot-major, then the known block; foot_heights() and
        foot_known() are [N, 4, K].  Foot rows and scan rows are not both attached: attaching one detaches the other.  A confidence at
        foot points is not built."""
        if channels is None:
            self._drop("foot_rows")
            return self._drop("map_rows")
        channels = tuple(channels)
        if channels in FOOT_CHANNELS:
            return self._attach_foot_rows(channels, FootScan() if foot_scan is None else foot_scan, var_ref)
        if foot_scan is not None:
            raise ValueError(f"attach_map_rows: foot_scan belongs to the channels ('foot_height',) and ('foot_height', 'foot_known'), got {channels}")
        if channels not in (("height",), ("height", "known"), ("height", "confidence")):
            raise ValueError(f"attach_map_rows: channels is ('height',), ('height', 'known'), ('height', 'confidence'), ('foot_height',) or "
                             f"('foot_height', 'foot_known'), got {channels}")
        em, mp = self._need("map").struct, self._need("map").buffers
        fused = channels[-1] == "confidence"
        if fused and self.map.fusion is None:
            raise ValueError("attach_map_rows: the channel 'confidence' needs a map with a fusion (ElevationMap(fusion=MapFusion(...)))")
        if var_ref is not None and not fused:
            raise ValueError("attach_map_rows: var_ref belongs to the channel 'confidence'")
        entry = "lsim_map_rows_fused" if fused else "lsim_map_rows"
        lib.entry(self._api, entry, "the map rows")
        P, C = int(em.num_points), len(channels)
        rows = self._zeros(int(self.env.num_envs), C * P)
        mf = abi.LsimMapRowsFused() if fused else None
        mr = abi.LsimMapRows() if mf is None else mf.mr
        if fused:
            mf.scan_var, mf.var_stride = mp["scan_var"].data_ptr(), P
            mf.var_ref = 16.0 * self.map.fusion.var_floor if var_ref is None else float(var_ref)
            if not (math.isfinite(mf.var_ref) and mf.var_ref > 0.0):
                raise ValueError(f"attach_map_rows: var_ref is finite and > 0, got {mf.var_ref} (a fusion with var_floor 0 needs one given)")
        mr.scan, mr.known, mr.pose, mr.rows = mp["scan"].data_ptr(), mp["known"].data_ptr(), self.map_pose().data_ptr(), rows.data_ptr()
        mr.num_points, mr.channels, mr.scan_stride, mr.known_stride, mr.ld = P, C, int(em.scan_stride), int(em.known_stride), C * P
        mr.z_offset, mr.scale = 0.5, float(self.env.lcfg.obs_scale_height)
        self._drop("foot_rows")             # foot rows and scan rows are not both attached
        stage = self._attach(Stage(self, "map_rows", entry, mr, {"rows": rows}, channels, outer=mf))
        if self.tick >= 0:
            stage.launch(self.tick, _FILL_ALL)
        return rows

    def _attach_foot_rows(self, channels, foot_scan, var_ref):
        """the stage "foot_rows": lsim_foot_scan with the map as its source, directly behind the map's launch, on the map's arrays and the
        pose the map is given; the scan rows, if attached, leave"""
        if var_ref is not None:
            raise ValueError("attach_map_rows: var_ref belongs to the channel 'confidence'; a confidence at foot points is not built")
        em, mp = self._need("map").struct, self._need("map").buffers
        held = {}
        fs = _foot_scan_struct(self.env, self._api, foot_scan, channels, self.map_pose(), self.out_rows.device, held)
        fs.source = abi.DEFINES["LSIM_FOOT_SCAN_MAP"]
        fs.height, fs.stamp, fs.cell = mp["height"].data_ptr(), mp["stamp"].data_ptr(), mp["cell"].data_ptr()
        fs.size, fs.res, fs.unknown_drop = int(em.size), float(em.res), float(em.unknown_drop)
        self._drop("map_rows")              # foot rows and scan rows are not both attached
        stage = self._attach(Stage(self, "foot_rows", "lsim_foot_scan", fs, held, foot_scan))
        stage.channels = channels
        if self.tick >= 0:
            stage.launch(self.tick, _FILL_ALL)
        return held["rows"]

    def map_rows(self):
        """live [N, channels * P] tensor: the rows lsim_map_rows writes (attach_map_rows) -- or, with foot channels, the [N, channels * 4K]
        rows lsim_foot_scan writes"""
        if "foot_rows" in self._stages:
            return self._stages["foot_rows"].buffers["rows"]
        return self._need("map_rows").buffers["rows"]

    def foot_heights(self):
        """live [N, 4, K] tensor: the map's height at every foot point; where it knows none, the given base height minus unknown_drop"""
        return self._need("foot_rows").buffers["heights"].unflatten(1, (4, self.foot_scan.num_points))

    def foot_known(self):
        """live uint8 [N, 4, K] tensor: 1 where foot_heights() is a height the map holds"""
        return self._need("foot_rows").buffers["known"].unflatten(1, (4, self.foot_scan.num_points))

    @property
    def foot_nonfinite(self):
        """0-d device tensor: visits of envs whose given pose or joints were not finite (their foot rows are zeros); must stay 0"""
        return self._need("foot_rows").buffers["state"][0]

    def map_scan(self):
        """live [N, P] tensor: the map's height at every scan point; where it knows none, the base height minus unknown_drop"""
        return self._need("map").buffers["scan"]

    def map_known(self):
        """live uint8 [N, P] tensor: 1 where map_scan() is a height the map holds"""
        return self._need("map").buffers["known"]

    def map_cleared(self):
        """live int32 [N] tensor: the cells the clean-up has forgotten since each env's episode began (ElevationMap(cleanup=...))"""
        return self._need("map_cleanup").buffers["cleared"]

    def map_state(self):
        """the live raw arrays (height f32, stamp i32, cell: the u32 words held in an int32 tensor, and with a fusion var f32), each
        [N, G, G], toroidal (lsim.h)"""
        mp = self._need("map").buffers
        return (mp["height"], mp["stamp"], mp["cell"]) + ((mp["var"],) if "var" in mp else ())

    def map_variance(self):
        """live [N, P] tensor: the variance (m^2) of map_scan() at every scan point, aged to the last launch's tick; var_max where the map
        knows nothing (an ElevationMap with a fusion only)"""
        mp = self._need("map").buffers
        if "scan_var" not in mp:
            raise ValueError("the sensor's elevation map has no fusion (ElevationMap(fusion=MapFusion(...)))")
        return mp["scan_var"]

    @property
    def map_nonfinite(self):
        """0-d device tensor: visits of envs whose pose was not finite (they insert nothing and scan zeros); must stay 0"""
        return self._need("map").buffers["state"][0]

    def map_heights(self):
        """[N, G, G] COPY in window order -- [e, i, j] is the cell (cx - G/2 + i, cy - G/2 + j) around env e's present position (the one the
        map was given: the estimate with odometry) -- with NaN
        where the map knows nothing.  For people and tools (tools/sensor_frames.py); nothing on a hot path reads it."""
        mp, G, N = self._need("map").buffers, self.map.size, int(self.env.num_envs)
        rinv = float(np.float32(1.0 / float(np.float32(self.map.resolution))))
        c = torch.floor(self.map_pose()[:, :2] * rinv).to(torch.int64).clamp(-40000, 40000)          # the window of the pose the map was given
        off = torch.arange(G, device=c.device) - G // 2
        ix, iy = c[:, 0:1] + off, c[:, 1:2] + off
        idx = ((ix & (G - 1)) * G)[:, :, None] + (iy & (G - 1))[:, None, :]
        take = lambda t: t.reshape(N, G * G).gather(1, idx.reshape(N, G * G)).reshape(N, G, G)
        word = ((ix + 32768) << 16)[:, :, None] | (iy + 32768)[:, None, :]
        inside = ((ix.abs() < 32768)[:, :, None] & (iy.abs() < 32768)[:, None, :])
        known = (take(mp["stamp"]) >= 0) & ((take(mp["cell"]).to(torch.int64) & 0xFFFFFFFF) == word) & inside
        return torch.where(known, take(mp["height"]), torch.full((), float("nan"), device=c.device))

    def attach_frames_log(self, steps, capacity=None, row_of=None):
        """the stage "frames_log", directly behind the capture: while a rollout of `steps` storage rows drives it, every update() is
        followed by lsim_sensor_frames_log on the same stream with the same tick and flags, which copies the image (slots 0 .. frames - 1
        of the history) of every env just captured into the next rows of the log and records in row `step` of frame_rows() which row of
        the log each env's latent of that storage row came from.  `capacity`: rows of the log; default N * (1 + ceil((steps - 1) /
        period) + 2) -- the start of the rollout, every tick-due capture, and room for two resets per env per rollout; an image that
        finds no room gets row -1 and counts in frames_log_state()[1].  `row_of`: a contiguous int32 [steps, N] tensor on the sensor's
        device to use as frame_rows() (a rollout storage's own field); default: one of the stage's.  The stage owns its buffers and
        goes with the encoder.  It needs env_stride == 1 and an attached encoder, else ValueError.  None: detach and free.
        Driving it: begin_rollout() logs every env's present image as storage row 0; set_frames_log_step(s) names the row the NEXT
        capture belongs to (the chain run behind env step s - 1 produces the latent of row s), None or s >= steps: idle."""
        if steps is None:
            return self._drop("frames_log")
        if self.model is None or self.encoder is None:
            raise ValueError("attach_frames_log: the sensor has no encoder (attach_encoder first): the log keeps the images the encoder reads")
        if self.env_stride != 1:
            raise ValueError(f"attach_frames_log: env_stride is {self.env_stride}; the log's rows are those of a rollout storage, which holds every env")
        lib.entry(self._api, "lsim_sensor_frames_log", "the frame log")
        steps, N, hist = int(steps), int(self.env.num_envs), self.history()
        if steps < 1:
            raise ValueError(f"attach_frames_log: steps >= 1, got {steps}")
        capacity = N * (1 + -(-(steps - 1) // self.model.period) + 2) if capacity is None else int(capacity)
        if capacity < 1:
            raise ValueError(f"attach_frames_log: capacity >= 1, got {capacity}")
        if row_of is None:
            row_of = self._zeros(steps, N, dtype=torch.int32).fill_(-1)
        elif not (row_of.dtype == torch.int32 and tuple(row_of.shape) == (steps, N) and row_of.is_contiguous() and row_of.device == hist.device):
            raise ValueError(f"attach_frames_log: row_of must be a contiguous int32 [{steps}, {N}] tensor on {hist.device}")
        F, stride = self.model.frames, hist.shape[2]
        held = {"log": self._zeros(capacity, F, stride), "row_of": row_of, "row_src": self._zeros(capacity, dtype=torch.int32).fill_(-1),
                "state": self._zeros(abi.DEFINES["LSIM_FRAMES_LOG_STATE_WORDS"], dtype=torch.int32)}
        fl = abi.LsimFramesLog()
        fl.hist, fl.hist_stride, fl.hist_slots = hist.data_ptr(), stride, hist.shape[1]
        fl.log, fl.row_of, fl.row_src, fl.state = (held[k].data_ptr() for k in ("log", "row_of", "row_src", "state"))
        fl.frames, fl.pixels, fl.row_stride, fl.num_steps, fl.capacity = F, self.num_rays, stride, steps, capacity
        fl.period, fl.stagger = self.model.period, int(self.model.stagger)

        def run(tick, flags, stream):
            if stage.step is None:                      # no rollout drives the log: an evaluation rollout, env.reset(), refresh()
                return
            if flags & _FILL_ALL and stage.step != 0:
                raise RuntimeError("the frame log is in the middle of a rollout (storage row %d): refresh() would start its rows again" % stage.step)
            fl.tick, fl.flags, fl.step = tick, flags, stage.step
            lib.check(self._api.lsim_sensor_frames_log(ctypes.byref(fl), self._stream(stream)), what="lsim_sensor_frames_log")
        stage = self._attach(Stage(self, "frames_log", "lsim_sensor_frames_log", fl, held, (steps, capacity), run=run))
        stage.step = None
        return stage

    def begin_rollout(self, stream=None):
        """the start of a rollout: ONE launch of the frame log with LSIM_SENSOR_FILL_ALL and storage row 0 -- the log starts again and
        every env's present image, the one its latent row was encoded from, becomes a row.  The stage then waits for row 1"""
        stage = self._need("frames_log")
        stage.step = 0
        try:
            stage.launch(max(self.tick, 0), _FILL_ALL, stream)
        finally:
            stage.step = None
        self.set_frames_log_step(1)

    def set_frames_log_step(self, step):
        """the storage row the next capture's images belong to; None, or a row the rollout does not have: the stage is idle"""
        stage = self._need("frames_log")
        stage.step = None if step is None or not 0 < int(step) < stage.option[0] else int(step)

    def frames_log(self):
        """live [capacity, frames, stride] tensor: the logged images, rows 0 .. frames_log_state()[0] - 1 in use; lsim_depth_encode reads
        it in place as a batch (hist_slots = frames)"""
        return self._need("frames_log").buffers["log"]

    def frame_rows(self):
        """live int32 [steps, N] tensor: the row of frames_log() that holds the image env e's latent of storage row t came from, or -1"""
        return self._need("frames_log").buffers["row_of"]

    def frames_log_sources(self):
        """live int32 [capacity] tensor: t * N + e of the storage row and env that wrote each row of the log"""
        return self._need("frames_log").buffers["row_src"]

    def frames_log_state(self):
        """live int32 tensor: [0] the rows in use, [1] the images that found no room (never reset by the launch), then the launch's own words"""
        return self._need("frames_log").buffers["state"]

    def attach_memory(self, mem):
        """from now on the encoder's launch of every update() / refresh() is followed by `mem`'s (learn.depth_memory.DepthMemory.step_device)
        on the same stream with the same flags; steps every env once now from h = 0 (LSIM_SENSOR_FILL_ALL).  Needs an attached encoder.
        The hidden state h [N, H] and the rows [N, L + H] are this sensor's, like its latent: one `mem` may serve several sensors.
        None: detach and free."""
        if mem is None:
            return self._drop("memory")
        if self.encoder is None:
            raise ValueError("attach_memory: the sensor has no encoder (attach_encoder first): the memory reads its latent rows")
        self.latent_buffer(self.encoder.latent_dim)
        N, widths = int(self.env.num_envs), (mem.hidden, mem.latent_dim + mem.hidden)
        buffers = self._kept("memory", dict)
        if [t.shape[1] for t in buffers.values()] != list(widths):
            buffers = {"h": self._zeros(N, widths[0]), "rows": self._zeros(N, widths[1])}
        stage = self._attach(Stage(self, "memory", "lsim_depth_memory_step", None, buffers, mem, run=lambda tick, flags, stream: mem.step_device(self, flags, stream)))
        stage.launch(self.tick, _FILL_ALL)
        return mem

    def memory_rows(self):
        """live [N, L + H] tensor: row e = [latent of env e | its memory's hidden state] (attach_memory)"""
        return self._need("memory").buffers["rows"]

    def memory_state(self):
        """live [N, H] tensor: the hidden state of every env's memory (attach_memory)"""
        return self._need("memory").buffers["h"]

    def _latent_held(self):
        """where the latent lives: the encoder stage's buffers, or the sensor's spare ones for an encoder launched by hand"""
        return self._stages["encoder"].buffers if "encoder" in self._stages else self._spare

    def latent_buffer(self, latent_dim):
        """the [N, stride] buffer an encoder's launch writes; created on first use"""
        held, stride = self._latent_held(), (int(latent_dim) + 3) // 4 * 4
        if "latent" not in held or held["latent"].shape[1] != stride:
            held["latent"] = self._zeros(int(self.env.num_envs), stride)
        self._latent_dim = int(latent_dim)
        return held["latent"]

    def latent(self):
        """live [N, latent_dim] tensor: row e is the encoding of env e's frames at its last capture (attach_encoder)"""
        if "latent" not in self._latent_held():
            raise ValueError(f"the sensor has no {_ABSENT['encoder']}")
        return self._latent_held()["latent"][:, :self._latent_dim]

    def labels(self):
        """live uint8 [N, R] tensor of the latest launch (labels=True): 0 nothing within [near, far], 1 terrain, 2 + b body b (`body_names[b]`)"""
        if self.label_rows is None:
            raise ValueError("the sensor was created without labels=True")
        return self.label_rows[:, :self.num_rays]

    def spec(self):
        """What rebuilds this sensor on another env (from_spec), as a dict of plain Python values and lists -- a checkpoint's record of the
        instrument a policy was trained with: kind ("camera" with width / height, "lidar" with channels / points_per_rev, else "rays"),
        dirs, scale, near, far, env_stride, see_robot, the names of the ignored bodies, labels, frame, the SensorModel's fields (None
        without one) and the mount: {"pos", "quat"} when all envs share it, {robot name: pose} when it is constant per robot, else None.
        With a mount jitter the mount recorded is the nominal one and "mount_jitter" holds the MountJitter's {"pos", "rot_deg"}; without
        one there is no such key.  Likewise "instrument" holds an InstrumentError's record, "map" an attached ElevationMap's,
        "odometry" the OdometryError the map was attached with, "stereo" a StereoArtifacts', "shading" a Shading's and "foot_scan" the FootScan of attached foot
        rows, each absent without one."""
        out = dict(self.kind)
        out["dirs"] = self.dirs.cpu().tolist()
        out["scale"] = None if self.scale is None else self.scale.cpu().tolist()
        out.update(near=self.near, far=self.far, env_stride=self.env_stride, see_robot=self.see_robot, labels=self.label_rows is not None, frame=self.frame)
        mask = self.body_mask if self.see_robot else None
        out["ignore_bodies"] = [] if mask is None else [n for i, n in enumerate(self.body_names) if not mask >> i & 1]
        out["model"] = None if self.model is None else self.model.record()
        mount = self.mount_nominal.cpu()
        pose = lambda row: {"pos": row[:3].tolist(), "quat": row[3:].tolist()}
        names, ids = getattr(self.env, "robot_names", None), getattr(self.env, "robot_ids", None)
        rows = [] if names is None or ids is None else [mount[ids.cpu() == k] for k in range(len(names))]
        if bool((mount == mount[:1]).all()):
            out["mount"] = pose(mount[0])
        elif rows and all(bool((r == r[:1]).all()) for r in rows):
            out["mount"] = {n: pose(r[0]) for n, r in zip(names, rows) if len(r)}
        else:
            out["mount"] = None
        for key, option in (("mount_jitter", self.mount_jitter), ("instrument", self.instrument), ("map", self.map), ("odometry", self.odometry), ("stereo", self.stereo),
                            ("shading", self.shading), ("foot_scan", self.foot_scan)):
            if option is not None:
                out[key] = option.record()
        return out

    @property
    def nonfinite_rays(self):
        """0-d device tensor: rays so far whose origin or direction was not finite (they report `far`); must stay 0"""
        return self.state[0]


class DepthCamera(RaySensor):
    """`rays` = (dirs, scale) and `mount_quat`: a recorded camera's own (from_spec), in place of the pinhole's of `hfov_deg` and `pitch_deg`"""

    def __init__(self, env, width, height, hfov_deg, mount_pos=(0.0, 0.0, 0.0), pitch_deg=0.0, near=0.05, far=5.0, env_stride=1, api=None,
                 rays=None, mount_quat=None, **options):
        dirs, scale = pinhole_dirs(width, height, hfov_deg) if rays is None else rays
        self.hfov_deg = None if rays is not None else float(hfov_deg)
        super().__init__(env, dirs, mount_pos, quat_from_pitch(pitch_deg) if mount_quat is None else mount_quat, near, far, scale=scale,
                         env_stride=env_stride, api=api, kind={"kind": "camera", "width": width, "height": height}, **options)

    def image(self):
        """[N, H, W] view of the output: z-depth along the optical axis in metres, far * cos where nothing is hit"""
        return self.out.unflatten(1, (self.height, self.width))

    def label_image(self):
        """[N, H, W] view of labels()"""
        return self.labels().unflatten(1, (self.height, self.width))

    def frame_images(self):
        """[N, frames, H, W] view of frames()"""
        return self.frames().unflatten(2, (self.height, self.width))

    def rgba_image(self):
        """live uint8 [N, H, W, 4] view of the shaded frame: red, green, blue, 255 (shading=...)"""
        return self.rgba().unflatten(1, (self.height, self.width))

    def rgb_image(self):
        """[N, H, W, 3] view of rgba_image(): what a PPM holds"""
        return self.rgba_image()[..., :3]


def depth_camera(env, width, height, hfov_deg, mount_pos=(0.0, 0.0, 0.0), pitch_deg=0.0, near=0.05, far=5.0, env_stride=1, api=None, **options):
    """a pinhole depth camera looking along the base x axis pitched down by `pitch_deg`; `mount_pos` and `options` (see_robot, ignore_bodies,
    labels, frame, model, mount_jitter, instrument, stereo, shading) as RaySensor's"""
    return DepthCamera(env, width, height, hfov_deg, mount_pos, pitch_deg, near, far, env_stride, api, **options)


def chase_camera(env, width=128, height=96, hfov_deg=60.0, mount_pos=(-1.2, 0.0, 0.7), pitch_deg=28.0, near=0.05, far=8.0, env_stride=1, api=None,
                 shading="default", **options):
    """the viewer's camera: behind and above the robot, following its position and yaw only (frame="yaw"), seeing the robot, labelled and
    shaded (`shading`: a Shading, None for depth and labels only; by default Shading()).  `rgb_image()` is the frame; width * height stays
    within LSIM_RAYCAST_MAX_RAYS.  `far` 8 m is a stated guess: the horizon of a 28 degree pitch over flat ground lies beyond any far."""
    if width * height > abi.DEFINES["LSIM_RAYCAST_MAX_RAYS"]:
        raise ValueError(f"chase_camera: {width} x {height} exceeds LSIM_RAYCAST_MAX_RAYS = {abi.DEFINES['LSIM_RAYCAST_MAX_RAYS']} pixels")
    shading = Shading() if isinstance(shading, str) and shading == "default" else shading
    return DepthCamera(env, width, height, hfov_deg, mount_pos, pitch_deg, near, far, env_stride, api, see_robot=True, labels=True, frame="yaw",
                       shading=shading, **options)


def lidar(env, channels, vfov_deg, points_per_rev, mount_pos=(0.0, 0.0, 0.0), mount_quat=(0.0, 0.0, 0.0, 1.0), near=0.05, far=10.0, env_stride=1, api=None,
          **options):
    """a spinning lidar: `channels` rings over the vertical field of view `vfov_deg` (a width centred on the horizon, or (low, high) degrees),
    `points_per_rev` azimuths each; reports range (scale=None); `options` (see_robot, ignore_bodies, labels, frame, model, mount_jitter,
    instrument) as RaySensor's"""
    return RaySensor(env, ring_dirs(channels, vfov_deg, points_per_rev), mount_pos, mount_quat, near, far, scale=None, env_stride=env_stride, api=api,
                     kind={"kind": "lidar", "channels": channels, "points_per_rev": points_per_rev}, **options)


_KIND_KEYS = {"rays": (), "camera": ("width", "height"), "lidar": ("channels", "points_per_rev")}


def from_spec(env, spec, mount_pos=None, mount_quat=None, api=None, mount_jitter="spec", instrument="spec", elevation_map="spec", odometry="spec", stereo="spec",
              shading="spec", foot_scan="spec"):
    """the sensor RaySensor.spec() describes, on `env`: same rays, range, model constants and body mask.  `mount_pos` / `mount_quat` (as
    RaySensor's) override the recorded mount; a recorded mount of None (it varied per env) without the override raises, and so does a
    per-robot mount that lacks one of the env's robots (RaySensor's own check).  `mount_jitter`: "spec" rebuilds the recorded MountJitter
    (none when the record has none); None or a MountJitter takes its place.  `instrument`: the same for the recorded InstrumentError, `elevation_map` for the recorded ElevationMap (attached to the new sensor),
    `odometry` for the OdometryError that map is attached with (without a map it has nothing to act on), `stereo` for the recorded
    StereoArtifacts, `shading` for the recorded Shading, `foot_scan` for the recorded FootScan: with one (and a map) the new sensor gets the
    one-channel foot rows, attach_map_rows(("foot_height",), foot_scan=...) -- the record holds the pattern, not the channels, which are a
    policy's; whoever wants the known block attaches again."""
    mount = spec.get("mount")
    if mount is not None and "pos" not in mount:
        pos, quat = {n: p["pos"] for n, p in mount.items()}, {n: p["quat"] for n, p in mount.items()}
    elif mount is not None:
        pos, quat = mount["pos"], mount["quat"]
    else:
        pos = quat = None
    pos = mount_pos if mount_pos is not None else pos
    quat = mount_quat if mount_quat is not None else quat
    if pos is None or quat is None:
        raise ValueError("from_spec: the recorded sensor's mount differed from env to env (spec['mount'] is None): pass mount_pos and mount_quat")
    def option(name, value, cls, key):
        """`value` of from_spec's keyword `name`: "spec" -- the record under `key` rebuilt (none: None); None or a `cls` -- that"""
        if isinstance(value, str) and value == "spec":
            return None if spec.get(key) is None else cls(**spec[key])
        if value is None or isinstance(value, cls):
            return value
        raise ValueError(f"from_spec: {name} is 'spec', None or of class {cls.__name__}, got {value!r}")

    model = option("model", "spec", SensorModel, "model")
    mount_jitter, instrument = option("mount_jitter", mount_jitter, MountJitter, "mount_jitter"), option("instrument", instrument, InstrumentError, "instrument")
    elevation_map, odometry = option("elevation_map", elevation_map, ElevationMap, "map"), option("odometry", odometry, OdometryError, "odometry")
    stereo, shading = option("stereo", stereo, StereoArtifacts, "stereo"), option("shading", shading, Shading, "shading")
    foot_scan = option("foot_scan", foot_scan, FootScan, "foot_scan")
    kind = spec.get("kind", "rays") if spec.get("kind") in _KIND_KEYS else "rays"
    dirs, scale = np.asarray(spec["dirs"], dtype=np.float32), None if spec["scale"] is None else np.asarray(spec["scale"], dtype=np.float32)
    options = dict(env_stride=spec["env_stride"], api=api, see_robot=spec["see_robot"], ignore_bodies=tuple(spec["ignore_bodies"]), labels=spec["labels"],
                   frame=spec["frame"], model=model, mount_jitter=mount_jitter, instrument=instrument, stereo=stereo, shading=shading)
    if kind == "camera":                    # DepthCamera's constructor derives the rays from a field of view; the record holds the rays themselves
        sensor = DepthCamera(env, spec["width"], spec["height"], None, pos, near=spec["near"], far=spec["far"], rays=(dirs, scale), mount_quat=quat, **options)
    else:
        sensor = RaySensor(env, dirs, pos, quat, spec["near"], spec["far"], scale=scale, kind={"kind": kind, **{k: spec[k] for k in _KIND_KEYS[kind]}}, **options)
    if elevation_map is not None:
        sensor.attach_map(elevation_map, odometry=odometry)
        if foot_scan is not None:
            sensor.attach_map_rows(FOOT_CHANNELS[0], foot_scan=foot_scan)
    return sensor

