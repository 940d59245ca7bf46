"""TEST INFRASTRUCTURE -- the scenes, suns and the launch rig shared by tests/test_sensor_shade.py (CPU shim) and
tests/test_gpu_sensor_shade.py (HIP launch).  The scenes are those of tests/raycast_bodies_scenes.py: a plane and stairs up and down, four
envs with two robots, the small camera in the trunk and the chase camera of frame="yaw"; on each, three suns with and without shadows.
The reference of a scene (tests/sensor_shade_reference.py: nine float64 evaluations) is computed once per process and shared: the
geometry by (ground, camera), the light by sun and flags on top of it."""
import ctypes
import math

import numpy as np

import emu_binding
import raycast_bodies_emu_binding as BE
import raycast_bodies_reference as RB
import raycast_bodies_scenes as BS
import raycast_scenes as S
import sensor_shade_reference as SR
from helpers import abi
from launch_rig import EditRig

GROUNDS = ("plane", "stairs_up", "stairs_down")
CAMERAS = ("camera", "chase")


def sun_vector(azimuth_deg, elevation_deg):
    az, el = math.radians(azimuth_deg), math.radians(elevation_deg)
    return np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)], np.float32)


# towards the sun.  high: near the zenith; low: 22 degrees up and BEHIND the robots of envs 0 and 1 (yaw 0.2 and -0.4), so trunk and legs throw a
# long shadow forward, into both cameras' view, and a riser that faces away from it shades its tread; side: from the robots' left
SUNS = {"high": sun_vector(40.0, 72.0), "low": sun_vector(185.0, 22.0), "side": sun_vector(95.0, 40.0)}
SHADE = {"ambient": 0.35, "checker": 0.37, "checker_gain": 0.8, "shadow_bias": 2e-3, "shadow_far": 4.0}
PALETTE = np.array([0xEBCE87, 0x6B8E6B] + [0x202020 * (1 + b % 5) + 0x30 * b for b in range(17)], np.uint32)
CASES = [(g, c, s, sh) for g in GROUNDS for c in CAMERAS for s in SUNS for sh in (1, 0)]
ids = lambda c: f"{c[0]}-{c[1]}-{c[2]}-{'shadows' if c[3] else 'plain'}"
_geo, _ref = {}, {}


def shim():
    """the CPU shim of the launch, bound from include/lsim.h (emu_binding.SHIMS is not edited: the shim names its headers here)"""
    return emu_binding.load_shim("sensor_shade", ["ls_raycast.h", "ls_raycast_bodies.h", "ls_sensor_shade.h"])


def inputs(ground, camera, capsule=True):
    """(scene, tables, root_states, dof_pos, mount, dirs, scale, flags) of tests/raycast_bodies_scenes.py"""
    return BS.case_inputs((f"{ground}-{camera}", ground, S.BORDER, camera, capsule))


def shade_dict(sun, shadows, **over):
    return dict(SHADE, sun=SUNS[sun] if isinstance(sun, str) else np.asarray(sun, np.float32), flags=SR.SHADOWS if shadows else 0, **over)


def reference(ground, camera, sun, shadows, body_mask=0x1FFFF, capsule=True):
    """nine() of a scene, computed once"""
    key = (ground, camera, body_mask, capsule)
    sc, tabs, rs, th, mt, dirs, scale, flags = inputs(ground, camera, capsule)
    robots = [RB.robot_dict(t) for t in tabs]
    if key not in _geo:
        _geo[key] = SR.geometries(sc, robots, BS.ENV_ROBOT, rs, th, mt, dirs, BS.NEAR, BS.FAR, body_mask, flags)
    if key + (sun, shadows) not in _ref:
        _ref[key + (sun, shadows)] = SR.nine(sc, robots, BS.ENV_ROBOT, rs, th, mt, dirs, BS.NEAR, BS.FAR, shade_dict(sun, shadows), body_mask, flags, geoms=_geo[key])
    return _ref[key + (sun, shadows)]


class ShadeRig(EditRig):
    """the arrays of an lsim_raycast_bodies and of the lsim_sensor_shade behind it, on the host (the two CPU shims) or on `device` (the HIP
    library); run() launches the pair and returns (rgba [N, R], surface [N, R, 4] or None, out [N, R], labels [N, R], state [4])"""

    def __init__(self, ground, camera, sun, shadows, device=None, env_stride=1, body_mask=0x1FFFF, surface=True, capsule=True, rs=None, th=None, **over):
        super().__init__(device)
        sc, tabs, rs0, th0, mt, dirs, scale, flags = inputs(ground, camera, capsule)
        rs, th = rs0 if rs is None else rs, th0 if th is None else th
        self.inputs = (sc, tabs, rs, th, mt, dirs, scale, flags)
        self.shade = shade_dict(sun, shadows, **over)
        N, R = rs.shape[0], dirs.shape[0]
        self.N, self.R, self.stride = N, R, (R + 3) // 4 * 4 + 4
        rb, a = BE.fill(sc, tabs, BS.ENV_ROBOT, rs, th, mt, dirs, BS.NEAR, BS.FAR, scale=scale, env_stride=env_stride, body_mask=body_mask, flags=flags)
        self._host = a                       # robots_host stays on the host
        for k in ("root_states", "mount", "dirs", "scale", "mesh", "dof_state", "env_robot"):
            if k in a:
                self.add(k, a[k])
        self.add("robots", np.frombuffer(a["robots"], dtype=np.uint8).copy())
        self.add("out", a["out"], guard=True)
        self.add("state", a["state"], guard=np.int64(-7))
        self.add("labels", a["labels"], guard=np.uint8(0xA5))
        self.add("rgba", np.full((N, self.stride), 0xDEADBEEF, np.uint32), guard=np.uint32(0xFEEDFACE))
        if surface:
            self.add("surface", np.full((N, R, 4), np.nan, np.float32), guard=True)
        self.add("palette", PALETTE)
        self.point(rb.rc, ("root_states", "mount", "dirs", "scale", "mesh", "out", "state"))
        self.point(rb, ("dof_state", "env_robot", "robots", "labels"))
        ss = abi.LsimSensorShade()
        ss.rb = rb
        self.point(ss, ("rgba", "surface", "palette"))
        for k in range(3):
            ss.sun[k] = float(self.shade["sun"][k])
        for k in ("ambient", "checker", "checker_gain", "shadow_bias", "shadow_far"):
            setattr(ss, k, self.shade[k])
        ss.rgba_stride, ss.shade_flags = self.stride, self.shade["flags"]
        if device is None:
            self._rays, entry = emu_binding.shim("raycast_bodies").emu_raycast_bodies, shim().emu_sensor_shade
        else:
            from launch_rig import device_lib
            self._rays, entry = device_lib().lsim_raycast_bodies, device_lib().lsim_sensor_shade
        self.bind(ss, entry)

    def rays(self, stream=None):
        rb = abi.LsimRaycastBodies.from_buffer_copy(self.struct.rb)
        return self._rays(ctypes.byref(rb), self.stream(stream))

    def read(self):
        self.assert_guards()
        R = self.R
        surface = self.get("surface") if "surface" in self.a else None
        return self.get("rgba")[:, :R], surface, self.get("out")[:, :R], self.get("labels")[:, :R], self.get("state")

    def run(self, edit=None):
        assert self.rays() == 0
        rv = self.launch(edit=edit)
        assert rv == 0, rv
        return self.read()

    def check(self, got, ref=None, label="", mutant=None, strict=True, body_mask=0x1FFFF):
        sc, tabs, rs, th, mt, dirs, scale, flags = self.inputs
        rgba, surface, out, labels, _ = got
        return SR.check(sc, [RB.robot_dict(t) for t in tabs], BS.ENV_ROBOT, rs, th, mt, dirs, BS.NEAR, BS.FAR, self.shade, PALETTE, rgba, surface, out, labels,
                        scale=scale, body_mask=body_mask, flags=flags, label=label, mutant=mutant, strict=strict, ref=ref)
