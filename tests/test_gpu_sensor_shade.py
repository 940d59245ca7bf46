"""GPU: the shaded-frame launch (lsim_sensor_shade, isaacgymloco_amd/csrc/ls_sensor_shade.h) on a real device against the float64 reference of
tests/sensor_shade_reference.py on the scenes of tests/sensor_shade_scenes.py (the rule and its tolerances: that reference's docstring),
against the CPU build of the same source, in a captured graph, and through envs/sensors.py on a LeggedRobot on stairs.  Every GPU step is
one launch or a few env steps and runs once."""
import numpy as np
import pytest

import raycast_bodies_reference as RB
import raycast_reference as REF
import sensor_shade_reference as SR
import sensor_shade_scenes as SS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("case", SS.CASES, ids=SS.ids)
def test_hip_launch_matches_the_reference_and_the_cpu_build(case):
    rig = SS.ShadeRig(*case, device=DEV)
    got = rig.run()
    assert got[4][0] == 0
    res = rig.check(got, SS.reference(*case), label="hip " + SS.ids(case), strict=False)
    assert res["normal"] <= REF.MAX_UNSTABLE and res["light"] <= REF.MAX_UNSTABLE
    ground, camera, sun, shadows = case
    c = (got[1][..., :3].astype(np.float64) * SS.SUNS[sun].astype(np.float64)).sum(-1)
    dark = int(((got[3] == 1) & (c > 1e-3) & (got[1][..., 3] == 0)).sum())
    if shadows and sun == "low":
        assert dark > 0, "the low sun must throw shadows on terrain that faces it"
    if not shadows:
        assert dark == 0, "without shadows nothing that faces the sun is dark"
    emu = SS.ShadeRig(*case).run()
    n_differ = np.linalg.norm(got[1][..., :3] - emu[1][..., :3], axis=-1) > SR.ANG_TOL
    l_differ = got[1][..., 3] != emu[1][..., 3]
    c_differ = (got[0] != emu[0])
    print(f"hip vs emu {SS.ids(case)}: normals {n_differ.mean():.4%}, lights {l_differ.mean():.4%}, colour words {c_differ.mean():.4%} of {l_differ.size} pixels differ")
    assert n_differ.mean() <= REF.MAX_UNSTABLE and l_differ.mean() <= REF.MAX_UNSTABLE and c_differ.mean() <= 2 * REF.MAX_UNSTABLE


def test_launch_conditions_on_the_device():
    """env_stride 3 with untouched rows and guards, surface == NULL, a zero body mask"""
    want = SS.ShadeRig("stairs_up", "camera", "side", 1, device=DEV).run()
    rig = SS.ShadeRig("stairs_up", "camera", "side", 1, device=DEV, env_stride=3)
    rgba, surface, out, labels, state = rig.run()
    for e in (0, 3):
        np.testing.assert_array_equal(rgba[e], want[0][e])
        np.testing.assert_array_equal(surface[e].view(np.int32), want[1][e].view(np.int32))
    for e in (1, 2):
        assert (rgba[e] == 0xDEADBEEF).all() and np.isnan(surface[e]).all()
    bare = SS.ShadeRig("stairs_up", "camera", "side", 1, device=DEV, surface=False).run()
    np.testing.assert_array_equal(bare[0], want[0])
    rgba, surface, out, labels, _ = SS.ShadeRig("plane", "chase", "low", 1, device=DEV, body_mask=0).run()
    assert set(np.unique(labels).tolist()) <= {0, 1} and (surface[..., 3][labels == 1] == 1).all()


def test_captured_pair_replays_bit_for_bit():
    """rays then shade, captured once on one stream (one linear chain) and replayed once"""
    import torch
    rig = SS.ShadeRig("stairs_up", "chase", "low", 1, device=DEV)
    eager = rig.run()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        assert rig.rays(stream=side) == 0 and rig.launch(stream=side) == 0
    rig.put("rgba", 0)
    rig.put("surface", np.nan)
    rig.put("out", -1.0)
    graph.replay()
    torch.cuda.synchronize()
    replayed = rig.read()
    np.testing.assert_array_equal(replayed[0], eager[0])
    np.testing.assert_array_equal(replayed[1].view(np.int32), eager[1].view(np.int32))


class _Counting:
    """the library with its calls counted by entry point"""

    def __init__(self, L):
        self._L, self.calls = L, {}

    def __getattr__(self, name):
        fn = getattr(self._L, name)

        def call(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return call


def test_chase_camera_on_a_legged_robot_on_stairs():
    """16 envs on stairs, a 64 x 48 chase camera on every 4th env, 5 steps of random actions: rgb_image() and surface() against the reference
    evaluated on a copy of the env's state (every 16th pixel: the brute force takes the whole 120 x 120 mesh nine times), the low sun's
    shadows on the ground, and a twin without the option that launches no shade kernel"""
    import torch
    from isaacgymloco_amd.envs import sensors
    from test_gpu_raycast import stairs_env
    env = stairs_env(16)
    api = _Counting(env._L)
    opt = sensors.Shading(sun=(185.0, 22.0), checker=0.37)        # no multiple of the grid's 0.1 m: no riser lies in a checker boundary
    cam = env.add_sensor("chase", sensors.chase_camera(env, 64, 48, env_stride=4, far=6.0, api=api, shading=opt))
    twin = env.add_sensor("twin", sensors.chase_camera(env, 64, 48, env_stride=4, far=6.0, api=api, shading=None))
    g = torch.Generator().manual_seed(4)
    for _ in range(5):
        env.step_device((torch.randn(16, 12, generator=g) * 0.5).to(DEV))
    torch.cuda.synchronize()
    assert api.calls["lsim_sensor_shade"] == 5 and api.calls["lsim_raycast_bodies"] == 10
    assert twin.chain() == ("lsim_raycast_bodies",) and twin.stage("shade") is None and cam.chain() == ("lsim_raycast_bodies", "lsim_sensor_shade")
    assert int(cam.nonfinite_rays) == 0 and torch.equal(cam.out, twin.out) and torch.equal(cam.labels(), twin.labels())
    rgb = cam.rgb_image()
    assert rgb.shape == (16, 48, 64, 3) and bool((cam.rgba_image()[1::4] == 0).all())
    sub, px = np.arange(0, 16, 4), np.arange(0, 64 * 48, 16)
    rs, th = env.root_states.cpu().numpy()[sub], env.dof_pos.cpu().numpy()[sub]
    sc = {"mesh_type": int(env.lcfg.mesh_type), "words": env.buf["terrain_mesh"].cpu().numpy(), "hs": env.lcfg.horizontal_scale,
          "vs": env.lcfg.vertical_scale, "border": env.lcfg.border_size}
    shade = dict(sun=np.asarray(opt.sun_vector(), np.float32), ambient=opt.ambient, checker=opt.checker, checker_gain=opt.checker_gain,
                 shadow_bias=opt.shadow_bias, shadow_far=opt.shadow_far, flags=SR.SHADOWS)
    words = cam.rgba_image().cpu().numpy().reshape(16, 64 * 48, 4).copy().view(np.uint32)[..., 0]
    surface, out, labels = cam.surface().cpu().numpy(), cam.out.cpu().numpy(), cam.labels().cpu().numpy()
    res = SR.check(sc, [RB.robot_dict(t) for t in cam._robots_host], env.robot_ids.cpu().numpy()[sub], rs, th, cam.mount.cpu().numpy()[sub],
                   cam.dirs.cpu().numpy()[px], cam.near, cam.far, shade, np.asarray(opt.palette_words(), np.uint32), words[sub][:, px], surface[sub][:, px],
                   out[sub][:, px], labels[sub][:, px], scale=cam.scale.cpu().numpy()[px], body_mask=cam.body_mask, flags=RB.FRAME_YAW,
                   label="hip env stairs chase", strict=False)
    assert res["normal"] <= REF.MAX_UNSTABLE and res["light"] <= REF.MAX_UNSTABLE
    c = (surface[sub][..., :3].astype(np.float64) * shade["sun"].astype(np.float64)).sum(-1)
    dark = (labels[sub] == 1) & (c > 1e-3) & (surface[sub][..., 3] == 0)
    print(f"hip env stairs chase: {int(dark.sum())} of {dark.size} pixels are terrain that faces the low sun and lies in a shadow")
    assert dark.sum() > 0, "the robot and the risers throw shadows on ground that faces the low sun"
    cam.set_shading(sensors.Shading(sun=(185.0, 22.0), shadows=False, checker=0.37))
    cam.update()
    torch.cuda.synchronize()
    s2, l2 = cam.surface().cpu().numpy()[sub], cam.labels().cpu().numpy()[sub]
    c2 = (s2[..., :3].astype(np.float64) * shade["sun"].astype(np.float64)).sum(-1)
    assert ((l2 > 0) & (c2 > 1e-3) & (s2[..., 3] == 0)).sum() == 0, "without shadows nothing that faces the sun is dark"
