"""GPU: the full chain of stages behind RaySensor.update() (envs/sensors.py) once on the device -- 8 Aliengo envs on stairs, a 16 x 12 camera
that sees and labels the robot, with mount jitter, instrument error, elevation map, odometry, map rows, encoder and memory -- through the
real library behind a wrapper that logs the entry points: the launches and their order, the tick, flags, seed, rank and stream id every
struct carries, where the one ray struct points, and outputs that are finite.  tests/test_sensor_chain.py runs every combination on the
CPU; what each launch computes is held to its reference in the tests of that launch."""
import pytest
import torch

from helpers import abi
from test_gpu_elevation_map_chain import DEV, FAR, _env

pytestmark = pytest.mark.gpu
N = 8
FILL_ALL, RESETS_ONLY = abi.DEFINES["LSIM_SENSOR_FILL_ALL"], abi.DEFINES["LSIM_SENSOR_RESETS_ONLY"]
CHAIN = ("lsim_odometry_step", "lsim_sensor_mount_jitter", "lsim_sensor_instrument", "lsim_sensor_capture_inst", "lsim_elevation_map", "lsim_map_rows",
         "lsim_depth_encode", "lsim_depth_memory_step")
SHARED = ("tick", "flags", "seed", "rank", "stream_id")


class Logged:
    """the library, with the calls of `names` appended to `log` in order"""

    def __init__(self, library, names):
        self._library, self.log = library, []
        for n in names:
            setattr(self, n, self._logging(n))

    def _logging(self, name):
        def call(*args):
            self.log.append(name)
            return getattr(self._library, name)(*args)
        return call

    def __getattr__(self, name):
        return getattr(self._library, name)


def test_the_full_chain_on_the_device_launches_in_order_with_one_tick_and_finite_outputs():
    from isaacgymloco_amd.envs import sensors
    from isaacgymloco_amd.learn.depth_encoder import DepthEncoder
    from isaacgymloco_amd.learn.depth_memory import DepthMemory
    env = _env(5, num_envs=N)
    api = Logged(env._L, CHAIN + ("lsim_sensor_capture", "lsim_raycast", "lsim_raycast_bodies"))
    jitter = sensors.MountJitter(pos=0.01, rot_deg=(1, 5, 1))
    cam = sensors.depth_camera(env, 16, 12, 87.0, mount_pos=(0.3, 0.0, 0.05), pitch_deg=30.0, near=0.05, far=FAR, api=api, see_robot=True, labels=True,
                               model=sensors.SensorModel(period=3, stagger=True, latency=1, frames=2, noise=(0.01, 0.002), normalise=True),
                               mount_jitter=jitter,
                               instrument=sensors.InstrumentError(latency=(0, 1), noise_gain=(0.5, 2.0), depth_scale=0.02, depth_quad=0.005, fov=0.02))
    cam.attach_map(sensors.ElevationMap(size=32), odometry=sensors.OdometryError(scale=0.02, yaw_per_m=0.02, z_per_m=0.02, noise=(0.005, 0.002, 0.002)))
    cam.attach_map_rows(("height", "known"))
    torch.manual_seed(2)
    cam.attach_encoder(DepthEncoder(12, 16, 2, c1=4, k1=3, s1=2, c2=8, k2=3, s2=1, latent_dim=10).to(DEV))
    cam.attach_memory(DepthMemory(10, env.num_one_step_obs, 32).to(DEV))
    assert cam.chain() == CHAIN and api.log == ["lsim_depth_memory_step"], "attach_memory is the one attach that launches before a capture"
    del api.log[:]

    def launched(tick, flags, times):
        assert tuple(api.log) == CHAIN * times, "the log is the chain, repeated"
        structs = {s.entry: s.struct for s in map(cam.stage, sensors._ORDER) if s is not None and s.struct is not None}
        assert set(structs) == set(CHAIN[:6])
        capture = {f: int(getattr(structs["lsim_sensor_capture_inst"], f)) for f in SHARED}
        assert capture == dict(zip(SHARED, (tick, flags, int(env.lcfg.seed), int(env.lcfg.rank), 0))) and cam.tick == tick and cam.stream_id == 0
        for entry, st in structs.items():
            assert all(int(getattr(st, f)) == capture[f] for f in SHARED if hasattr(st, f)), entry
        assert cam.stage("capture").struct.rb.rc.mount == cam.bodies_struct.rc.mount == cam.ray_struct.mount == cam.mount.data_ptr() != cam.mount_nominal.data_ptr()

    tick = int(env.common_step_counter)
    env.add_sensor("depth", cam)
    launched(tick, FILL_ALL, 1)
    g = torch.Generator().manual_seed(0)
    for step in range(3):
        tick = int(env.common_step_counter)
        env.step_device((torch.randn(N, 12, generator=g) * 0.3).to(DEV))
        launched(tick, 0, 2 + step)
    env.reset_idx([1])
    launched(int(env.common_step_counter), RESETS_ONLY, 5)
    torch.cuda.synchronize()
    outputs = {"out": cam.out, "history": cam.history(), "mount": cam.mount, "instrument": cam.instrument_rows(), "map height": cam.map_state()[0],
               "map scan": cam.map_scan(), "odometry pose": cam.odometry_pose(), "odometry state": cam.odometry_state(), "map rows": cam.map_rows(),
               "latent": cam.latent(), "memory rows": cam.memory_rows(), "memory state": cam.memory_state()}
    for name, t in outputs.items():
        assert bool(torch.isfinite(t).all()), name
    assert int(cam.labels().max()) >= 1 and int(cam.nonfinite_rays.item()) == 0 and int(cam.map_nonfinite.item()) == 0
    assert bool(cam.map_known().any()) and bool((cam.mount != cam.mount_nominal).any())
    cam.stream_id = 5
    assert all(int(cam.stage(n).struct.stream_id) == 5 for n in ("odometry", "mount_jitter", "instrument", "capture"))
    cam.set_mount_jitter(None)
    assert cam.stage("capture").struct.rb.rc.mount == cam.ray_struct.mount == cam.mount.data_ptr() == cam.mount_nominal.data_ptr()
    assert cam.chain() == CHAIN[:1] + CHAIN[2:]
