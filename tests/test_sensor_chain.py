"""CPU: the chain of stages behind RaySensor.update() (envs/sensors.py) -- which entry points are launched, in which order, with which tick,
flags, seed, rank and stream id, where the one ray struct points, and what is left when everything is detached again -- over every
combination of the options, on the emulated LeggedRobot with every launch through the CPU builds of the kernel sources.  What each launch
computes is held to its reference in the tests of that launch."""
import gc
import itertools
import weakref

import pytest
import torch

import odometry_emu_binding as OB
from helpers import abi
from isaacgymloco_amd.envs import sensors
from isaacgymloco_amd.learn.depth_encoder import DepthEncoder
from isaacgymloco_amd.learn.depth_memory import DepthMemory
from test_elevation_map_chain import ENC, _camera, _env, _logged
from test_map_policy_chain import ODO

N = 8
FILL_ALL, RESETS_ONLY = abi.DEFINES["LSIM_SENSOR_FILL_ALL"], abi.DEFINES["LSIM_SENSOR_RESETS_ONLY"]
JITTER = sensors.MountJitter(pos=0.01, rot_deg=(1, 5, 1))
INSTRUMENT = sensors.InstrumentError(latency=(0, 1), noise_gain=(0.5, 2.0), depth_scale=0.02, depth_quad=0.005, fov=0.02)
SHARED = ("tick", "flags", "seed", "rank", "stream_id")
MAPS = {"none": (False, False, False), "map": (True, False, False), "map+odometry": (True, True, False), "map+rows": (True, False, True),
        "map+odometry+rows": (True, True, True)}
ENCODERS = {"none": (False, False), "encoder": (True, False), "encoder+memory": (True, True)}
ENTRIES = ("lsim_raycast", "lsim_raycast_bodies", "lsim_odometry_step", "lsim_sensor_mount_jitter", "lsim_sensor_instrument", "lsim_sensor_capture",
           "lsim_sensor_capture_inst", "lsim_elevation_map", "lsim_map_rows", "lsim_depth_encode", "lsim_depth_memory_step")


@pytest.fixture(scope="module")
def rig():
    """one emulated env and one api for every case; each case starts from an env without sensors and an empty log"""
    env, api = _env(N), OB.EmuApi()
    torch.manual_seed(2)
    return env, api, _logged(api, ENTRIES), DepthEncoder(12, 16, 2, **ENC), DepthMemory(ENC["latent_dim"], 9, 16)


def _chain_of(jitter, instrument, emap, odometry, rows, encoder, memory):
    """the fixed launch order, filtered to what is attached"""
    order = (("lsim_odometry_step", odometry), ("lsim_sensor_mount_jitter", jitter), ("lsim_sensor_instrument", instrument),
             ("lsim_sensor_capture_inst" if instrument else "lsim_sensor_capture", True), ("lsim_elevation_map", emap), ("lsim_map_rows", rows),
             ("lsim_depth_encode", encoder), ("lsim_depth_memory_step", memory))
    return tuple(e for e, on in order if on)


def _shared(cam):
    """{entry: (tick, flags, seed, rank, stream_id) as far as the stage's struct has them}"""
    stages = [s for s in map(cam.stage, sensors._ORDER) if s is not None and s.struct is not None]
    return {s.entry: {f: int(getattr(s.struct, f)) for f in SHARED if hasattr(s.struct, f)} for s in stages}


def _mounts(cam):
    """the mount pointer through every view of the launched struct"""
    views = [cam.stage("capture").struct.rb.rc.mount, cam.ray_struct.mount] + ([] if cam.bodies_struct is None else [cam.bodies_struct.rc.mount])
    assert len(set(views)) == 1
    return views[0]


def _run_case(rig, jitter, instrument, emap, odometry, rows, encoder, memory, **bodies):
    env, api, log, enc, mem = rig
    env.sensors.clear()
    bare = _camera(env, api, 16, 12, **bodies)
    cam = _camera(env, api, 16, 12, mount_jitter=JITTER if jitter else None, instrument=INSTRUMENT if instrument else None, **bodies)
    if emap:
        cam.attach_map(sensors.ElevationMap(size=16), odometry=ODO if odometry else None)
    if rows:
        cam.attach_map_rows(("height", "known"))
    if encoder:
        cam.attach_encoder(enc)
    if memory:
        cam.attach_memory(mem)              # the one attach that launches before the sensor has captured
    want = _chain_of(jitter, instrument, emap, odometry, rows, encoder, memory)
    assert cam.chain() == want and bare.chain() == ("lsim_sensor_capture",)
    assert [n for n in sensors._ORDER if cam.stage(n) is not None] == [n for n, on in zip(sensors._ORDER, (False, odometry, jitter, instrument, True, emap, rows, encoder, memory)) if on]
    del log[:]

    def launched(tick, flags, times):
        assert tuple(log) == want * times, "the log is the chain, repeated"
        shared = _shared(cam)
        assert set(shared) == {e for e in want if e not in ("lsim_depth_encode", "lsim_depth_memory_step")}      # those two build their struct per launch
        capture = shared["lsim_sensor_capture_inst" if instrument else "lsim_sensor_capture"]
        assert capture == dict(zip(SHARED, (tick, flags, int(env.lcfg.seed), int(env.lcfg.rank), cam.stream_id))) and cam.tick == tick
        for entry, fields in shared.items():
            assert fields == {f: capture[f] for f in fields}, entry

    tick = int(env.common_step_counter)
    env.add_sensor("depth", cam)
    launched(tick, FILL_ALL, 1)
    for step in range(2):
        tick = int(env.common_step_counter)
        env.step_device(torch.zeros(N, 12))
        launched(tick, 0, 2 + step)
    env.reset_idx([1])
    launched(int(env.common_step_counter), RESETS_ONLY, 4)
    cam.stream_id = 5
    assert cam.stream_id == 5 and all(f["stream_id"] == 5 for f in _shared(cam).values() if "stream_id" in f)

    # _point_mount writes the one field every view reads
    assert _mounts(cam) == cam.mount.data_ptr() and (cam.mount is not cam.mount_nominal) == bool(jitter)
    cam.set_mount_jitter(JITTER)
    assert _mounts(cam) == cam.mount.data_ptr() != cam.mount_nominal.data_ptr() and cam.stage("mount_jitter").struct.stream_id == 5
    refs = [weakref.ref(t) for n in sensors._ORDER if cam.stage(n) is not None and n != "capture" for t in cam.stage(n).buffers.values()]
    assert len(refs) == 1 + instrument + 8 * emap + 2 * odometry + rows + encoder + 2 * memory and all(r() is not None for r in refs)

    # detach everything: the sensor that was built without the options
    cam.set_mount_jitter(None)
    cam.set_instrument(None)
    assert cam.attach_map(None) is None and cam.attach_encoder(None) is None
    assert _mounts(cam) == cam.mount.data_ptr() == cam.mount_nominal.data_ptr() and cam.mount is cam.mount_nominal
    assert cam.chain() == bare.chain() and list(cam.spec()) == list(bare.spec())
    assert all(cam.stage(n) is None for n in sensors._ORDER if n != "capture")
    assert (cam.mount_jitter, cam.instrument, cam.map, cam.odometry, cam.map_channels, cam.encoder, cam.memory) == (None,) * 7
    gc.collect()
    assert [r() for r in refs] == [None] * len(refs), "a detached stage's buffers die with it"
    del log[:]
    env.step_device(torch.zeros(N, 12))
    assert tuple(log) == bare.chain()


@pytest.mark.parametrize("jitter,instrument,emap,encoder", list(itertools.product((False, True), (False, True), MAPS, ENCODERS)),
                         ids=lambda v: v if isinstance(v, str) else "on" if v else "off")
def test_every_combination_launches_its_chain_in_the_fixed_order_and_detaches_to_the_bare_sensor(rig, jitter, instrument, emap, encoder):
    _run_case(rig, jitter, instrument, *MAPS[emap], *ENCODERS[encoder])


def test_the_full_chain_on_a_sensor_that_sees_the_robot_and_labels_it(rig):
    _run_case(rig, True, True, True, True, True, True, True, see_robot=True, labels=True)


def test_without_a_model_the_chain_is_the_one_ray_stage_and_tick_and_flags_are_ignored(rig):
    env, api, log, *_ = rig
    for kw, entry in ((dict(), "lsim_raycast"), (dict(see_robot=True, labels=True), "lsim_raycast_bodies")):
        cam = _camera(env, api, 16, 12, model=None, **kw)
        assert cam.chain() == (entry,) and cam.stage("rays").struct is (cam.ray_struct if cam.bodies_struct is None else cam.bodies_struct)
        flags = int(cam.stage("rays").struct.flags) if kw else 0
        del log[:]
        cam.update(tick=7, flags=FILL_ALL)
        assert log == [entry] and not hasattr(cam, "tick") and (not kw or int(cam.bodies_struct.flags) == flags)
        cam.stream_id = 5
        assert cam.stream_id == 0 and cam.ray_struct.mount == cam.mount.data_ptr()
