"""CPU: the range-sensor options of envs/sensors.py as values -- the text every tool and learn/evaluate.py's command line takes for one, against
the object it must give, and the record spec() stores, through the constructor and through JSON."""
import json

import pytest

from isaacgymloco_amd.envs import sensors as S
from isaacgymloco_amd.learn import evaluate as E

GRID = [[x / 4.0, y / 4.0] for x in range(-2, 3) for y in range(-1, 2)]
TEXTS = [
    (E.parse_camera_jitter, "pos=0.01,rot_deg=1/2/3", S.MountJitter(pos=0.01, rot_deg=(1.0, 2.0, 3.0))),
    (E.parse_camera_jitter, "rot_deg=3", S.MountJitter(rot_deg=3.0)),
    (E.parse_camera_jitter, "pos=0.01/0.02/0.03", S.MountJitter(pos=(0.01, 0.02, 0.03))),
    (E.parse_camera_instrument, "latency=0:1,noise_gain=0.5:2,depth_scale=0.02,depth_quad=0.005,fov=0.02",
     S.InstrumentError(latency=(0, 1), noise_gain=(0.5, 2.0), depth_scale=0.02, depth_quad=0.005, fov=0.02)),
    (E.parse_camera_instrument, "fov=0.03", S.InstrumentError(fov=0.03)),
    (E.parse_camera_instrument, "latency=2:2", S.InstrumentError(latency=(2, 2))),
    (E.parse_odometry, "scale=0.02,yaw_per_m=0.01,z_per_m=0.01,noise=0.005:0.002:0.002",
     S.OdometryError(scale=0.02, yaw_per_m=0.01, z_per_m=0.01, noise=(0.005, 0.002, 0.002))),
    (E.parse_odometry, "yaw_per_m=0.4", S.OdometryError(yaw_per_m=0.4)),
    (S.parse_odometry, "scale=0.02,yaw_per_m=0.01,z_per_m=0.01,noise=0.005:0.002:0.002",
     S.OdometryError(scale=0.02, yaw_per_m=0.01, z_per_m=0.01, noise=(0.005, 0.002, 0.002))),
    (S.parse_odometry, "noise=0.1:0:0", S.OdometryError(noise=(0.1, 0.0, 0.0))),
    (S.parse_odometry, "", S.OdometryError()),
    (S.parse_odometry, "default", S.OdometryError()),
    (S.parse_elevation_map, "size=32,resolution=0.0625,source=noisy,max_range=3,unknown_drop=0.4",
     S.ElevationMap(size=32, resolution=0.0625, source="noisy", max_range=3.0, unknown_drop=0.4)),
    (S.parse_elevation_map, "size=16,source=clean", S.ElevationMap(size=16, source="clean")),
    (S.parse_elevation_map, "", S.ElevationMap()),
    (S.parse_elevation_map, "default", S.ElevationMap()),
    (lambda text: S.parse_option(S.SensorModel, text), "period=5,stagger=1,latency=1,frames=2,noise=0.01:0.002,dropout=0.02,drop_value=0,clip=0.1:3,normalise=1",
     S.SensorModel(period=5, stagger=True, latency=1, frames=2, noise=(0.01, 0.002), dropout=0.02, drop_value=0.0, clip=(0.1, 3.0), normalise=True)),
    (lambda text: S.parse_option(S.SensorModel, text), "period=3,stagger=0", S.SensorModel(period=3)),
    (lambda text: S.parse_option(S.SensorModel, text), "", S.SensorModel()),
    (lambda text: S.parse_option(S.MountJitter, text), "default", S.MountJitter()),
    (lambda text: S.parse_option(S.InstrumentError, text), "", S.InstrumentError()),
]
OBJECTS = [
    S.MountJitter(), S.MountJitter(pos=0.01, rot_deg=(1, 5, 1)),
    S.InstrumentError(), S.InstrumentError(latency=(0, 2), noise_gain=(0.5, 2), depth_scale=0.02, depth_quad=0.005, fov=0.02),
    S.ElevationMap(), S.ElevationMap(size=16, resolution=0.125, source="clean", max_range=3, points=GRID, unknown_drop=0.4),
    S.OdometryError(), S.OdometryError(scale=0.02, yaw_per_m=0.05, z_per_m=0.02, noise=(0.005, 0.002, 0.002)),
    S.SensorModel(), S.SensorModel(period=5, stagger=True, latency=1, frames=2, noise=(0.01, 0.002), dropout=0.02, drop_value=5.0, clip=(0.1, 3.0), normalise=True),
]
# what no text of the class may hold, with the key the error has to name: an unknown key, a key twice, no "=", a list of the wrong length
BAD = [
    (S.SensorModel, "rate=5", "rate"), (S.SensorModel, "period=5,period=6", "period"), (S.SensorModel, "stagger", "stagger"), (S.SensorModel, "noise=0.01", "noise"),
    (S.SensorModel, "clip=0:1:2", "clip"),
    (S.MountJitter, "yaw=3", "yaw"), (S.MountJitter, "pos=0.1,pos=0.2", "pos"), (S.MountJitter, "rot_deg", "rot_deg"), (S.MountJitter, "pos=1/2", "pos"),
    (S.InstrumentError, "gain=3", "gain"), (S.InstrumentError, "fov=0.1,fov=0.2", "fov"), (S.InstrumentError, "fov", "fov"),
    (S.InstrumentError, "latency=1", "latency"), (S.InstrumentError, "noise_gain=1:2:3", "noise_gain"),
    (S.ElevationMap, "cells=32", "cells"), (S.ElevationMap, "size=32,size=16", "size"), (S.ElevationMap, "source", "source"),
    (S.ElevationMap, "points=0:0", "points"),
    (S.OdometryError, "drift=0.1", "drift"), (S.OdometryError, "scale=0.1,scale=0.2", "scale"), (S.OdometryError, "scale", "scale"),
    (S.OdometryError, "noise=0.1:0.2", "noise"),
]


@pytest.mark.parametrize("parse,text,want", TEXTS, ids=[f"{p.__module__.split('.')[-1]}.{p.__name__}-{type(w).__name__}-{t or 'empty'}" for p, t, w in TEXTS])
def test_a_text_gives_the_object(parse, text, want):
    got = parse(text)
    assert type(got) is type(want) and got == want and got.record() == want.record()


@pytest.mark.parametrize("text", ["trained", "off"])
def test_evaluates_two_words_stand_above_the_grammar(text):
    want = "trained" if text == "trained" else None
    assert E.parse_camera_jitter(text) == want and E.parse_camera_instrument(text) == want and E.parse_odometry(text) == want


@pytest.mark.parametrize("obj", OBJECTS, ids=[f"{type(o).__name__}-{'defaults' if k % 2 == 0 else 'set'}" for k, o in enumerate(OBJECTS)])
def test_a_record_rebuilds_its_object_and_survives_json(obj):
    rec = obj.record()
    assert type(obj)(**rec) == obj and json.loads(json.dumps(rec)) == rec
    assert [o == obj for o in OBJECTS] == [o is obj for o in OBJECTS], "equal to itself alone: not to its class's other object, not to another class's"
    line = repr(obj)
    assert "\n" not in line and line.startswith(type(obj).__name__ + "(") and all(k + "=" in line for k in rec)
    with pytest.raises(TypeError):
        hash(obj)


@pytest.mark.parametrize("cls,text,key", BAD, ids=[f"{c.__name__}-{t}" for c, t, _ in BAD])
def test_a_text_outside_the_grammar_is_a_value_error_that_names_the_key(cls, text, key):
    with pytest.raises(ValueError, match=key):
        S.parse_option(cls, text)


def test_evaluates_parsers_refuse_what_only_the_tools_take_and_the_sensors_record_is_the_models():
    for parse in (E.parse_camera_jitter, E.parse_camera_instrument, E.parse_odometry):
        for text in ("", "default", "on"):
            with pytest.raises(ValueError):
                parse(text)
    m = S.SensorModel(period=5, stagger=True, latency=1, frames=2, noise=(0.01, 0.002), clip=(0.1, 3.0), normalise=True)
    assert m.record() == {"period": 5, "stagger": True, "latency": 1, "frames": 2, "noise": [0.01, 0.002], "dropout": 0.0, "drop_value": 0.0,
                          "clip": [0.1, 3.0], "normalise": True} and list(m.record()) == list(S.SensorModel.FIELDS)
    assert S.SensorModel().record()["clip"] is None and [type(v) for v in m.record().values()] == [int, bool, int, int, list, float, float, list, bool]
    assert "points=3" in repr(S.ElevationMap(points=GRID[:3])) and "points=None" in repr(S.ElevationMap())
