"""lsim_robot_model of a task's asset.  A module of its own, free of torch: the CPU oracle's timing process (oracle/cpu_bench.py) builds models
too, and a torch import there brings a second OpenMP runtime into the process (see its random_policy)."""
from . import aliengo


def build_robot_model(asset):
    """lsim_robot_model for cfg.asset (LR:1135-1219): the hand-checked Aliengo table, a URDF file if `asset.file` resolves to one, or a
    stored table of robots/tables/ (go1, go2, a1) chosen by `asset.name`."""
    import os
    from . import urdf
    pats = dict(penalize_contacts_on=tuple(asset.penalize_contacts_on), terminate_after_contacts_on=tuple(asset.terminate_after_contacts_on),
                foot_name=asset.foot_name)
    if asset.name == "aliengo":
        return aliengo.build_model(pats["penalize_contacts_on"], pats["terminate_after_contacts_on"], pats["foot_name"])
    path = str(asset.file).replace("{LEGGED_GYM_ROOT_DIR}", os.environ.get("LEGGED_GYM_ROOT_DIR", ""))
    if path and os.path.isfile(path):
        return urdf.build_model(path, **pats)[0]
    return urdf.build_model_from_table(asset.name, **pats)[0]


def robot_bodies(asset):
    """(bodies, names): the collapsed body list with its URDF collision primitives (`prims`) that build_robot_model's table came from"""
    import json
    import os
    from . import urdf
    if asset.name == "aliengo":
        bodies = aliengo.body_table()
        for b, prims in zip(bodies, aliengo._prims()):
            b["prims"] = prims
        return bodies, [b["name"] for b in bodies]
    path = str(asset.file).replace("{LEGGED_GYM_ROOT_DIR}", os.environ.get("LEGGED_GYM_ROOT_DIR", ""))
    if path and os.path.isfile(path):
        bodies = urdf.parse(path)[0]
    else:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "tables", asset.name + ".json")) as f:
            bodies = urdf.table_from_json(json.load(f))[0]
    return bodies, ["base" if i == 0 else b["name"] for i, b in enumerate(bodies)]


def build_sensor_table(asset):
    """(lsim_raycast_robot, body names) of cfg.asset for the body-aware range sensors: every collision primitive, cylinders as capsules when
    asset.replace_cylinder_with_capsule (robots/common.py, sensor_table)"""
    from .common import sensor_table
    bodies, names = robot_bodies(asset)
    return sensor_table(bodies, capsule=bool(getattr(asset, "replace_cylinder_with_capsule", True))), names
