"""tests/golden/urdf_aliengo_values.json: the values of the reference's aliengo.urdf that tests/test_model.py checks the hand table
against (per leg: hip and thigh-rotor masses, hip joint origin, calf joint limits, calf centre of mass, sign of the thigh's ixy; trunk mass).

    python tools/gen_golden_urdf.py PATH/TO/aliengo.urdf"""
import json
import os
import sys
import xml.etree.ElementTree as ET

LEGS = ("FL", "FR", "RL", "RR")


def extract(path):
    root = ET.parse(path).getroot()
    links = {l.get("name"): l for l in root.findall("link")}
    joints = {j.get("name"): j for j in root.findall("joint")}
    xyz = lambda e: [float(x) for x in e.get("xyz").split()]
    out = {"trunk_mass": float(links["trunk"].find("inertial").find("mass").get("value")), "legs": {}}
    for leg in LEGS:
        lim = joints[f"{leg}_calf_joint"].find("limit")
        out["legs"][leg] = {
            "hip_mass": float(links[f"{leg}_hip"].find("inertial").find("mass").get("value")),
            "thigh_rotor_mass": float(links[f"{leg}_thigh_rotor"].find("inertial").find("mass").get("value")),
            "hip_joint_origin": xyz(joints[f"{leg}_hip_joint"].find("origin")),
            "calf_limit_lower": float(lim.get("lower")), "calf_limit_effort": float(lim.get("effort")),
            "calf_com": xyz(links[f"{leg}_calf"].find("inertial").find("origin")),
            "thigh_ixy": float(links[f"{leg}_thigh"].find("inertial").find("inertia").get("ixy")),
        }
    return out


if __name__ == "__main__":
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "urdf_aliengo_values.json")
    with open(dst, "w") as f:
        json.dump(extract(sys.argv[1]), f, indent=1)
        f.write("\n")
