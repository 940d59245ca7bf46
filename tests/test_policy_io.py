"""CPU: learn/policy_io.py -- the kind and the parts of a policy from a runner, from its checkpoint and from a bare module, the checkpoint's
keys, and the refusals of evaluate() and DistillRunner that go through it -- on the emulated env of tests/policy_cases.py (8 envs, a
16 x 12 camera), every launch through the CPU builds of the kernel sources."""
import json

import numpy as np
import pytest
import torch

import eval_columns_emu_binding as CB
import policy_cases as PC
from isaacgymloco_amd.learn import policy_io
from isaacgymloco_amd.learn.depth_encoder import DepthEncoder
from isaacgymloco_amd.learn.evaluate import Evaluator, evaluate
from isaacgymloco_amd.learn.modules import HIMActorCritic
from isaacgymloco_amd.learn.vision import VisionActorCritic

HIM_KEYS = ["env_state_dict", "estimator_optimizer_state_dict", "infos", "iter", "learning_rate", "model_state_dict", "optimizer_state_dict"]
VISION_KEYS = ["depth_encoder_state_dict", "depth_head_state_dict", "depth_optimizer_state_dict", "vision"]
ENCODER_KEYS = ["c1", "c2", "final_act", "frames", "height", "k1", "k2", "latent_dim", "s1", "s2", "width"]
E2E_KEYS = {"": sorted(HIM_KEYS + VISION_KEYS + ["depth_e2e_optimizer_state_dict"]), "vision": ["encoder", "end_to_end", "latent_dim", "sensor"],
            "vision.encoder": ENCODER_KEYS, "vision.end_to_end": ["capacity", "epochs", "learning_rate"]}
KEYS = {
    "him": {"": HIM_KEYS},
    "vision": {"": sorted(HIM_KEYS + VISION_KEYS), "vision": ["encoder", "latent_dim", "sensor"], "vision.encoder": ENCODER_KEYS},
    "vision_memory": {"": sorted(HIM_KEYS + VISION_KEYS + ["depth_memory_head_state_dict", "depth_memory_optimizer_state_dict", "depth_memory_state_dict"]),
                      "vision": ["encoder", "latent_dim", "memory", "sensor"], "vision.encoder": ENCODER_KEYS,
                      "vision.memory": ["hidden", "latent_dim", "proprio_dim"]},
    "vision_e2e": E2E_KEYS,
    "distill": dict(E2E_KEYS, **{"": sorted(E2E_KEYS[""] + ["distill"]), "distill": ["distill_optimizer_state_dict", "epochs", "learning_rate", "teacher"],
                                 "distill.teacher": ["dim", "offset", "width"]}),
    "map": {"": sorted(HIM_KEYS + ["map_policy"]), "map_policy": ["channels", "dim", "sensor"]},
    "scan": {"": sorted(HIM_KEYS + ["scan_policy"]), "scan_policy": ["dim", "offset", "width"]},
}
MODULES = ("actor_critic", "encoder", "depth_head", "memory", "memory_head")


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    """case -> (env, runner, path of the runner's checkpoint), each case built and saved once"""
    made, where = {}, tmp_path_factory.mktemp("policy_io")

    def get(case):
        if case not in made:
            env, run = PC.build(case)
            run.save(str(where / f"{case}.pt"))
            made[case] = env, run, str(where / f"{case}.pt")
        return made[case]
    return get


def _evaluate(env, policy, **kw):
    return evaluate(env, policy, 3, commands=(0.5, 0.0, 0.0), evaluator=Evaluator(env, api=CB.EmuApi()), **kw)


@pytest.mark.parametrize("case", PC.CASES)
def test_a_checkpoint_has_the_keys_it_had_before_the_loader(saved, case):
    """The top-level keys and the keys of each nested record, for every kind of runner.  The literals were recorded by running
    policy_cases.build(case) and runner.save on the commit BEFORE learn/policy_io.py existed, not from the code under test."""
    d = torch.load(saved(case)[2], weights_only=False)
    assert PC.key_sets(d) == KEYS[case]


@pytest.mark.parametrize("case,kind", [("him", "him"), ("vision", "vision"), ("vision_memory", "vision"), ("map", "map"), ("scan", "scan")])
def test_the_runner_and_its_checkpoint_give_the_same_parts_and_the_same_evaluation(tmp_path, case, kind):
    (env, run), path = PC.build(case), str(tmp_path / "model.pt")
    run.save(path)
    env2 = PC.build(case)[0]                    # the same construction again: an identically seeded env with the same sensor in the same state
    a, b = policy_io.policy_parts(env, run), policy_io.policy_parts(env2, path, "cpu")
    assert a.kind == b.kind == kind and a.checkpoint is None and sorted(b.checkpoint) == KEYS[case][""]
    assert a.channels == b.channels and a.scan == b.scan and a.sensor_record == b.sensor_record
    assert (a.channels, a.scan is None, a.sensor_record is None) == {"map": (("height", "known"), True, False), "scan": (None, False, True),
                                                                      "vision": (None, True, False), "him": (None, True, True)}[kind]
    assert a.sensor is getattr(run, "sensor", None) and b.sensor is None
    for name in MODULES:
        ma, mb = getattr(a, name), getattr(b, name)
        assert (ma is None) == (mb is None), name
        if ma is not None:
            sa, sb = ma.state_dict(), mb.state_dict()
            assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa), name
    assert [n for n in MODULES if getattr(a, n) is not None] == {"vision": list(MODULES[:3]), "vision_memory": list(MODULES)}.get(case, ["actor_critic"])
    ev_a, ev_b = _evaluate(env, run), _evaluate(env2, path)
    np.testing.assert_array_equal(ev_a.table.numpy(), ev_b.table.numpy())
    assert (ev_a.col_table is None) == (ev_b.col_table is None) == (kind in ("him", "scan"))
    if ev_a.col_table is not None:
        np.testing.assert_array_equal(ev_a.col_table.numpy(), ev_b.col_table.numpy())
    ra, rb = ev_a.result(), ev_b.result()
    assert ra["conventions"] == rb["conventions"] and json.dumps(ra, sort_keys=True) == json.dumps(rb, sort_keys=True)
    assert ra["total"]["samples"] > 0


def test_a_bare_module_is_a_map_policy_only_with_map_rows_and_no_encoder():
    env = PC.env()
    cam = PC.camera(env, with_map=True)
    rows = cam.attach_map_rows(("height", "known"))
    ac = VisionActorCritic(env.num_obs, env.num_privileged_obs, env.num_one_step_obs, env.num_actions, depth_latent_dim=rows.shape[1])
    enc = DepthEncoder(12, 16, 2, **PC.ENC)
    parts = policy_io.policy_parts(env, ac, sensor=cam)
    assert parts.kind == "map" and parts.sensor is cam and parts.actor_critic is ac and parts.encoder is None and parts.checkpoint is None
    with_encoder = policy_io.policy_parts(env, ac, sensor=cam, encoder=enc)
    assert with_encoder.kind == "vision" and with_encoder.encoder is enc
    assert policy_io.policy_parts(env, ac).kind == "vision", "no sensor, so no map rows"
    assert policy_io.policy_parts(env, ac, sensor=PC.camera(PC.env())).kind == "vision", "a sensor without map rows"
    him = HIMActorCritic(env.num_obs, env.num_privileged_obs, env.num_one_step_obs, env.num_actions)
    assert policy_io.policy_parts(env, him, sensor=cam).kind == "him"
    with pytest.raises(TypeError, match="policy must be a HIMActorCritic, a runner or a checkpoint path, got int"):
        policy_io.policy_parts(env, 3)
    assert _evaluate(env, ac, sensor=cam, vision_metrics=("map_coverage",)).result()["conventions"]["columns"] == ["map_coverage"]


def test_the_refusals_of_before_come_through_the_loader_with_their_messages(saved):
    from isaacgymloco_amd.learn.distill import DistillRunner
    env, run, path = saved("vision")
    d = torch.load(path, weights_only=False)
    bare = {k: v for k, v in d.items() if k != "vision"}
    assert policy_io.policy_record(bare) == ("vision", {}) and policy_io.policy_record(d) == ("vision", d["vision"])
    with pytest.raises(ValueError, match=r"evaluate: the checkpoint has no 'vision' record \(vision\['encoder'\], the depth encoder's hyperparameters\)"):
        _evaluate(env, bare)
    wide = DepthEncoder(12, 16, 2, **dict(PC.ENC, latent_dim=PC.L + 2))
    with pytest.raises(ValueError, match=f"evaluate: the encoder's latent has {PC.L + 2} columns, the actor reads {PC.L}"):
        _evaluate(env, run.alg.actor_critic, sensor=run.sensor, encoder=wide)
    with pytest.raises(ValueError, match="evaluate: a vision policy needs a sensor with a SensorModel"):
        _evaluate(PC.env(), path)
    map_path, scan_path = saved("map")[2], saved("scan")[2]
    no_map = PC.env()
    with pytest.raises(ValueError, match="evaluate: a map policy needs a sensor with an elevation map"):
        _evaluate(no_map, map_path, sensor=PC.camera(no_map))
    with pytest.raises(ValueError, match="evaluate: a scan policy reads the privileged height scan itself -- it has no sensor, encoder or map, so no vision"):
        _evaluate(saved("scan")[0], scan_path, vision_metrics=("depth_influence",))
    for teacher in (map_path, saved("him")[2], d):
        with pytest.raises(ValueError, match=r"DistillRunner: the teacher's checkpoint has no 'scan_policy' record \(it is no ScanOnPolicyRunner's\)"):
            DistillRunner(env, PC.train_cfg(), teacher=teacher, sensor=run.sensor)
    with pytest.raises(TypeError, match="DistillRunner: teacher is a checkpoint path, a loaded checkpoint dict or a ScanOnPolicyRunner"):
        DistillRunner(env, PC.train_cfg(), teacher=saved("map")[1], sensor=run.sensor)
