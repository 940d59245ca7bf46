"""What kind of policy a runner, a checkpoint or a bare module is, and the parts it brings: the one loader behind learn/evaluate.py,
learn/distill.py, the exporter and the tools.  The kinds share VisionActorCritic's "some [N, dim] rows behind the latent": "him" (none),
"vision" (the depth encoder's latent, with a memory [z | h]), "map" (the elevation map's rows), "scan" (the scan block of the privileged
observation).  A runner names its kind in `policy_kind`, a checkpoint by the record it carries (policy_record), a bare module not at all
(the heuristic of policy_parts)."""
import dataclasses

import torch

_RECORD_KEY = {"vision": "vision", "map": "map_policy", "scan": "scan_policy"}      # kind -> the checkpoint key of its record
# (checkpoint key, attribute of the learner): the modules and optimisers a learner may own beside the actor-critic; None or absent: not saved
CHECKPOINT_PARTS = (("depth_encoder_state_dict", "encoder"), ("depth_head_state_dict", "depth_head"), ("depth_optimizer_state_dict", "aux_optimizer"),
                    ("depth_memory_state_dict", "memory"), ("depth_memory_head_state_dict", "memory_head"),
                    ("depth_memory_optimizer_state_dict", "memory_optimizer"), ("depth_e2e_optimizer_state_dict", "e2e_optimizer"))


@dataclasses.dataclass
class PolicyParts:
    """a policy and what it brings along; None: the kind has none, or nobody brought it"""
    kind: str                       # "him", "vision", "map" or "scan"
    actor_critic: torch.nn.Module
    sensor: object = None           # the live sensor: the caller's, else the runner's
    sensor_record: dict = None      # the sensor's spec() as a checkpoint stores it
    encoder: torch.nn.Module = None
    depth_head: torch.nn.Module = None
    memory: torch.nn.Module = None
    memory_head: torch.nn.Module = None
    channels: tuple = None          # a map policy's row channels
    scan: dict = None               # a scan policy's {"offset", "width", "dim"}
    checkpoint: dict = None         # the loaded checkpoint


def check_conventions(saved, live):
    """refuse a checkpoint made under other simulator conventions or another robot mix, naming the first differing key"""
    if saved is None:
        return
    for k in ("robots", "lin_vel_at_com", "tgs_limit_passes", "solver_type", "num_position_iterations"):
        if saved.get(k) != live.get(k):
            raise ValueError(f"checkpoint conventions differ from the env's in {k!r}: saved {saved.get(k)!r}, live {live.get(k)!r}")


def layer_widths(sd):
    """(actor, critic, estimator encoder) of a model state dict: each network's layer widths, in order"""
    widths = lambda prefix: [sd[k].shape[0] for k in sorted((k for k in sd if k.startswith(prefix) and k.endswith(".weight")), key=lambda k: int(k.split(".")[-2]))]
    return widths("actor."), widths("critic."), widths("estimator.encoder.")


def actor_critic_from_state_dict(env, sd, device=None, rows=False, activation="elu"):
    """the HIMActorCritic for `env` with the hidden widths of `sd`, loaded; `rows`: a VisionActorCritic when actor.0.weight has more columns
    than a HIM actor reads -- they come last (learn/vision.py) and are its depth_latent_dim"""
    from .modules import HIMActorCritic
    from .vision import VisionActorCritic
    actor, critic, enc = layer_widths(sd)
    extra = sd["actor.0.weight"].shape[1] - (env.num_one_step_obs + 3 + 16)
    cls, more = (VisionActorCritic, {"depth_latent_dim": extra}) if rows and extra > 0 else (HIMActorCritic, {})
    ac = cls(env.num_obs, env.num_privileged_obs if env.num_privileged_obs is not None else env.num_obs, env.num_one_step_obs, env.num_actions,
             actor_hidden_dims=tuple(actor[:-1]), critic_hidden_dims=tuple(critic[:-1]), activation=activation, init_noise_std=1.0, **more).to(device)
    if enc != [l.out_features for l in ac.estimator.encoder if isinstance(l, torch.nn.Linear)]:
        raise ValueError(f"checkpoint estimator encoder widths {enc} differ from the default HIMEstimator's: pass the HIMActorCritic itself")
    ac.load_state_dict(sd)
    return ac


def policy_record(d):
    """(kind, record) of a checkpoint dict: the kind whose record it carries and that record; {} for a HIM policy, and for a vision
    checkpoint from before the record"""
    for kind in ("scan", "map", "vision"):
        if _RECORD_KEY[kind] in d:
            return kind, d[_RECORD_KEY[kind]] or {}
    return ("vision" if "depth_encoder_state_dict" in d else "him"), {}


def checkpoint_state(alg, kind, record):
    """what the runner of a policy of `kind` adds to its checkpoint: the state dict of every part of CHECKPOINT_PARTS the learner `alg` has,
    and the kind's `record` under its key"""
    return {_RECORD_KEY[kind]: record, **{key: getattr(alg, attr).state_dict() for key, attr in CHECKPOINT_PARTS if getattr(alg, attr, None) is not None}}


def load_checkpoint_state(alg, d):
    """the reverse: every part the learner has and the checkpoint `d` holds"""
    for key, attr in CHECKPOINT_PARTS:
        if getattr(alg, attr, None) is not None and key in d:
            getattr(alg, attr).load_state_dict(d[key])


def _record_fields(kind, record):
    """the fields of PolicyParts a kind's record fills: a runner's policy_record() and its checkpoint's record say the same"""
    return {"sensor_record": record.get("sensor"), "channels": tuple(record["channels"]) if kind == "map" and record.get("channels") else None,
            "scan": dict(record) if kind == "scan" else None}


def _from_checkpoint(env, d, device, encoder):
    from .depth_encoder import DepthEncoder
    from .depth_memory import DepthMemory
    check_conventions((d.get("env_state_dict") or {}).get("conventions"), env._conventions())
    kind, record = policy_record(d)
    ac = actor_critic_from_state_dict(env, d["model_state_dict"], device, rows=kind != "him")
    kind = kind if hasattr(ac, "depth_latent_dim") else "him"
    parts = PolicyParts(kind, ac.eval(), checkpoint=d, **_record_fields(kind, record))
    if kind == "vision":
        state = {attr: d[key] for key, attr in CHECKPOINT_PARTS if key in d}
        heads = {name: torch.nn.Linear(*reversed(state[name]["weight"].shape)) for name in ("depth_head", "memory_head") if name in state}
        for name, head in heads.items():
            head.load_state_dict(state[name])
        parts.encoder = encoder if encoder is not None else DepthEncoder(**record["encoder"]) if record.get("encoder") is not None else None
        if parts.encoder is not None:
            parts.encoder.load_state_dict(state["encoder"])
        parts.depth_head = heads.get("depth_head")
        if record.get("memory") is not None:            # a policy trained with a depth memory
            parts.memory, parts.memory_head = DepthMemory(**record["memory"]), heads.get("memory_head")
            parts.memory.load_state_dict(state["memory"])
    return parts


def _from_runner(runner):
    runner.get_inference_policy()           # flushes a deferred rollout store, eval mode
    kind, alg = runner.policy_kind, runner.alg
    own = {attr: getattr(alg, attr, None) for _, attr in CHECKPOINT_PARTS if attr in PolicyParts.__dataclass_fields__}      # encoder, head, memory, its head
    return PolicyParts(kind, alg.actor_critic, sensor=getattr(runner, "sensor", None), **own,
                       **_record_fields(kind, runner.policy_record() if kind != "him" else {}))


def policy_parts(env, policy, device=None, sensor=None, encoder=None, depth_head=None):
    """The PolicyParts of `policy`: a HIMActorCritic (a VisionActorCritic is one), a runner, or a checkpoint written by runner.save (its
    path or the loaded dict; refused when made under other conventions than `env`'s).  `sensor`, `encoder`, `depth_head`: the caller's
    own, which take the place of what the policy brings -- a checkpoint's encoder weights are loaded into the caller's encoder, and a
    vision checkpoint without a record of its encoder and without the caller's has encoder None.
    A bare module says nothing of its kind, so one heuristic decides: a VisionActorCritic with no encoder anywhere and a `sensor` whose map
    rows are attached is a map policy, any other VisionActorCritic a vision policy."""
    from .modules import HIMActorCritic
    if isinstance(policy, HIMActorCritic):
        is_map = encoder is None and getattr(sensor, "map_channels", None) is not None
        parts = PolicyParts(("map" if is_map else "vision") if hasattr(policy, "depth_latent_dim") else "him", policy)
    elif getattr(policy, "policy_kind", None) is not None:
        parts = _from_runner(policy)
    elif isinstance(policy, (str, dict)):
        d = torch.load(policy, map_location=device, weights_only=False) if isinstance(policy, str) else policy
        parts = _from_checkpoint(env, d, device, encoder)
    else:
        raise TypeError(f"policy must be a HIMActorCritic, a runner or a checkpoint path, got {type(policy).__name__}")
    given = {"sensor": sensor, "encoder": encoder, "depth_head": depth_head}
    return dataclasses.replace(parts, **{name: part for name, part in given.items() if part is not None})
