"""ctypes mirror of include/lsim.h, generated at import time by parsing the header.

The header is the single source of truth for the C-ABI (struct layouts, enums,
#defines and function prototypes); parsing it here means a field added to `lsim_config`
or a parameter added to an entry point can never silently disagree with the Python side.
`lsim_sizeof_config()` / `lsim_sizeof_model()` are checked against these mirrors when a
library is loaded (see `check_abi`); `bind` types a library's functions from `PROTOTYPES`.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
REPO_ROOT = os.path.dirname(_HERE)
HEADER_PATH = os.path.join(REPO_ROOT, "include", "lsim.h")

_CTYPES = {
    "float": ctypes.c_float, "double": ctypes.c_double,
    "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32,
    "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
    "int16_t": ctypes.c_int16, "uint8_t": ctypes.c_uint8, "int": ctypes.c_int,
}


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _parse(text, overrides=None):
    """`overrides`: values for the header's #ifndef-guarded defines, as a build with -DNAME=value sees them (test-only oracle variants)"""
    text = _strip_comments(text)
    defines = {}
    for m in re.finditer(r"^\s*#define\s+(\w+)\s+(.+?)\s*$", text, flags=re.M):
        name, expr = m.group(1), m.group(2)
        expr = re.sub(r"(\d+)u\b", r"\1", expr)
        if overrides and name in overrides:
            defines[name] = int(overrides[name])
            continue
        try:
            defines[name] = int(eval(expr, {}, dict(defines)))  # only integer arithmetic on earlier defines
        except Exception:
            pass
    enums = {}
    for m in re.finditer(r"enum\s+(\w+)\s*\{(.*?)\}", text, flags=re.S):
        val = -1
        members = {}
        for item in m.group(2).split(","):
            item = item.strip()
            if not item:
                continue
            if "=" in item:
                k, v = item.split("=")
                val = int(eval(v, {}, {**defines, **members}))
                members[k.strip()] = val
            else:
                val += 1
                members[item] = val
        enums[m.group(1)] = members
        defines.update(members)
    for m in re.finditer(r"^\s*#define\s+(\w+)\s+(.+?)\s*$", text, flags=re.M):   # second pass: defines that use enum members
        name, expr = m.group(1), re.sub(r"(\d+)u\b", r"\1", m.group(2))
        if name not in defines:
            try:
                defines[name] = int(eval(expr, {}, dict(defines)))
            except Exception:
                pass
    structs = {}
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        fields = []
        for stmt in m.group(2).split(";"):
            stmt = " ".join(stmt.split())
            if not stmt:
                continue
            if stmt.startswith("const "):
                stmt = stmt[len("const "):]
            ty, rest = stmt.split(" ", 1)
            if ty.endswith("*"):                         # pointer members (device pointers) bind as void*
                base = ctypes.c_void_p
            else:
                base = structs[ty] if ty in structs else _CTYPES[ty]
            for decl in rest.split(","):
                decl = decl.strip()
                dm = re.match(r"(\w+)((?:\[[^\]]+\])*)$", decl)
                name, dims = dm.group(1), re.findall(r"\[([^\]]+)\]", dm.group(2))
                ct = base
                for d in reversed(dims):
                    ct = ct * int(eval(d, {}, defines))
                fields.append((name, ct))
        structs[m.group(3)] = type(m.group(3), (ctypes.Structure,), {"_fields_": fields})
    return defines, enums, structs


with open(HEADER_PATH) as _f:
    DEFINES, ENUMS, STRUCTS = _parse(_f.read())

LsimConfig = STRUCTS["lsim_config"]
LsimRobotModel = STRUCTS["lsim_robot_model"]
LsimBody = STRUCTS["lsim_body"]
LsimCollisionPoint = STRUCTS["lsim_collision_point"]
LsimRolloutStorage = STRUCTS["lsim_rollout_storage"]
LsimMlpLayer = STRUCTS["lsim_mlp_layer"]
LsimHimPolicy = STRUCTS["lsim_him_policy"]
LsimPolicyExtra = STRUCTS["lsim_policy_extra"]
LsimWgradPending = STRUCTS["lsim_wgrad_pending"]
LsimAmpDisc = STRUCTS["lsim_amp_disc"]
LsimEval = STRUCTS["lsim_eval"]
LsimEvalColumns = STRUCTS["lsim_eval_columns"]
LsimRaycast = STRUCTS["lsim_raycast_t"]
LsimRaycastBodies = STRUCTS["lsim_raycast_bodies_t"]
LsimRaycastRobot = STRUCTS["lsim_raycast_robot"]
LsimRaycastPrim = STRUCTS["lsim_raycast_prim"]
LsimSensorModel = STRUCTS["lsim_sensor_model_t"]
LsimSensorMountJitter = STRUCTS["lsim_sensor_mount_jitter_t"]
LsimSensorInstrument = STRUCTS["lsim_sensor_instrument_t"]
LsimSensorStereo = STRUCTS["lsim_sensor_stereo_t"]
LsimSensorShade = STRUCTS["lsim_sensor_shade_t"]
LsimElevationMap = STRUCTS["lsim_elevation_map_t"]
LsimOdometry = STRUCTS["lsim_odometry_t"]
LsimMapRows = STRUCTS["lsim_map_rows_t"]
LsimElevationMapFused = STRUCTS["lsim_elevation_map_fused_t"]
LsimMapRowsFused = STRUCTS["lsim_map_rows_fused_t"]
LsimElevationMapCleanup = STRUCTS["lsim_elevation_map_cleanup_t"]
LsimFootScan = STRUCTS["lsim_foot_scan_t"]
LsimDepthEncoder = STRUCTS["lsim_depth_encoder_t"]
LsimDepthEncoderBwd = STRUCTS["lsim_depth_encoder_bwd_t"]
LsimFramesLog = STRUCTS["lsim_frames_log_t"]
LsimLatentRowsGrad = STRUCTS["lsim_latent_rows_grad_t"]
LsimDistillLoss = STRUCTS["lsim_distill_loss_t"]

REWARD_IDS = {k[len("LSIM_R_"):].lower(): v for k, v in ENUMS["lsim_reward_id"].items() if k.startswith("LSIM_R_")}
NUM_REWARD_TERMS = ENUMS["lsim_reward_id"]["LSIM_NUM_REWARD_TERMS"]
REWARD_NAMES = [n for n, _ in sorted(REWARD_IDS.items(), key=lambda kv: kv[1])]
BUFFER_IDS = {k[len("LSIM_BUF_"):].lower(): v for k, v in ENUMS["lsim_buffer_id"].items() if k.startswith("LSIM_BUF_")}
NUM_BUFFERS = ENUMS["lsim_buffer_id"]["LSIM_NUM_BUFFERS"]
RNG_TAGS = {k[len("LSIM_RNG_"):].lower(): v for k, v in ENUMS["lsim_rng_tag"].items()}

DT_F32, DT_I64, DT_U8, DT_I32, DT_I16 = (DEFINES[k] for k in ("LSIM_DT_F32", "LSIM_DT_I64", "LSIM_DT_U8", "LSIM_DT_I32", "LSIM_DT_I16"))
E_INVALID, E_NOMEM, E_HIP, E_UNSUPPORTED, E_ABI = (DEFINES[k] for k in ("LSIM_E_INVALID", "LSIM_E_NOMEM", "LSIM_E_HIP", "LSIM_E_UNSUPPORTED", "LSIM_E_ABI"))
ABI_VERSION = DEFINES["LSIM_ABI_VERSION"]
RAYCAST_PRIM_KINDS = {k[len("LSIM_RAYCAST_PRIM_"):].lower(): v for k, v in DEFINES.items() if k.startswith("LSIM_RAYCAST_PRIM_")}
RAYCAST_FRAME_YAW = DEFINES["LSIM_RAYCAST_FRAME_YAW"]
STEP_SKIP_PHYSICS = DEFINES["LSIM_STEP_SKIP_PHYSICS"]
STEP_NO_RESET = DEFINES["LSIM_STEP_NO_RESET"]
STEP_RECORD_SUBSTEPS = DEFINES["LSIM_STEP_RECORD_SUBSTEPS"]
STEP_TWO_KERNELS = DEFINES["LSIM_STEP_TWO_KERNELS"]
STEP_FLAT_PRIORITY = DEFINES["LSIM_STEP_FLAT_PRIORITY"]
EVAL_WORDS = {k[len("LSIM_EVAL_W_"):].lower(): v for k, v in ENUMS["lsim_eval_word"].items() if k.startswith("LSIM_EVAL_W_")}
NUM_EVAL_WORDS = ENUMS["lsim_eval_word"]["LSIM_EVAL_WORDS"]
STATS = {k[len("LSIM_STATS_"):].lower(): v for k, v in DEFINES.items() if k.startswith("LSIM_STATS_")}


def structs_for(overrides):
    """struct mirrors of a library compiled with -DNAME=value overrides of the header's guarded defines (oracle variants only)"""
    with open(HEADER_PATH) as f:
        return _parse(f.read(), overrides)[2]


_SCALARS = {**_CTYPES, "long": ctypes.c_long, "size_t": ctypes.c_size_t, "lsim_handle": ctypes.c_void_p}
_RESTYPES = {"int": ctypes.c_int, "void": None, "const char*": ctypes.c_char_p}


def _param_type(param, structs, decl):
    """a scalar by its fixed-width type, lsim_handle as void*, a pointer to a header struct as POINTER(mirror), any other pointer or array as void*"""
    m = re.match(r"(\w+)\s*((?:\*\s*)*)(\w+)?\s*((?:\[[^\]]*\])*)$", re.sub(r"\bconst\b", "", param).strip())
    if m:
        base, stars, dims = m.group(1), m.group(2).count("*"), m.group(4)
        if not stars and not dims and base in _SCALARS:
            return _SCALARS[base]
        if stars == 1 and not dims and base in structs:      # byref(struct) and arrays of the struct
            return ctypes.POINTER(structs[base])
        if (stars or dims) and (base == "void" or base in _SCALARS):
            return ctypes.c_void_p
    raise ValueError(f"include/lsim.h: cannot bind parameter '{param.strip()}' of '{decl}'")


def parse_prototypes(text, structs):
    """{name: (restype, argtypes)} of every function `text` declares; a declaration the rules above cannot type raises, naming it"""
    text = re.sub(r"^\s*#.*$", "", _strip_comments(text), flags=re.M)
    protos = {}
    for m in re.finditer(r"([\w \t*]+?)\b(lsim_\w+)\s*\(([^()]*)\)\s*;", text):
        decl = " ".join(m.group(0).split())
        ret = re.sub(r"\s*\*", "*", " ".join(m.group(1).split()))
        if ret not in _RESTYPES or m.group(2) in protos:
            raise ValueError(f"include/lsim.h: cannot bind '{decl}' (return type or a second declaration)")
        params = [] if m.group(3).strip() in ("", "void") else m.group(3).split(",")
        protos[m.group(2)] = (_RESTYPES[ret], [_param_type(p, structs, decl) for p in params])
    skipped = set(re.findall(r"\b(lsim_\w+)\s*\(", text)) - set(protos)
    if skipped:
        raise ValueError(f"include/lsim.h: declarations not understood: {sorted(skipped)}")
    return protos


with open(HEADER_PATH) as _f:
    PROTOTYPES = parse_prototypes(_f.read(), STRUCTS)


def declared_functions():
    """Names of every function the header declares."""
    return sorted(PROTOTYPES)


def bind(L, prefix="lsim", names=None):
    """set restype / argtypes of `prefix`_<name> on the library `L` from the header, for every declared function or for `names` (header
    names, lsim_<name>); raises, listing them, if `L` lacks any of those symbols"""
    names = sorted(PROTOTYPES) if names is None else list(names)
    symbol = {n: prefix + n[len("lsim"):] for n in names}
    missing = [s for s in symbol.values() if not hasattr(L, s)]
    if missing:
        raise RuntimeError(f"{getattr(L, '_name', L)} does not export {missing}")
    for n, s in symbol.items():
        fn = getattr(L, s)
        fn.restype, fn.argtypes = PROTOTYPES[n]
    return L


def check_abi(lib, prefix="lsim", structs=None):
    """Raise if the loaded library was built against a different struct layout."""
    structs = structs or STRUCTS
    for what, struct in (("config", structs["lsim_config"]), ("model", structs["lsim_robot_model"])):
        got = getattr(lib, f"{prefix}_sizeof_{what}")()
        if got != ctypes.sizeof(struct):
            raise RuntimeError(f"ABI mismatch: {prefix}_sizeof_{what}() = {got}, python mirror = {ctypes.sizeof(struct)}; rebuild the library")
