"""CPU checks of the C-ABI: the HIP library loads and exports every symbol include/lsim.h declares (no compute
calls here: there is no GPU), struct mirrors agree, argument validation works on the host side."""
import ctypes
import os

import pytest

from helpers import ROOT, abi


def test_header_parses_and_mirrors():
    assert ctypes.sizeof(abi.LsimConfig) > 1000
    assert abi.NUM_REWARD_TERMS == 51
    assert abi.REWARD_NAMES == sorted(abi.REWARD_NAMES), "reward ids must be in the reference's alphabetical order"
    assert abi.BUFFER_IDS["obs"] == 0


def test_library_exports_every_declared_symbol():
    from isaacgymloco_amd.csrc import build
    path = build.build()
    L = ctypes.CDLL(path)
    for fn in abi.declared_functions():
        assert hasattr(L, fn), f"liblsim.so does not export {fn}"
    abi.check_abi(L, "lsim")
    abi.bind(L, names=("lsim_reward_name", "lsim_buffer_name"))
    assert [L.lsim_reward_name(i).decode() for i in range(abi.NUM_REWARD_TERMS)] == abi.REWARD_NAMES
    names = sorted(abi.BUFFER_IDS, key=abi.BUFFER_IDS.get)
    assert [L.lsim_buffer_name(i).decode() for i in range(abi.NUM_BUFFERS)] == names


def test_every_declared_function_has_a_prototype_of_the_headers_arity():
    import re
    text = re.sub(r"^\s*#.*$", "", abi._strip_comments(open(abi.HEADER_PATH).read()), flags=re.M)
    assert len(abi.declared_functions()) >= 72 and set(abi.declared_functions()) == set(abi.PROTOTYPES)
    for name in abi.declared_functions():
        params, = re.findall(r"\b%s\s*\(([^()]*)\)\s*;" % name, text)
        want = 0 if params.strip() in ("", "void") else params.count(",") + 1
        assert len(abi.PROTOTYPES[name][1]) == want, name


def test_prototypes_follow_the_mapping_rules():
    """one literal signature per rule: scalars by width, lsim_handle and plain pointers as void*, struct pointers typed, the three return types"""
    c = ctypes
    vp, i64, P = c.c_void_p, c.c_int64, abi.PROTOTYPES
    assert P["lsim_step_ex"] == (c.c_int, [vp, vp, c.c_uint32, vp])
    assert P["lsim_amp_pair_rows"] == (c.c_int, [vp, i64, vp, i64, vp, vp, c.c_double, c.c_double, i64, c.c_int, vp, i64, vp])
    assert P["lsim_linear_wgrad_workspace"] == (c.c_int, [c.c_long, c.c_int, c.c_int, vp, vp])
    assert P["lsim_raycast_bodies"] == (c.c_int, [c.POINTER(abi.LsimRaycastBodies), vp])
    assert P["lsim_create_mixed"] == (c.c_int, [c.POINTER(abi.LsimConfig), c.POINTER(abi.LsimRobotModel), c.c_int32, vp, vp, vp, vp, c.c_int, vp])
    assert P["lsim_get_buffer"] == (c.c_int, [vp, c.c_int, vp, vp, vp, vp])                       # void**, int64_t [4]
    assert P["lsim_adam_clip_step"][1][:4] == [c.c_int, vp, vp, vp] and P["lsim_adam_clip_step"][1][-2] is c.c_size_t      # float* const*
    assert P["lsim_rollout_gae"][1][2:4] == [c.c_float, c.c_float]
    assert P["lsim_destroy"] == (None, [vp])
    assert P["lsim_last_error"] == (c.c_char_p, [vp])
    assert P["lsim_reward_name"] == (c.c_char_p, [c.c_int])
    assert P["lsim_sizeof_config"] == (c.c_int, [])


def test_loaded_library_has_every_prototype_set():
    from isaacgymloco_amd import lib
    L = lib.load()
    for name in abi.declared_functions():
        fn = getattr(L, name)
        assert fn.argtypes is not None and (fn.restype, list(fn.argtypes)) == abi.PROTOTYPES[name], name


def test_bind_names_the_missing_symbols():
    class Partial:
        def lsim_step(self):
            pass
    with pytest.raises(RuntimeError, match=r"lsim_destroy.*lsim_raycast_bodies|lsim_raycast_bodies.*lsim_destroy"):
        abi.bind(Partial(), names=("lsim_step", "lsim_raycast_bodies", "lsim_destroy"))
    with pytest.raises(RuntimeError, match="emu_raycast"):
        abi.bind(Partial(), prefix="emu", names=("lsim_raycast",))


def test_library_without_a_declared_symbol_is_refused_at_load(tmp_path):
    import subprocess
    from isaacgymloco_amd import lib
    src, out = os.path.join(tmp_path, "old.c"), os.path.join(tmp_path, "libold.so")
    with open(src, "w") as f:
        f.write("int lsim_sizeof_config(void) { return %d; }\nint lsim_sizeof_model(void) { return %d; }\nint lsim_abi_version(void) { return %d; }\n"
                % (ctypes.sizeof(abi.LsimConfig), ctypes.sizeof(abi.LsimRobotModel), abi.ABI_VERSION))
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-o", out, src])
    with pytest.raises(lib.LsimError, match="lsim_raycast_bodies"):
        lib.load_path(out)


@pytest.mark.parametrize("decl", ["int lsim_new(unsigned int flags);", "int lsim_new(lsim_config cfg);", "int lsim_new(struct foo* p);",
                                  "float lsim_new(int a);", "int lsim_new(int (*callback)(int));"])
def test_unknown_type_spelling_in_a_declaration_raises(decl):
    assert abi.parse_prototypes("int lsim_ok(const lsim_config* cfg, size_t* n);", abi.STRUCTS) == \
        {"lsim_ok": (ctypes.c_int, [ctypes.POINTER(abi.LsimConfig), ctypes.c_void_p])}
    with pytest.raises(ValueError, match="lsim_new"):
        abi.parse_prototypes("int lsim_ok(void);\n" + decl, abi.STRUCTS)


def test_integration_document_names_every_entry_point():
    """INTEGRATION.md's table maps the reference's calls to the C-ABI: an entry point added to include/lsim.h without a row there is undocumented"""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    missing = [fn for fn in abi.declared_functions() if fn not in doc]
    assert not missing, missing


def test_environment_variables_are_documented():
    """every LSIM_* variable the package or the library reads (os.environ.get / getenv) has an entry in INTEGRATION.md: the set of overrides stays closed"""
    import re
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    names = set()
    for d, _, files in os.walk(os.path.join(ROOT, "isaacgymloco_amd")):
        for f in files:
            if f.endswith((".py", ".h", ".hip")):
                names.update(re.findall(r'(?:os\.environ\.get|getenv)\(\s*"(LSIM_[A-Z0-9_]+)"', open(os.path.join(d, f)).read()))
    assert len(names) >= 15, sorted(names)       # the scan itself works
    missing = sorted(n for n in names if not re.search(r"`" + n + r"`", doc))
    assert not missing, missing


def test_query_arena_validates_config():
    from isaacgymloco_amd.csrc import build
    L = ctypes.CDLL(build.build())
    cfg = abi.LsimConfig()
    n = ctypes.c_size_t()
    assert L.lsim_query_arena(ctypes.byref(cfg), ctypes.byref(n)) == abi.DEFINES["LSIM_E_ABI"] - (1 << 32) or \
        L.lsim_query_arena(ctypes.byref(cfg), ctypes.byref(n)) == -5
    from helpers import C, T, LC, aliengo
    c = C.aliengo_cfg()
    c.terrain.terrain_proportions = [1.0, 0, 0, 0]
    ter = T.Terrain(c.terrain, 64)
    lc = LC.make_lsim_config(c, num_envs=64, terrain=ter)
    assert L.lsim_query_arena(ctypes.byref(lc), ctypes.byref(n)) == 0
    assert n.value > 64 * (270 + 238) * 4


def test_env_refuses_to_run_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from isaacgymloco_amd import lib
    from isaacgymloco_amd.envs.legged_robot import LeggedRobot
    from helpers import C
    with pytest.raises(lib.LsimError):
        LeggedRobot(C.aliengo_cfg(), sim_device="cuda:0")


def test_learner_workspace_queries_validate_shapes():
    """the host-side planners of the learner entry points (no launches): sizes grow with the batch, unsupported shapes are refused"""
    from isaacgymloco_amd import lib
    L = lib.load()             # loading needs no GPU; only the launches do
    n, parts = ctypes.c_size_t(), ctypes.c_int()
    B = 102400
    # weight gradient: every layer of the three networks has a plan; a 1024 x 1024 layer (discriminator-sized) is left to BLAS
    for k_in, n_out in ((270, 128), (128, 64), (64, 19), (64, 512), (512, 256), (256, 128), (128, 12), (238, 512), (128, 1), (45, 128), (64, 16)):
        assert L.lsim_linear_wgrad_workspace(B, k_in, n_out, ctypes.byref(n), ctypes.byref(parts)) == 0, (k_in, n_out)
        assert parts.value >= 1 and n.value >= parts.value * (k_in * n_out + n_out) * 4
    assert L.lsim_linear_wgrad_workspace(B, 1024, 1024, ctypes.byref(n), ctypes.byref(parts)) == abi.E_UNSUPPORTED
    assert L.lsim_linear_wgrad_workspace(0, 64, 64, ctypes.byref(n), ctypes.byref(parts)) == abi.E_UNSUPPORTED
    # Sinkhorn / estimator loss head: K <= 64 prototypes, latent <= 32
    assert L.lsim_sinkhorn_workspace(B, 32, ctypes.byref(n)) == 0 and n.value >= B * 32 * 4
    assert L.lsim_sinkhorn_workspace(B, 65, ctypes.byref(n)) == abi.E_INVALID
    small = ctypes.c_size_t()
    assert L.lsim_estimator_loss_workspace(4096, 16, 32, ctypes.byref(small)) == 0
    assert L.lsim_estimator_loss_workspace(B, 16, 32, ctypes.byref(n)) == 0 and n.value > small.value
    assert n.value >= (2 * B * 16 + 2 * B * 32) * 4          # z and the scores of both matrices at least (E = exp(S / eps) is formed again where it is used)
    assert L.lsim_estimator_loss_workspace(B, 33, 32, ctypes.byref(n)) == abi.E_INVALID
    assert L.lsim_estimator_loss_workspace(B, 16, 65, ctypes.byref(n)) == abi.E_INVALID
    assert L.lsim_estimator_loss_workspace(B, 16, 32, None) == abi.E_INVALID
    assert L.lsim_ppo_loss_workspace(B, ctypes.byref(n)) == 0 and n.value > 0
