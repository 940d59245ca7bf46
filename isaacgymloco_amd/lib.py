"""ctypes binding of liblsim.so (include/lsim.h).  There is NO fallback: if the HIP library is missing, was built against
another header or lacks a function the header declares, loading it fails loudly.  No prototype is written here: abi.bind types
every entry point from the header's own declarations."""
import ctypes
import os

from . import abi

# LSIM_LIB selects another build of the same HIP library (A/B experiments on kernel variants); never a fallback
LIB_PATH = os.environ.get("LSIM_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "liblsim.so")
_lib = None


class LsimError(RuntimeError):
    pass


def load():
    global _lib
    if _lib is None:
        _lib = load_path(LIB_PATH)
    return _lib


def load_path(path):
    """a build of the HIP library at `path`, prototypes set from the header (load() = the product build, cached; tests load diagnostics variants beside it)"""
    if not os.path.exists(path):
        raise LsimError(f"{path} not found: build the HIP extension first (python -m isaacgymloco_amd.csrc.build); "
                        "there is no CPU fallback for the simulator")
    L = ctypes.CDLL(path)
    abi.check_abi(L, prefix="lsim")
    if L.lsim_abi_version() != abi.ABI_VERSION:
        raise LsimError("liblsim.so ABI version mismatch; rebuild")
    try:
        return abi.bind(L)
    except RuntimeError as e:       # a library that lacks an entry point the header declares: an older build; rebuild
        raise LsimError(str(e)) from None


# ---- roctx ranges (SURVEY.md 8d "roctx ranges per K1-K4"): LSIM_ROCTX=1 brackets the simulator step, the policy / storage kernels of the
# rollout and the learner update with named ranges that `rocprofv3 --marker-trace` shows on the timeline.  Off by default: a push / pop
# pair is two library calls per range on the host-bound rollout loop.
_roctx = None


def _roctx_lib():
    global _roctx
    if _roctx is None:
        _roctx = False
        if os.environ.get("LSIM_ROCTX") == "1":
            for name in ("librocprofiler-sdk-roctx.so", "libroctx64.so"):
                try:
                    R = ctypes.CDLL(name)
                    R.roctxRangePushA.argtypes = [ctypes.c_char_p]
                    _roctx = R
                    break
                except OSError:
                    continue
    return _roctx


class roctx_range:
    """with roctx_range("lsim_step"): ...   (no-op unless LSIM_ROCTX=1 and a roctx library is present)"""
    __slots__ = ("name", "on")

    def __init__(self, name):
        self.name = name.encode()
        self.on = False

    def __enter__(self):
        R = _roctx_lib()
        if R:
            R.roctxRangePushA(self.name)
            self.on = True
        return self

    def __exit__(self, *exc):
        if self.on:
            _roctx.roctxRangePop()
        return False


def entry(api, name, what):
    """`api`'s entry point `name`; a library (or a CPU shim of the tests) without it raises: nothing falls back to torch for `what`"""
    if not hasattr(api, name):
        raise LsimError(f"the loaded library has no {name}: rebuild it (there is no torch fall-back for {what})")
    return getattr(api, name)


def check(rc, handle=None, what="lsim call"):
    if rc != 0:
        msg = ""
        if handle is not None and _lib is not None:
            m = _lib.lsim_last_error(handle)
            msg = m.decode() if m else ""
        raise LsimError(f"{what} failed with code {rc} {msg}")
