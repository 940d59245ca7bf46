"""TEST INFRASTRUCTURE -- the one holder of a kernel rig's arrays and the one launch.  Arrays keeps named arrays in host memory (numpy, for a
CPU shim) or on a torch device (for the HIP library) and is the only code that tells the two apart; every array a launch may write gets
GUARD_WORDS guard elements behind it, which assert_guards() checks.  LaunchRig adds the launch's ctypes struct and entry point.  A new
kernel's rig derives from LaunchRig: add() its arrays, point() and fill its struct, bind() it, and call assert_guards() in its read().
torch is imported only once a device is asked for."""
import ctypes

import numpy as np

from emu_binding import aligned

GUARD_WORDS = 16                 # elements behind every guarded array
NAN_GUARD = 0x7FC0FEED           # the default pattern (guard=True): a NaN no kernel produces, repeated over the guard's bytes
_SIGNED = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}      # dtypes torch lacks


class Arrays:
    """named flat arrays, on the host (numpy, 64-byte aligned) or on `device` (torch); `a[name]` is the allocation, guard included"""

    def __init__(self, device=None):
        self.device, self.a, self.n, self.guards = device, {}, {}, {}

    def add(self, name, value, guard=None):
        """store `value`; `guard`: None (a read-only input), True (NAN_GUARD) or a value of the array's dtype"""
        v = np.ascontiguousarray(value)
        store = aligned((v.size + (0 if guard is None else GUARD_WORDS),), v.dtype)
        store[:v.size] = v.reshape(-1)
        if guard is not None:
            words = np.full(GUARD_WORDS * v.dtype.itemsize // 4 + 1, NAN_GUARD, np.uint32).view(np.uint8)[:GUARD_WORDS * v.dtype.itemsize]
            self.guards[name] = words.view(v.dtype).copy() if guard is True else np.full(GUARD_WORDS, guard, v.dtype)
            store[v.size:] = self.guards[name]
        self.n[name] = (v.shape, v.dtype)
        if self.device is not None:
            import torch
            store = torch.from_numpy(store.view(_SIGNED.get(v.dtype, v.dtype)).copy()).to(self.device)
        self.a[name] = store

    def ptr(self, name):
        return self.a[name].data_ptr() if self.device is not None else self.a[name].ctypes.data

    def raw(self, name):
        """host copy of the whole allocation, guard included, flat"""
        if self.device is None:
            return self.a[name].copy()
        import torch
        torch.cuda.synchronize()
        return self.a[name].cpu().numpy().view(self.n[name][1])

    def get(self, name):
        """host copy in the logical shape and dtype"""
        shape, _ = self.n[name]
        return self.raw(name)[:int(np.prod(shape))].reshape(shape)

    def put(self, name, value):
        """`value`, broadcast, into the logical extent; the guard is never touched"""
        shape, dt = self.n[name]
        v = np.broadcast_to(np.asarray(value, dt), shape).reshape(-1)
        if self.device is not None:
            import torch
            self.a[name][:v.size].copy_(torch.from_numpy(v.view(_SIGNED.get(dt, dt)).copy()).to(self.device))
        else:
            self.a[name][:v.size] = v

    def _bytes(self, v):
        return np.ascontiguousarray(v).view(np.uint8)

    def guards_intact(self):
        return not self._broken()

    def _broken(self):
        return [k for k, g in self.guards.items() if not np.array_equal(self._bytes(self.raw(k)[-GUARD_WORDS:]), self._bytes(g))]

    def assert_guards(self):
        bad = self._broken()
        assert not bad, f"guard of {', '.join(bad)} overwritten"

    def stream(self, stream=None):
        """None on the host; on a device the handle of `stream` (a torch stream or a raw handle), by default the current stream's"""
        if self.device is None:
            return None
        import torch
        s = torch.cuda.current_stream() if stream is None else stream
        return ctypes.c_void_p(getattr(s, "cuda_stream", s))


class LaunchRig(Arrays):
    """Arrays plus one struct and its entry point"""

    def bind(self, struct, entry):
        self.struct, self._entry = struct, entry
        return struct

    def point(self, struct, names):
        """the pointer fields `names` of `struct`: the address of the array of that name, NULL where there is none"""
        for k in names:
            setattr(struct, k, self.ptr(k) if k in self.a else None)

    def launch(self, tick=None, flags=None, edit=None, stream=None, entry=None):
        """one launch; `edit(s)` changes a copy of the struct first; `entry`: another entry point than the bound one; returns its value"""
        s = type(self.struct).from_buffer_copy(self.struct)
        for k, v in (("tick", tick), ("flags", flags)):
            if v is not None and hasattr(s, k):
                setattr(s, k, v)
        if edit:
            edit(s)
        return (entry or self._entry)(ctypes.byref(s), self.stream(stream))


class EditRig(LaunchRig):
    """a LaunchRig whose struct has neither tick nor flags: launch(edit, stream)"""

    def launch(self, edit=None, stream=None):
        return super().launch(edit=edit, stream=stream)


def device_lib():
    from isaacgymloco_amd import lib
    return lib.load()


def current_stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def bits32(a):
    """the fp32 bits of `a` with -0.0 folded into +0.0"""
    return (np.asarray(a, dtype=np.float32) + np.float32(0.0)).view(np.int32)


class NanDevice:
    """NaN-filled device blocks, 16-byte aligned; untouched(): every one still all NaN"""

    def __init__(self, device="cuda:0"):
        self.device, self.keep = device, []

    def address(self, floats):
        import torch
        t = torch.full((floats + 4,), float("nan"), device=self.device)
        assert t.data_ptr() % 16 == 0
        self.keep.append(t)
        return t.data_ptr()

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return all(bool(torch.isnan(t).all()) for t in self.keep)
