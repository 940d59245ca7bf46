"""tests/launch_rig.py itself: the array holder's round trips and guards on the host and on a device, and the launch on a dummy struct."""
import ctypes

import numpy as np
import pytest

from launch_rig import GUARD_WORDS, NAN_GUARD, Arrays, LaunchRig

# logical shapes whose byte sizes (60, 24, 7, 20) are no multiples of 16
CASES = [("f", np.float32, (3, 5), -123.5), ("i", np.int64, (3,), 0x5A5A5A5A5A5A), ("b", np.uint8, (7,), True), ("u", np.uint32, (5,), 0xA5A5A5A5)]


def _values(dt, shape):
    n = int(np.prod(shape))
    return (np.arange(n).reshape(shape) * 3 + 1).astype(dt) if dt != np.uint32 else (np.arange(n, dtype=np.uint32).reshape(shape) + np.uint32(0xFFFFFFF0))


def _round_trips(device):
    h = Arrays(device)
    for name, dt, shape, guard in CASES:
        h.add(name, np.zeros(shape, dt), guard=guard)
    h.add("input", np.arange(6, dtype=np.float32).reshape(2, 3))
    for name, dt, shape, guard in CASES:
        assert h.ptr(name) % 16 == 0 and h.ptr(name) != 0
        got = h.get(name)
        assert got.shape == shape and got.dtype == dt and not got.any()
        want = _values(dt, shape)
        h.put(name, want)
        np.testing.assert_array_equal(h.get(name), want)
        raw = h.raw(name)
        assert raw.dtype == dt and raw.shape == (want.size + GUARD_WORDS,)
        np.testing.assert_array_equal(raw[:want.size], want.reshape(-1))
        if guard is not True:
            assert (raw[want.size:] == np.array(guard).astype(dt)).all()
        h.put(name, 5)                                       # a broadcast scalar fills the logical extent and nothing else
        assert (h.get(name) == 5).all() and h.guards_intact()
    assert (h.raw("b")[7:].tobytes() == np.full(4, NAN_GUARD, np.uint32).tobytes()) and h.raw("input").shape == (6,)
    np.testing.assert_array_equal(h.get("input"), np.arange(6, dtype=np.float32).reshape(2, 3))
    h.assert_guards()
    return h


def test_put_and_get_round_trip_on_the_host_and_leave_the_guards():
    h = _round_trips(None)
    assert h.stream() is None and h.stream(object()) is None
    assert all(isinstance(a, np.ndarray) and a.ctypes.data % 64 == 0 for a in h.a.values())


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_one_element_past_the_logical_end_is_detected_and_named(name):
    h = _round_trips(None)
    n = h.get(name).size
    raw = h.raw(name)
    assert raw[n] != 0
    raw[n] = 0                                               # raw() is a copy: the holder is unchanged
    h.assert_guards()
    h.a[name][n] = 0                                         # the array itself
    assert not h.guards_intact()
    with pytest.raises(AssertionError, match=f"guard of {name} overwritten"):
        h.assert_guards()


class _Two(ctypes.Structure):
    _fields_ = [("tick", ctypes.c_int), ("flags", ctypes.c_uint32)]


class _Pointers(ctypes.Structure):
    _fields_ = [("x", ctypes.c_void_p), ("y", ctypes.c_void_p), ("n", ctypes.c_int)]


def test_launch_copies_the_struct_sets_tick_and_flags_and_applies_the_edit():
    seen = []

    def entry(ref, stream):
        s = ref._obj
        seen.append((s.tick, s.flags, stream))
        return 7 + len(seen)

    rig = LaunchRig()
    stored = rig.bind(_Two(tick=11, flags=2), entry)
    assert rig.launch(5, 1) == 8 and rig.launch() == 9
    assert rig.launch(5, 1, edit=lambda s: setattr(s, "flags", s.flags | 4)) == 10
    assert rig.launch(6, entry=lambda ref, stream: ref._obj.tick * 100) == 600
    assert seen == [(5, 1, None), (11, 2, None), (5, 5, None)]
    assert (stored.tick, stored.flags) == (11, 2) and rig.struct is stored


def test_launch_on_a_struct_without_tick_and_point():
    rig = LaunchRig()
    rig.add("x", np.zeros(3, np.float32), guard=True)
    p = _Pointers(y=1234, n=3)
    rig.point(p, ("x", "y"))
    assert (p.x, p.y, p.n) == (rig.ptr("x"), None, 3)
    rig.bind(p, lambda ref, stream: ref._obj.n)
    assert rig.launch(9, 9) == 3 and rig.launch(edit=lambda s: setattr(s, "n", 4)) == 4 and p.n == 3


@pytest.mark.gpu
def test_round_trip_guards_and_the_stream_on_the_device():
    import torch
    h = _round_trips("cuda:0")
    assert all(isinstance(a, torch.Tensor) and a.device.type == "cuda" for a in h.a.values())
    assert (h.stream().value or 0) == torch.cuda.current_stream().cuda_stream          # (the NULL stream's value reads back as None)
    side = torch.cuda.Stream()
    assert h.stream(side).value == h.stream(side.cuda_stream).value == side.cuda_stream
    with torch.cuda.stream(side):
        assert h.stream().value == side.cuda_stream
    for name, dt, shape, _ in CASES:
        n = int(np.prod(shape))
        assert h.a[name].numel() == n + GUARD_WORDS
        h.a[name][n] = 0                                     # inside the tensor's own allocation: its first guard element
        with pytest.raises(AssertionError, match=f"guard of {name} overwritten"):
            h.assert_guards()
        h.a[name][n] = h.a[name][n + 4]                      # the pattern repeats every four bytes: mended
        h.assert_guards()
