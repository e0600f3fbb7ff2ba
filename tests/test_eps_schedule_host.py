"""CPU: the exploration schedule's host side (gnn_hex_amd.multi_env_manager.EpsSchedule, include/hexgnn.h: hexgnn_rollout_ply,
hexgnn_frames_add).  ``EpsSchedule.value`` is the formula the header fixes, evaluated in float64 with one rounding per operation and
one final rounding to float32 -- the test writes the same evaluation out in numpy float64 scalars and compares bits.  The call
descriptor agrees with its ctypes mirror field for field and the entry points refuse a missing handle or counter before anything
is launched.  Nothing here touches a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def _f64(init, final, decay, burnin, frame):
    """The header's formula in numpy float64 scalars (IEEE double, every operation rounded on its own), then float32."""
    init, final = np.float64(init), np.float64(final)
    if frame < burnin:
        return np.float32(init)
    p = np.float64(1.0)
    if decay > 0:
        p = np.minimum(np.float64(1.0), np.float64(frame - burnin) / np.float64(decay))
    return np.float32(init + (final - init) * p)


def _bits(v):
    assert isinstance(v, np.float32), type(v)
    return v.tobytes()


def test_value_at_the_corners_of_the_schedule():
    from gnn_hex_amd.multi_env_manager import EpsSchedule
    s = EpsSchedule(0.12, 0.05, 100000, burnin=2000)
    assert _bits(s.value(0)) == _bits(s.value(1999)) == np.float32(0.12).tobytes()          # burnin - 1: still init
    assert _bits(s.value(2000)) == np.float32(0.12).tobytes()                              # burnin: p = 0
    mid = s.value(52000)
    assert _bits(mid) == _bits(_f64(0.12, 0.05, 100000, 2000, 52000))
    assert abs(float(mid) - 0.085) < 1e-7                                                  # half way, to float32 precision
    end = s.value(102000)
    assert _bits(end) == _bits(_f64(0.12, 0.05, 100000, 2000, 102000))
    assert abs(float(end) - 0.05) < 1e-7
    for beyond in (102001, 10 ** 7, 2 ** 40):
        assert _bits(s.value(beyond)) == _bits(end)                                        # p is clamped at 1
    # exactly representable ends come out exactly
    t = EpsSchedule(1.0, 0.0, 50, burnin=10)
    assert float(t.value(9)) == 1.0 and float(t.value(10)) == 1.0 and float(t.value(35)) == 0.5
    assert float(t.value(60)) == 0.0 and float(t.value(61)) == 0.0


def test_zero_decay_is_a_step_at_burnin():
    from gnn_hex_amd.multi_env_manager import EpsSchedule
    s = EpsSchedule(0.5, 0.25, 0, burnin=7)
    assert float(s.value(6)) == 0.5 and float(s.value(7)) == 0.25 and float(s.value(10 ** 6)) == 0.25
    assert float(EpsSchedule(0.5, 0.25, 0).value(0)) == 0.25


def test_an_increasing_schedule():
    from gnn_hex_amd.multi_env_manager import EpsSchedule
    s = EpsSchedule(0.0, 0.5, 64, burnin=0)
    assert float(s.value(0)) == 0.0 and float(s.value(16)) == 0.125 and float(s.value(64)) == 0.5 == float(s.value(65))
    vals = [float(s.value(f)) for f in range(0, 80)]
    assert all(a <= b for a, b in zip(vals, vals[1:]))


@pytest.mark.parametrize("init,final,decay,burnin", [(0.12, 0.05, 100000, 0), (0.12, 0.05, 100000, 2000), (1.0, 0.0, 50, 10),
                                                       (0.05, 0.9, 12345, 77), (0.3, 0.3, 1000, 0), (0.7, 0.1, 3, 1)])
def test_float32_result_equals_the_float64_evaluation_and_is_monotone(init, final, decay, burnin):
    from gnn_hex_amd.multi_env_manager import EpsSchedule
    s = EpsSchedule(init, final, decay, burnin=burnin)
    rng = np.random.default_rng(decay + burnin)
    frames = np.sort(np.concatenate([rng.integers(0, burnin + 2 * decay + 10, 990), [0, burnin, burnin + decay, burnin + decay + 1],
                                     rng.integers(0, 2 ** 50, 6)]))
    assert len(frames) == 1000
    vals = []
    for f in frames.tolist():
        v = s.value(f)
        assert _bits(v) == _bits(_f64(init, final, decay, burnin, f)), f
        vals.append(float(v))
    step = np.diff(np.array(vals))
    assert (step <= 0).all() if final <= init else (step >= 0).all()
    lo, hi = min(np.float32(init), np.float32(final)), max(np.float32(init), np.float32(final))
    assert lo <= min(vals) and max(vals) <= hi


def test_update_and_validation():
    from gnn_hex_amd.multi_env_manager import EpsSchedule
    s = EpsSchedule(0.12, 0.05, 100000)
    s.update(final=0.01, decay_frames=10)
    assert (s.init, s.final, s.decay_frames, s.burnin) == (0.12, 0.01, 10, 0)
    assert _bits(s.value(10)) == _bits(_f64(0.12, 0.01, 10, 0, 10))
    for bad in ((1.5, 0.0, 1, 0), (0.1, -0.2, 1, 0), (0.1, 0.1, -1, 0), (0.1, 0.1, 1, -1), (0.1, 0.1, 1.5, 0), (float("nan"), 0.1, 1, 0)):
        with pytest.raises(ValueError):
            EpsSchedule(*bad)


def test_entry_points_are_declared_exported_and_mirrored():
    from gnn_hex_amd import _lib
    header = open(os.path.join(ROOT, "include", "hexgnn.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"\bint\s+hexgnn_rollout_ply\s*\(\s*hexgnn_env\s*\*\s*\w+\s*,\s*const\s+hexgnn_rollout_call\s*\*", header)
    assert re.search(r"\bint\s+hexgnn_frames_add\s*\(\s*int64_t\s*\*", header)
    for name in ("hexgnn_rollout_ply", "hexgnn_frames_add"):
        assert hasattr(raw, name) and name in _lib.exported_symbols()
    assert "PARITY UNPINNED" in header[header.index("self-play ply with the exploration schedule"):header.index("hexgnn_rollout_call {")]
    m = re.search(r"typedef\s+struct\s+hexgnn_rollout_call\s*\{(.*?)\}\s*hexgnn_rollout_call\s*;", header, re.S)
    kinds = {"size_t": ctypes.c_size_t, "int": ctypes.c_int, "int64_t": ctypes.c_int64}
    want = []
    for decl in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        head = re.match(r"(?:const\s+)?(\w+)", decl)
        for item in decl[head.end():].split(","):
            name = re.search(r"(\w+)\s*$", item).group(1)
            want.append((name, ctypes.c_void_p if "*" in item else kinds[head.group(1)]))
    assert [(n, t) for n, t in _lib.RolloutCall._fields_] == want
    assert want[0] == ("struct_bytes", ctypes.c_size_t) and ("sched", ctypes.c_void_p) in want and ("frames", ctypes.c_void_p) in want


def test_refusals_that_need_no_device():
    from gnn_hex_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    call = _lib.RolloutCall(struct_bytes=ctypes.sizeof(_lib.RolloutCall), frame_add=0, reset_maker_turn=0)
    for name, kind in _lib.RolloutCall._fields_:
        if kind is ctypes.c_void_p:
            setattr(call, name, p)
    assert L.hexgnn_rollout_ply(None, ctypes.byref(call), None) == EINVAL        # no env handle
    assert L.hexgnn_rollout_ply(p, None, None) == EINVAL                         # no descriptor
    call.struct_bytes = 8
    assert L.hexgnn_rollout_ply(p, ctypes.byref(call), None) == EINVAL           # another ABI's descriptor: checked before the handle is read
    assert L.hexgnn_frames_add(None, 5, None) == EINVAL
