"""CPU: the entry points of the multi-set forward (hexgnn_qnet_forward_jobs / _multi, hexgnn_dqn_targets) refuse bad arguments
before anything touches the device, and their byte queries are pure, monotone host arithmetic.  Nothing here launches anything:
every pointer handed over is host memory that a correct argument check never dereferences on the device."""
import ctypes

import pytest

EINVAL, EUNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def L():
    from gnn_hex_amd import _lib
    return _lib.lib()


def _buf(n=4096):
    b = (ctypes.c_char * n)()
    return b, ctypes.addressof(b)


def test_byte_queries_are_monotone(L):
    assert L.hexgnn_qnet_jobs_bytes(256, 2) == 4 * 256 * 2 and L.hexgnn_qnet_jobs_bytes(0, 1) == 0
    for k in (0, 5, -1):
        assert L.hexgnn_qnet_jobs_bytes(8, k) == 0 and L.hexgnn_qnet_multi_workspace_bytes(100, 8, 2, 35, 5, k) == 0
    assert L.hexgnn_qnet_jobs_bytes(-1, 2) == 0
    assert L.hexgnn_qnet_multi_workspace_bytes(-1, 8, 2, 35, 5, 2) == 0 and L.hexgnn_qnet_multi_workspace_bytes(100, -1, 2, 35, 5, 2) == 0
    for hidden in (128, 113, 1, 2000):          # hexgnn_qnet_supported == 0
        assert L.hexgnn_qnet_supported(2, hidden, 0) == 0
        assert L.hexgnn_qnet_multi_workspace_bytes(100, 8, 2, hidden, 5, 2) == 0
    pack = L.hexgnn_sage_stack_pack_bytes(2, 35, 5)
    for k in (1, 2, 3, 4):
        w = L.hexgnn_qnet_multi_workspace_bytes(100, 8, 2, 35, 5, k)
        assert w >= k * pack + 4 * 8 * k and w % 256 == 0
    last = 0
    for k in (1, 2, 3, 4):
        prev_b = 0
        for b in (0, 1, 7, 64, 65, 256, 768, 5000):
            prev_n = 0
            for n in (0, 1, 100, 10 ** 4, 10 ** 6):
                w = L.hexgnn_qnet_multi_workspace_bytes(n, b, 2, 110, 17, k)
                assert w > 0 and w >= prev_n and w >= prev_b and w >= last
                prev_n = w
            prev_b = L.hexgnn_qnet_multi_workspace_bytes(0, b, 2, 110, 17, k)
            assert L.hexgnn_qnet_jobs_bytes(b, k) == 4 * b * k
        last = L.hexgnn_qnet_multi_workspace_bytes(0, 0, 2, 110, 17, k)


def test_forward_jobs_rejects_bad_arguments(L):
    _, p = _buf()
    one = (ctypes.c_void_p * 8)(*([p] * 8))          # a "layer array": 8 non-null pointers
    sets = (ctypes.c_void_p * 4)(*([ctypes.addressof(one)] * 4))
    call = lambda b, k, gptr, jobs, hidden=35, wl=sets, bl=sets, wr=sets, wpack=one: L.hexgnn_qnet_forward_jobs(   # noqa: E731
        b, k, gptr, jobs, 2, hidden, 5, wl, bl, wr, wpack, None)
    for k in (0, 5, -3):
        assert call(4, k, p, p) == EINVAL
    assert call(4, 2, p, None) == EINVAL                 # null job table
    assert call(-1, 2, p, p) == EINVAL                   # negative b
    assert call(4, 2, None, p) == EINVAL
    for hidden in (128, 113, 1):
        assert call(4, 2, p, p, hidden=hidden) == EUNSUPPORTED
    assert call(4, 2, p, p, wl=None) == EINVAL and call(4, 2, p, p, wpack=None) == EINVAL     # packs: all four or none
    nulls = (ctypes.c_void_p * 4)()
    assert call(4, 2, p, p, wr=nulls) == EINVAL
    hole = (ctypes.c_void_p * 8)(*([p] * 3 + [None] + [p] * 4))
    assert call(4, 2, p, p, bl=(ctypes.c_void_p * 4)(*([ctypes.addressof(hole)] * 4))) == EINVAL


def test_forward_multi_rejects_bad_arguments(L):
    _, p = _buf()
    _, p2 = _buf()
    six = (ctypes.c_void_p * 6)(*([p] * 6))
    tails = (ctypes.c_void_p * 4)(*([ctypes.addressof(six)] * 4))
    same = (ctypes.c_void_p * 4)(*([p] * 4))
    qs = (ctypes.c_void_p * 4)(p, p2, p + 1024, p2 + 1024)

    def call(n=100, b=4, k=2, hidden=35, gptr=p, x=p, x_stride=2, jobs=p, wpack=same, tail=tails, q=qs, status=same):
        return L.hexgnn_qnet_forward_multi(n, b, k, 2, hidden, 5, gptr, p, p, p, x, x_stride, jobs, wpack, tail, q, status, None)
    for k in (0, 5):
        assert call(k=k) == EINVAL
    assert call(jobs=None) == EINVAL                     # null job table
    assert call(b=-1) == EINVAL and call(n=-1) == EINVAL
    for hidden in (128, 113, 1):
        assert call(hidden=hidden) == EUNSUPPORTED
    assert call(gptr=None) == EINVAL and call(x=None) == EINVAL and call(x_stride=1) == EINVAL
    assert call(wpack=None) == EINVAL and call(tail=None) == EINVAL and call(q=None) == EINVAL and call(status=None) == EINVAL
    assert call(q=same) == EINVAL                        # two sets must not share an output
    short = (ctypes.c_void_p * 6)(p, p, p, None, p, p)
    assert call(tail=(ctypes.c_void_p * 4)(*([ctypes.addressof(short)] * 4))) == EINVAL
    assert call(n=0, b=0) == 0                           # an empty batch is fine, and launches nothing


def test_dqn_targets_rejects_bad_arguments(L):
    _, p = _buf()
    good = [p, p, p, p, p]
    assert L.hexgnn_dqn_targets(-1, *good, 0.97, p, p, None) == EINVAL
    for hole in range(5):
        args = list(good)
        args[hole] = None
        assert L.hexgnn_dqn_targets(3, *args, 0.97, p, p, None) == EINVAL
    assert L.hexgnn_dqn_targets(3, *good, 0.97, None, p, None) == EINVAL
    assert L.hexgnn_dqn_targets(3, *good, 0.97, p, None, None) == EINVAL
    assert L.hexgnn_dqn_targets(0, None, None, None, None, None, 0.97, None, None, None) == 0


def test_python_surface_checks_its_arguments_on_the_host():
    import torch
    from gnn_hex_amd import ops
    from gnn_hex_amd._lib import HexGnnError
    assert ops.MAX_SETS == 4
    x = torch.zeros(4, 3)
    ei = torch.zeros((2, 0), dtype=torch.long)
    with pytest.raises(ValueError):
        ops.multi_forward([], x, ei)
    with pytest.raises(ValueError):
        ops.multi_forward([None] * 5, x, ei)
    with pytest.raises(HexGnnError):
        ops.multi_forward([None], x, ei)                 # CPU tensors: no fallback
    with pytest.raises(HexGnnError):
        ops.double_dqn_targets(None, None, x, ei, None, None, torch.zeros(1), torch.zeros(1, dtype=torch.bool), 0.9)
    with pytest.raises(HexGnnError):
        ops.forward_jobs(torch.tensor([0, 4]), 2)
