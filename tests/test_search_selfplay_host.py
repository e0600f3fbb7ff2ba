"""CPU: the search self-play entry points (include/hexgnn.h: hexgnn_search_root_noise, hexgnn_search_record,
hexgnn_samples_finish, hexgnn_pv_loss) without a device.  (a) the four declarations, the exported symbols and the two ctypes
mirrors field by field, (b) every host refusal in its documented order on fake pointers, (c) the oracle's proportional pick
against a direct numpy restatement, (d) the oracle's loss against the reference expression in torch float64, (e) the python
objects' refusals.  Nothing here touches a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import selfplay_oracle as spo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -2

CALL = r"const\s+hexgnn_search_call\s*\*\s*\w+"
STREAM = r"hexgnn_stream_t\s+\w+"
ENTRY = {
    "hexgnn_search_root_noise": CALL + r"\s*,\s*float\s+\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,\s*" + STREAM,
    "hexgnn_search_record": r"const\s+hexgnn_env\s*\*\s*\w+\s*,\s*" + CALL + r"\s*,\s*const\s+hexgnn_record_call\s*\*\s*\w+\s*,\s*" + STREAM,
    "hexgnn_samples_finish": r"int\s+\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*const\s+int\s*\*\s*\w+\s*,\s*"
                             r"const\s+uint8_t\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*,\s*const\s+int\s*\*\s*\w+\s*,\s*int\s*\*\s*\w+\s*,\s*"
                             + STREAM,
    "hexgnn_pv_loss": r"const\s+hexgnn_pv_loss_call\s*\*\s*\w+\s*,\s*" + STREAM,
}


def _struct_fields(header, name):
    m = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), header, re.S)
    kinds = {"size_t": ctypes.c_size_t, "int": ctypes.c_int, "float": ctypes.c_float}
    want = []
    for decl in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        head = re.match(r"(?:const\s+)?(\w+)", decl)
        for item in decl[head.end():].split(","):
            field = re.search(r"(\w+)\s*$", item).group(1)
            want.append((field, ctypes.c_void_p if "*" in item else kinds[head.group(1)]))
    return want


def test_entry_points_are_declared_exported_and_mirrored():
    from gnn_hex_amd import _lib
    header = open(os.path.join(ROOT, "include", "hexgnn.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, args in ENTRY.items():
        assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)" % (name, args), header), name
        assert hasattr(raw, name) and name in _lib.exported_symbols(), name
    assert _lib.lib().hexgnn_abi_version() == 8
    rec = _struct_fields(header, "hexgnn_record_call")
    assert [(n, t) for n, t in _lib.RecordCall._fields_] == rec
    assert [n for n, _ in rec] == ["struct_bytes", "capacity", "ply", "pick_mode", "head", "recorded", "u", "pick", "policy",
                                   "root_q", "z", "adj", "alive", "side", "sizes", "meta"]
    pv = _struct_fields(header, "hexgnn_pv_loss_call")
    assert [(n, t) for n, t in _lib.PVLossCall._fields_] == pv
    assert [n for n, _ in pv] == ["struct_bytes", "b", "n", "m", "hex_size", "capacity", "q_ratio", "val_factor", "pol_factor",
                                  "logp", "out_ptr", "gptr", "backmap", "value", "policy", "z", "root_q", "index", "loss",
                                  "d_logp", "d_value", "per_graph", "status"]
    # hexgnn_search_call keeps its fields: the new entry points read it as it is
    assert [n for n, _ in _lib.SearchCall._fields_][:4] == ["struct_bytes", "num_games", "hex_size", "max_sims"]


def _search_call(_lib, p, **kw):
    need = _lib.lib().hexgnn_search_workspace_bytes(2, 5, 8)
    call = _lib.SearchCall(struct_bytes=ctypes.sizeof(_lib.SearchCall), num_games=2, hex_size=5, max_sims=8, skip=2, c_puct=1.5,
                           temperature=1.0, fill=0.0, workspace=p, workspace_bytes=need, status=p, active=None, path=p, leaf=p,
                           result=p, logits=p, offsets=p, value=p, gptr=p, scores=p, counts=None, q=None, best=None)
    for k, v in kw.items():
        setattr(call, k, v)
    return call


def _record_call(_lib, p, **kw):
    call = _lib.RecordCall(struct_bytes=ctypes.sizeof(_lib.RecordCall), capacity=50, ply=0, pick_mode=1,
                           **{n: p for n in "head recorded u pick policy root_q z adj alive side sizes meta".split()})
    for k, v in kw.items():
        setattr(call, k, v)
    return call


PV_POINTERS = "logp out_ptr gptr backmap value policy z root_q index loss d_logp d_value per_graph status".split()


def _pv_call(_lib, p, **kw):
    call = _lib.PVLossCall(struct_bytes=ctypes.sizeof(_lib.PVLossCall), b=2, n=30, m=26, hex_size=5, capacity=50, q_ratio=0.0,
                           val_factor=1.0, pol_factor=1.0, **{n: p for n in PV_POINTERS})
    for k, v in kw.items():
        setattr(call, k, v)
    return call


def test_refusals_that_need_no_device():
    """Every refusal comes from the host checks, before anything is launched, in the header's order."""
    from gnn_hex_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    fake = ctypes.c_void_p(p)
    rec = ctypes.byref(_record_call(_lib, p))
    entries = {"root_noise": lambda c: L.hexgnn_search_root_noise(c, 0.25, fake, None),
               "record": lambda c: L.hexgnn_search_record(fake, c, rec, None)}
    for name, fn in entries.items():                       # the checks of hexgnn_search_*, in their order
        assert fn(None) == EINVAL, name
        assert fn(ctypes.byref(_search_call(_lib, p, struct_bytes=ctypes.sizeof(_lib.SearchCall) - 8))) == EINVAL, name
        for kw in (dict(num_games=-1), dict(hex_size=1), dict(max_sims=0), dict(max_sims=65536)):
            assert fn(ctypes.byref(_search_call(_lib, p, **kw))) == EINVAL, (name, kw)
        assert fn(ctypes.byref(_search_call(_lib, p, hex_size=26))) == EUNSUPPORTED, name
        assert fn(ctypes.byref(_search_call(_lib, p, hex_size=26, max_sims=0))) == EINVAL, name
        assert fn(ctypes.byref(_search_call(_lib, None, num_games=0, status=None))) == 0, name
        assert fn(ctypes.byref(_search_call(_lib, p, num_games=0, hex_size=26))) == EUNSUPPORTED, name
        for kw in (dict(workspace=None), dict(status=None), dict(workspace_bytes=_search_call(_lib, p).workspace_bytes - 1)):
            assert fn(ctypes.byref(_search_call(_lib, p, **kw))) == EINVAL, (name, kw)
    c = ctypes.byref(_search_call(_lib, p))
    # root noise: eps, then the noise
    for bad in (-0.01, 1.01, float("nan"), float("inf")):
        assert L.hexgnn_search_root_noise(c, bad, fake, None) == EINVAL, bad
    assert L.hexgnn_search_root_noise(c, 0.25, None, None) == EINVAL
    assert L.hexgnn_search_root_noise(ctypes.byref(_search_call(_lib, None, num_games=0)), 7.0, None, None) == 0     # the order
    # record: the handle comes first of its own checks (nothing of it is read before), and num_games == 0 before that
    assert L.hexgnn_search_record(None, c, rec, None) == EINVAL
    assert L.hexgnn_search_record(None, ctypes.byref(_search_call(_lib, None, num_games=0)), None, None) == 0
    # a fake env handle of Hex-5 with 2 games: EnvDev starts (num_envs, size, nv, W, K)
    env = (ctypes.c_int * 64)(2, 5, 27, 1, 1)
    h = ctypes.c_void_p(ctypes.addressof(env))
    for other in ((3, 5, 27, 1, 1), (2, 4, 18, 1, 1)):
        wrong = (ctypes.c_int * 64)(*other)
        assert L.hexgnn_search_record(ctypes.c_void_p(ctypes.addressof(wrong)), c, rec, None) == EINVAL, other
    assert L.hexgnn_search_record(h, c, None, None) == EINVAL
    assert L.hexgnn_search_record(h, c, ctypes.byref(_record_call(_lib, p, struct_bytes=8)), None) == EINVAL
    for kw in (dict(capacity=49), dict(capacity=-1), dict(ply=-1), dict(pick_mode=2), dict(pick_mode=-1)):
        assert L.hexgnn_search_record(h, c, ctypes.byref(_record_call(_lib, p, **kw)), None) == EINVAL, kw
    for name in "head recorded u pick policy root_q z adj alive side sizes meta".split():
        assert L.hexgnn_search_record(h, c, ctypes.byref(_record_call(_lib, p, **{name: None})), None) == EINVAL, name
    assert L.hexgnn_search_record(h, c, ctypes.byref(_record_call(_lib, p, capacity=49, head=None)), None) == EINVAL
    # samples_finish
    fin = lambda first=0, count=3, cap=50, G=2, meta=fake, side=fake, z=fake, game=fake, status=fake: \
        L.hexgnn_samples_finish(first, count, cap, G, meta, side, z, game, status, None)                      # noqa: E731
    for kw in (dict(count=-1), dict(cap=0), dict(G=-1), dict(first=-1), dict(first=50), dict(count=51)):
        assert fin(**kw) == EINVAL, kw
    assert fin(count=0, meta=None, side=None, z=None, game=None, status=None) == 0
    assert fin(count=0, first=50) == EINVAL                                                                     # the order
    for name in ("meta", "side", "z", "game", "status"):
        assert fin(**{name: None}) == EINVAL, name
    # pv_loss
    assert L.hexgnn_pv_loss(None, None) == EINVAL
    assert L.hexgnn_pv_loss(ctypes.byref(_pv_call(_lib, p, struct_bytes=0)), None) == EINVAL
    for kw in (dict(b=-1), dict(n=-1), dict(m=-1), dict(hex_size=1), dict(capacity=0)):
        assert L.hexgnn_pv_loss(ctypes.byref(_pv_call(_lib, p, **kw)), None) == EINVAL, kw
    assert L.hexgnn_pv_loss(ctypes.byref(_pv_call(_lib, p, hex_size=26)), None) == EUNSUPPORTED
    assert L.hexgnn_pv_loss(ctypes.byref(_pv_call(_lib, p, hex_size=26, b=-1)), None) == EINVAL               # the order
    assert L.hexgnn_pv_loss(ctypes.byref(_pv_call(_lib, None, b=0)), None) == 0
    assert L.hexgnn_pv_loss(ctypes.byref(_pv_call(_lib, p, b=0, hex_size=26)), None) == EUNSUPPORTED
    for name in PV_POINTERS:
        assert L.hexgnn_pv_loss(ctypes.byref(_pv_call(_lib, p, **{name: None})), None) == EINVAL, name


# ---- (c) the proportional pick ---------------------------------------------------------------------------
def test_proportional_pick_against_a_numpy_restatement():
    rng = np.random.default_rng(3)
    last_u = np.nextafter(np.float32(1), np.float32(0))
    assert spo.prop_k(last_u, 12345) == 12344 and spo.prop_k(0.0, 12345) == 0
    for trial in range(40):
        ne = int(rng.integers(1, 90))
        N = rng.integers(0, 6, ne) * (rng.random(ne) < 0.6)
        if N.sum() == 0:
            N[int(rng.integers(0, ne))] = 3
        T = int(N.sum())
        owner = np.repeat(np.arange(ne), N)                  # owner[k] = the edge that owns visit k
        visited = np.nonzero(N)[0]
        # every k in [0, T) lands on the edge that owns it: u = (k 2^24 / T rounded up + a hair) / 2^24 maps to k
        for k in range(T):
            t = -(-(k << 24) // T)
            u = np.float32(t) / np.float32(16777216.0)
            assert spo.prop_k(u, T) == k, (trial, k)
            assert spo.proportional_pick(N, u) == owner[k] == int(np.searchsorted(np.cumsum(N), k, side="right")), (trial, k)
        assert spo.proportional_pick(N, np.float32(0)) == visited[0]
        assert spo.proportional_pick(N, last_u) == visited[-1]
        assert spo.greedy_pick(N) == int(np.argmax(N))
    row = spo.visit_policy(np.array([2, 5, 9]), np.array([3, 0, 4]), 9)
    assert row.dtype == np.float32 and row[0] == np.float32(3) / np.float32(7) and row[7] == np.float32(4) / np.float32(7)
    assert row[3] == 0 and np.count_nonzero(row) == 2


# ---- (d) the loss ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("q_ratio,vf,pf", [(0.0, 1.0, 1.0), (0.5, 0.01, 0.99)])
def test_oracle_loss_is_the_reference_expression(q_ratio, vf, pf):
    torch.manual_seed(1)
    rows = [3, 17, 146, 64]
    logp = [torch.log_softmax(torch.randn(r, dtype=torch.float64), 0).requires_grad_() for r in rows]
    target = []
    for r in rows:
        t = torch.rand(r, dtype=torch.float64) * (torch.rand(r) < 0.5)
        t[0] = 0.5
        target.append(t / t.sum())
    value = torch.tanh(torch.randn(len(rows), dtype=torch.float64)).requires_grad_()
    z = torch.tensor([1.0, -1.0, -1.0, 1.0], dtype=torch.float64)
    rq = torch.tanh(torch.randn(len(rows), dtype=torch.float64))
    # rl_loop/trainer_agent_pytorch.py: MSELoss(value, (1 - r) z + r q) * B and sum(-target * log_policy)
    y = (1 - q_ratio) * z + q_ratio * rq
    B = len(rows)
    policy_loss = torch.sum(-torch.cat(target) * torch.cat(logp))
    loss = vf * torch.nn.MSELoss()(value, y) * B + pf * policy_loss
    loss.backward()
    got, per, d_logp, d_value = spo.pv_loss([l.detach().numpy() for l in logp], [t.numpy() for t in target],
                                            value.detach().numpy(), z.numpy(), rq.numpy(), q_ratio, vf, pf)
    assert abs(got - loss.item()) <= 1e-12 * abs(loss.item())
    assert np.allclose(d_logp, torch.cat([l.grad for l in logp]).numpy(), rtol=1e-12, atol=0)
    assert np.allclose(d_value, value.grad.numpy(), rtol=1e-12, atol=1e-15)
    for g in range(B):
        assert per[g, 2] == float(int(torch.argmax(logp[g])) == int(torch.argmax(target[g])))
        assert per[g, 3] == float(torch.sign(value[g]) == torch.sign(y[g]))
    # first-index ties in both argmax metrics
    lp = np.log(np.array([0.25, 0.25, 0.25, 0.25]))
    assert spo.pv_loss([lp], [np.array([0.5, 0.5, 0, 0])], [0.0], [1.0], [0.0], 0.0, 1.0, 1.0)[1][0, 2] == 1
    assert spo.pv_loss([lp], [np.array([0.0, 0.5, 0.5, 0])], [0.0], [1.0], [0.0], 0.0, 1.0, 1.0)[1][0, 2] == 0
    assert spo.z_label(0, 1) == 1 and spo.z_label(0, 0) == -1 and spo.z_label(1, 0) == 1 and np.isnan(spo.z_label(-1, 1))


# ---- (e) python objects ----------------------------------------------------------------------------------
def test_python_objects_without_a_device():
    from gnn_hex_amd import ops, search_selfplay as ss
    assert hasattr(ops, "PolicyValueLossFn")
    with pytest.raises(ValueError):
        ss.SearchSampleBuffer(0, 5)
    with pytest.raises(ValueError):
        ss.SearchSampleBuffer(10, 26)
    with pytest.raises(Exception):
        ss.SearchSampleBuffer(10, 5, device="cpu")
    with pytest.raises(NotImplementedError):
        ss.PolicyValueUpdate(object(), None)
    with pytest.raises(TypeError):
        ss.SearchSelfPlay(4, 2, object(), 8, None)
