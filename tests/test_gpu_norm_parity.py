"""The two whole-batch normalisations under the float64 rule: the LayerNorm of ``modern_two_headed --norm=True`` (norm_*_kernel of
gnn_hex_amd/csrc/norm.hip, hexgnn_sage_norm_stack_*) and the CachedGraphNorm of the ``two_headed`` family (colnorm_*_kernel).

tests/test_gpu_norm.py and tests/test_gpu_two_headed.py hold these paths to absolute gates (2e-5 max-abs at five (n, hidden) pairs, 1e-4
on default-initialised networks whose gradients are ~ 1e-5).  This file runs beside them with the rule and the machinery of
tests/test_gpu_feature_counts.py and tests/test_gpu_wide_parity.py (tests/helpers.py).

Parity rule: ground truth is the torch expression / the oracle network in float64, the same in fp32 on the CPU gives the yardstick.
Outputs (y, Q, final_conv_acts, the mean CachedGraphNorm returns): max-abs error <= max(3 x fp32 oracle's, 5e-6).  Every gradient
tensor, dx, and the variance CachedGraphNorm returns: ||g - g64|| / ||g64|| <= max(3 x fp32 oracle's own, 2e-3), absolute 1e-6 where
||g64|| < 1e-6.  Inputs are chosen from the float64 oracle alone and every test asserts their conditions again: no tensor a ReLU is
applied to has an element within 2^-16 of its rms of zero, every gradient tensor has |g|max >= 1e-2, at model level the Q spread is
>= 0.5 (the stacks also keep the feature-sensitivity and column-share conditions of tests/test_gpu_feature_counts.py); the seed of a
case is the first below 400 that meets them.

Every reduction of norm.hip has the fixed shape of kNormBlocks = 512 row ranges, rows_per = ceil(n / 512); block r owns rows
[r rows_per, min(n, (r + 1) rows_per)), blocks past the end own nothing and must still write a zero partial.  The backward column sums
run in nph = min(16, 256 / (hp / 4)) row phases: 16, 16, 16, 16, 12, 10, 9, 8 for hp = 16..128.

1. The kernels through ops.graph_layernorm / ops.graph_colnorm (fresh and cached statistics), forward and backward of sum(y * R),
   ReLU off and on; x = randn * 3 + 1.5, weight ~ U(0.5, 1.5), bias ~ 0.3 N(0, 1), mean_scale ~ U(0.6, 1.4) (so that m (2 - m) and
   m^2 differ and d_mean_scale does not vanish).  y, dx, d_weight, d_bias, d_mean_scale and the returned statistics under the rule,
   pad columns of the padded y (and of the dx the backward returns) exactly zero, a second call bit-identical.
   - rows: n in {1, 2, 511, 512, 513, 1023, 1024, 1025} x H in {35, 80, 128}: one live block, the last block empty, every block
     one row, rows_per 2 and 3, a one-row ragged last block;
   - widths: n = 513, H = hp - 15 and H = hp for every hp = 16..128: all eight phase counts, a 16-byte column group that is all
     padding, no padding at all;
   - shifted: x moved to a mean of ten standard deviations (the variance comes from sum x^2 / cnt - mu^2), three shapes;
   - correlated: R = U(-1, 1) + (x - 1.5) / 3 at the same three shapes.  With R independent of x the statistics' own share of dx
     (k (x - mu), B o) is ~ 1 / sqrt(n H) of dx, and the other families cannot see 1 % of it (mutation (b) below);
   - dead and constant channels (colnorm): two all-zero columns (var_c = 0), one column constant at 1.5, one column with
     mean_scale == 1.  The zero columns' dx carries 1 / sqrt(eps) and would own the tensor's norm, so here every gradient is held
     to the rule per column group (zero / constant / mean_scale 1 / the others) as well;
   - constant batch (layernorm), every element 1.5: sigma == 0, which norm_bwd_apply_kernel special-cases as torch's std backward does.
     torch's float64 result is finite there (checked in the test) and equals the closed form dx = (g w - mean(g w)) / eps; the
     device is compared with it.  d_weight vanishes identically in this case (absolute 1e-6, as the rule has it);
   - empty batch (n = 0) through ops: the forward succeeds, the backward returns zero d_weight, d_bias, d_mean_scale;
   - live row count: ops.live_rows over a 1025-row buffer whose rows behind the count hold NaN, counts {0, 1, 511, 512, 513}: the
     bits of the exact-size call, and no element behind the count is written (y preset through ops' torch.empty);
   - poisoned scratch: per function n = 2 (510 empty blocks) and n = 1025 (rows_per 3) under PoisonedTorch(0xFF) and (0x00): the
     bits of the clean run.
2. ops.sage_norm_stack, three layers, perturbed norm weight and bias: c_in {1, 2, 8} x hidden {35, 80, 128} on the 196-row batch
   of tests/test_gpu_feature_counts.py; c_in == hidden == 35 (padded layout, with dx); 526 and 1036 rows (rows_per 2 and 3).  The
   loss is scaled by the smallest power of two at which the ORACLE's gradients meet 1e-2 (tests/test_gpu_wide_parity.py, section 3).
3. modern_two_headed --norm=True and two_headed with CachedGraphNorm: sharpen_ weights, every norm's weight, bias and mean_scale
   moved by 0.2 N(0, 1), 3 body + 2 head layers, both heads, default and advantages_only, loss mse(Q[sel], tgt); hidden 35 on a
   batch just over 512 rows and hidden 110 on four small boards.  Q, final_conv_acts and every parameter gradient under the rule
   (after_embed_norm and every norm's weight, bias and mean_scale included).  two_headed runs fresh statistics in train mode and
   the cache protocol: a set_cache forward in eval mode (Q and every cached mean / var under the rule), then an eval forward and
   backward on a different batch with the cached statistics.

Worst figures measured on the MI355X (printed per case and summed up at the end of the module; in brackets the fp32 oracle's own
distance from float64 in the same case):

  family                          y / Q, max-abs         gradient tensor, relative   dx, relative          statistics: mean max-abs, var relative
  1. rows                         1.15e-6 (1.04e-6)      9.86e-5 (2.91e-5)           2.62e-5 (9.09e-6)     2.38e-7 (2.38e-7), 3.27e-8 (6.56e-8)
  1. widths                       9.74e-7 (6.86e-7)      1.37e-7 (1.59e-7)           7.40e-8 (6.68e-8)     5.95e-8 (3.01e-7), 3.62e-8 (4.55e-8)
  1. shifted                      1.82e-6 (1.82e-6)      3.18e-7 (3.42e-7)           5.47e-8 (4.85e-8)     9.47e-7 (3.71e-6), 3.06e-8 (2.44e-7)
  1. correlated                   9.42e-7 (9.42e-7)      9.91e-8 (1.17e-7)           1.16e-7 (1.58e-7)     5.95e-8 (2.46e-7), 3.02e-8 (5.62e-8)
  1. dead channels                9.16e-7 (8.79e-7)      2.76e-4 (4.46e-3)           5.11e-8 (3.93e-8)     5.95e-8 (2.46e-7), 2.99e-8 (7.48e-8)
  1. constant batch               0 (0)                  9.83e-8 (1.43e-7)           (with the gradients)  --
  1. scratch                      9.16e-7 (8.79e-7)      1.68e-7 (2.62e-7)           2.88e-7 (2.83e-7)     2.38e-7 (2.38e-7), 2.99e-8 (7.43e-8)
  2. norm stack                   5.72e-6 (3.82e-6) [y]  8.12e-7 (5.85e-7)           2.89e-7 (2.08e-7)     layer-0 column 8.24e-7 (5.93e-7)
  3. modern_two_headed            2.16e-6 (1.51e-6)      2.02e-6 (1.13e-6)           acts 6.23e-6 (5.85e-6)   norm parameters 1.51e-6 (8.55e-7)
  3. two_headed, fresh            5.70e-6 (1.69e-5)      6.80e-6 (5.71e-6)           acts 9.99e-6 (1.57e-5)   norm parameters 4.29e-6 (4.45e-6)
  3. two_headed, cache protocol   4.18e-6 (6.52e-6)      5.91e-6 (9.22e-6)           acts 2.15e-5 (3.79e-5)   norm parameters 6.18e-6 (8.90e-6); cached mean
                                                                                                            5.00e-7 (2.65e-6), var 4.62e-7 (1.21e-6)

(the worst kernel gradients are d_mean_scale and dx of CachedGraphNorm on ONE row, n = 1: y = w o / sqrt(o^2 + eps) there, and
g - B o cancels to eps / (o^2 + eps) of g in both the kernel and the fp32 oracle; the 2.76e-4 is d_mean_scale of the constant column,
where the fp32 oracle itself is 4.46e-3 off).  The closest any case came to its bound: 0.74 on the norm stack's y (c_in 8, hidden 128:
5.72e-6 where the fp32 oracle is 3.82e-6 off, |y| ~ 10), 0.63 on final_conv_acts, 0.43 on Q; every gradient figure is below 0.05 of
its bound.  Of the 2739 summed-up figures 14 lie above three times the fp32 oracle's own and so rest on the 2e-3 floor (ten of them
CachedGraphNorm at n = 1 and 2, all <= 9.9e-5; the others <= 6e-6); no output needed the 5e-6 constant.  Every seed search ends below
16 (kernels <= 9, stacks <= 9, models <= 15); together they take about 25 s of CPU time per session.

Against libraries with one value-only change in norm.hip (built aside, never committed):
  (a) norm_apply_kernel, norm_bwd_apply_kernel and colnorm_finalize_kernel sum only the first 256 of the 512 partials: 182 cases
      fail -- every layernorm and fresh-colnorm kernel case with n >= 511 (more than 256 live blocks), the shifted, correlated, dead
      and constant cases, the rows_per-3 scratch cases, the stacks of 526 and 1036 rows, all eight hidden-35 model cases (517 / 522
      rows) and the hidden-35 cache protocol; n = 1 and 2, the cached-statistics kernel cases, the 196-row stacks and the hidden-110
      models (fewer than 257 live blocks: the dropped partials are zero) pass, as they must.
  (b) norm_bwd_apply_kernel uses 0.99 k: 17 cases fail -- all six correlated layernorm cases, layernorm at n = 1 (ReLU) and n = 2, the
      510-empty-blocks layernorm scratch case, three norm stacks (c_in 2 and 8 at hidden 35 on 196 rows, 1036 rows) and all four
      hidden-35 modern_two_headed cases; every colnorm case passes (untouched code), and so do the layernorm cases with R independent
      of x at n >= 511, where k (x - mu) is below 1 / 100 of dx: the reason the correlated family exists.
  (c) colnorm_bwd_finalize_kernel leaves C = 0 with fresh statistics: 110 cases fail -- every fresh-colnorm kernel case (rows,
      widths, shifted, correlated, dead, scratch), all eight two_headed model cases and the four
      cache-protocol cases (after_embed_norm is always fresh); every layernorm and cached-statistics case passes.
  (d) colnorm_finalize_kernel uses m * m for m * (2 - m): the same cases as (c) fail (variance, y and everything behind them).
tests/test_gpu_norm.py and tests/test_gpu_two_headed.py were not run against these libraries.
"""
import copy

import pytest
import torch

from helpers import (DEAD_CONST, DEAD_MS1, DEAD_ZERO, MARGIN, NORM_KINDS, SEEDS, PoisonedTorch, abs_bound, batch_tensors, check_grads,
                     model_step, norm_fwd_bwd, norm_inputs, norm_kernel_oracle, norm_leaves, norm_model_hip, norm_model_margin,
                     norm_model_ref, rel_bound, sel_and_targets, stack_oracle, stack_params)

pytestmark = pytest.mark.gpu

_kernels, _stacks, _models, _caches = {}, {}, {}, {}
_figures = {}           # (family, quantity) -> [worst error, oracle32's there, closest to its bound, figures, of them on a floor]


@pytest.fixture(autouse=True)
def _fp32():
    from gnn_hex_amd import ops
    ops.set_fused(True)
    ops.set_math("fp32")
    yield
    ops.set_fused(True)
    ops.set_math("fp32")


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    for (family, quantity), (e, e32, close, count, floored) in sorted(_figures.items()):
        print("worst %-22s %-12s %.3g (%.3g); closest to its bound %.3g; %d figures, %d above 3 x oracle32 (on the floor)"
              % (family, quantity, e, e32, close, count, floored))


def _note(family, quantity, e, e32, floor):
    bound = max(3.0 * e32, floor)
    ent = _figures.setdefault((family, quantity), [0.0, 0.0, 0.0, 0, 0])
    if e >= ent[0]:
        ent[0], ent[1] = e, e32
    ent[2] = max(ent[2], e / bound)
    ent[3] += 1
    ent[4] += int(e > 3.0 * e32)
    return e, e32


def _abs(family, quantity, tag, name, y, y32, y64):
    return _note(family, quantity, *abs_bound(tag, name, y, y32, y64, 5e-6), 5e-6)


def _rel(family, quantity, tag, name, g, g32, g64):
    return _note(family, quantity, *rel_bound(tag, name, g, g32, g64), 2e-3)


# ---- 1. the norm kernels ------------------------------------------------------------------------------------------------------

ROWS = [(n, h, "plain") for n in (1, 2, 511, 512, 513, 1023, 1024, 1025) for h in (35, 80, 128)]
WIDTHS = [(513, h, "plain") for hp in range(16, 129, 16) for h in (hp - 15, hp)]
SHIFTED = [(513, 35, "shift"), (512, 80, "shift"), (1025, 128, "shift")]
CORRELATED = [(513, 35, "corr"), (512, 80, "corr"), (1025, 128, "corr")]
DEAD = [(513, 35, "dead"), (1025, 128, "dead")]


def _hp(hidden):
    return (hidden + 15) // 16 * 16


def _rows_per(n):
    return (n + 511) // 512


def test_the_shapes_sit_where_this_file_says():
    from gnn_hex_amd import ops
    assert [_rows_per(n) for n in (1, 2, 511, 512, 513, 1023, 1024, 1025)] == [1, 1, 1, 1, 2, 2, 2, 3]
    assert 511 - 510 * 1 == 1 and 513 - 256 * 2 == 1 and 1025 - 341 * 3 == 2 and 1023 - 511 * 2 == 1        # ragged last live blocks
    assert (513 + 1) // 2 == 257 and (1025 + 2) // 3 == 342                                                # live blocks of 512
    assert [min(16, 256 // (hp // 4)) for hp in range(16, 129, 16)] == [16, 16, 16, 16, 12, 10, 9, 8]
    assert all(ops.padded_width(h) == _hp(h) for _, h, _ in ROWS + WIDTHS)


def _kernel_oracle(kind, n, hidden, variant):
    key = (kind, n, hidden, variant)
    if key not in _kernels:
        _kernels[key] = norm_kernel_oracle(kind, n, hidden, variant, zero_grads=("w",) if variant == "const" else ())
    o = _kernels[key]
    assert o["ok"], "%s: %s" % (key, o["text"])
    return o


def _padded(t, hidden):
    """The [n, hp] buffer behind a logical view [n, hidden] this library returned."""
    hp, n = _hp(hidden), t.shape[0]
    assert tuple(t.shape) == (n, hidden) and (n <= 1 or t.stride() == (hp, 1)), (tuple(t.shape), t.stride())
    return torch.as_strided(t, (n, hp), (hp, 1))


def _same_kernel_bits(tag, a, b):
    assert torch.equal(a["y"], b["y"]), "%s: y differs" % tag
    assert (a["stats"] is None) == (b["stats"] is None) and (a["stats"] is None or torch.equal(a["stats"], b["stats"])), tag
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), "%s: d_%s differs" % (tag, k)


def _column_groups(variant, hidden):
    if variant != "dead":
        return [("", slice(None))]
    special = list(DEAD_ZERO) + [DEAD_CONST, DEAD_MS1]
    return [("", slice(None)), ("[zero columns]", list(DEAD_ZERO)), ("[constant column]", [DEAD_CONST]),
            ("[mean_scale 1]", [DEAD_MS1]), ("[other columns]", [c for c in range(hidden) if c not in special])]


def _check_kernel(family, tag, kind, o, relu, got, variant="plain"):
    r64, r32, hidden = o["r64"][relu], o["r32"][relu], o["inp"]["x"].shape[1]
    assert tuple(got["y"].shape) == tuple(r64["y"].shape)
    ey = _abs(family, "y", tag, "y", got["y"], r32["y"], r64["y"])
    out = ["|y-y64| %.3g (oracle32 %.3g)" % ey]
    for k in norm_leaves(kind):
        quantity = "dx" if k == "x" else "gradient"
        for gname, cols in _column_groups(variant, hidden):
            e = _rel(family, quantity, tag, "d_%s%s" % (k, gname), got["grads"][k][..., cols], r32["grads"][k][..., cols],
                     r64["grads"][k][..., cols])
            out.append("d_%s%s rel %.3g (oracle32 %.3g)" % ((k, gname) + e))
    if kind == "colnorm":
        em = _abs(family, "mean", tag, "mean", got["stats"][0], r32["stats"][0], r64["stats"][0])
        ev = _rel(family, "var", tag, "var", got["stats"][1], r32["stats"][1], r64["stats"][1])
        out.append("|mean-mean64| %.3g (oracle32 %.3g), var rel %.3g (oracle32 %.3g)" % (em + ev))
    elif kind == "colnorm-cached":
        assert torch.equal(got["stats"].cpu(), o["inp"]["cache"]), "%s: the cached statistics came back changed" % tag
    hp = _hp(hidden)
    if hp != hidden:
        assert float(_padded(got["y"], hidden)[:, hidden:].abs().max()) == 0.0, "%s: a pad column of y is not zero" % tag
        assert float(_padded(got["raw_dx"], hidden)[:, hidden:].abs().max()) == 0.0, "%s: a pad column of dx is not zero" % tag
    print("%s: %s" % (tag, "; ".join(out)))


def _kernel_case(family, kind, n, hidden, variant, relu):
    o = _kernel_oracle(kind, n, hidden, variant)
    tag = "%s %s n %d hidden %d relu %d (rows_per %d, seed %d)" % (family, kind, n, hidden, relu, _rows_per(n), o["seed"])
    got = norm_fwd_bwd(kind, o["inp"], relu, device="cuda")
    _check_kernel(family, tag, kind, o, relu, got, variant)
    _same_kernel_bits(tag, got, norm_fwd_bwd(kind, o["inp"], relu, device="cuda"))
    return o, got


def _ids(cases):
    return ["n%d-h%d" % t[:2] for t in cases]


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("kind", NORM_KINDS)
@pytest.mark.parametrize("n,hidden,variant", ROWS, ids=_ids(ROWS))
def test_row_partition(n, hidden, variant, kind, relu):
    _kernel_case("1. rows", kind, n, hidden, variant, relu)


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("kind", NORM_KINDS)
@pytest.mark.parametrize("n,hidden,variant", WIDTHS, ids=_ids(WIDTHS))
def test_every_padded_width(n, hidden, variant, kind, relu):
    _kernel_case("1. widths", kind, n, hidden, variant, relu)


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("kind", NORM_KINDS)
@pytest.mark.parametrize("n,hidden,variant", SHIFTED, ids=_ids(SHIFTED))
def test_mean_of_ten_standard_deviations(n, hidden, variant, kind, relu):
    _kernel_case("1. shifted", kind, n, hidden, variant, relu)


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("kind", NORM_KINDS)
@pytest.mark.parametrize("n,hidden,variant", CORRELATED, ids=_ids(CORRELATED))
def test_upstream_gradient_correlated_with_the_input(n, hidden, variant, kind, relu):
    """R = U(-1, 1) + (x - 1.5) / 3: with R independent of x the k (x - mu) term of norm_bwd_apply_kernel and the B o term of
    colnorm_bwd_apply_kernel are ~ 1 / sqrt(n H) and 1 / sqrt(n) of dx, and 1 % of them hides under the 2e-3 floor."""
    _kernel_case("1. correlated", kind, n, hidden, variant, relu)


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("kind", ["colnorm", "colnorm-cached"])
@pytest.mark.parametrize("n,hidden,variant", DEAD, ids=_ids(DEAD))
def test_dead_and_constant_channels(n, hidden, variant, kind, relu):
    o, got = _kernel_case("1. dead channels", kind, n, hidden, variant, relu)
    x = o["inp"]["x"]
    assert float(x[:, list(DEAD_ZERO)].abs().max()) == 0.0 and bool((x[:, DEAD_CONST] == 1.5).all()) and o["inp"]["ms"][DEAD_MS1] == 1.0
    if kind == "colnorm":
        assert float(o["r64"][relu]["stats"][1][list(DEAD_ZERO)].abs().max()) == 0.0
        assert float(got["stats"][1][list(DEAD_ZERO)].abs().max()) == 0.0, "var of an all-zero column"


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("n,hidden", [(513, 35), (1025, 128)])
def test_constant_batch_layernorm(n, hidden, relu):
    """Every element 1.5: sigma == 0.  torch's float64 backward is finite there (std's backward masks the 0 / 0) and equals
    dx = (g w - mean(g w)) / eps; both are asserted before the device is compared with the float64 result."""
    o = _kernel_oracle("layernorm", n, hidden, "const")
    r64, inp = o["r64"][relu], o["inp"]
    assert all(bool(torch.isfinite(g).all()) for g in r64["grads"].values()) and bool(torch.isfinite(r64["y"]).all())
    g = inp["r"].double() * ((inp["b"].double() > 0) if relu else 1.0)
    gw = g * inp["w"].double()
    closed = (gw - gw.mean()) / 1e-5
    assert (r64["grads"]["x"] - closed).norm().item() <= 1e-9 * closed.norm().item()
    _kernel_case("1. constant batch", "layernorm", n, hidden, "const", relu)


@pytest.mark.parametrize("kind", NORM_KINDS)
@pytest.mark.parametrize("hidden", [35, 128])
def test_empty_batch(kind, hidden):
    inp = norm_inputs(kind, 0, hidden, "plain", 0)
    for relu in (False, True):
        got = norm_fwd_bwd(kind, inp, relu, device="cuda")
        assert tuple(got["y"].shape) == (0, hidden) and tuple(got["grads"]["x"].shape) == (0, hidden)
        for k in norm_leaves(kind)[1:]:
            g = got["grads"][k]
            assert tuple(g.shape) == (hidden,) and float(g.abs().max()) == 0.0, "%s n 0: d_%s is not zero" % (kind, k)


class _SentinelTorch(PoisonedTorch):
    """As PoisonedTorch, and every fp32 device tensor ops allocates (y, stats) starts at a value no norm output takes."""
    VALUE = -12345.0

    def empty(self, *args, **kwargs):
        t = PoisonedTorch.empty(self, *args, **kwargs)
        if t.dtype == torch.float32 and t.is_cuda:
            t.fill_(self.VALUE)
        return t


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("hidden", [35, 128])
def test_live_row_count(hidden, relu, monkeypatch):
    from gnn_hex_amd import ops
    cap = 1025
    inp = norm_inputs("layernorm", cap, hidden, "plain", 0)
    w, b = inp["w"].cuda(), inp["b"].cuda()
    for live in (0, 1, 511, 512, 513):
        x = inp["x"].cuda()
        x[live:] = float("nan")
        cnt = torch.tensor([live], dtype=torch.int32, device="cuda")
        stand_in = _SentinelTorch(0xFF)
        with monkeypatch.context() as mp:
            mp.setattr(ops, "torch", stand_in)
            with torch.no_grad(), ops.live_rows(cnt):
                got = ops.graph_layernorm(x, w, b, 1e-5, relu)
            torch.cuda.synchronize()
        assert stand_in.filled >= 1
        with torch.no_grad():
            want = ops.graph_layernorm(x[:live].contiguous(), w, b, 1e-5, relu)
        assert tuple(got.shape) == (cap, hidden) and tuple(want.shape) == (live, hidden)
        assert torch.equal(got[:live], want), "live %d of %d: not the bits of the exact-size call" % (live, cap)
        assert live == 0 or bool(torch.isfinite(want).all())
        behind = _padded(got, hidden)[live:]
        assert bool((behind == _SentinelTorch.VALUE).all()), "live %d of %d: a row behind the count was written" % (live, cap)


@pytest.mark.parametrize("kind", NORM_KINDS)
@pytest.mark.parametrize("n,hidden", [(2, 35), (1025, 128)], ids=["510-empty-blocks", "rows_per-3"])
def test_results_do_not_depend_on_the_scratch(n, hidden, kind, monkeypatch):
    from gnn_hex_amd import ops
    o = _kernel_oracle(kind, n, hidden, "plain")
    clean = norm_fwd_bwd(kind, o["inp"], True, device="cuda")
    _check_kernel("1. scratch", "scratch %s n %d hidden %d" % (kind, n, hidden), kind, o, True, clean)
    for byte in (0xFF, 0x00):
        stand_in = PoisonedTorch(byte)
        with monkeypatch.context() as mp:
            mp.setattr(ops, "torch", stand_in)
            got = norm_fwd_bwd(kind, o["inp"], True, device="cuda")
        assert stand_in.filled >= 2, "the scratch of this path did not come through ops' torch.empty"
        _same_kernel_bits("%s n %d hidden %d with 0x%02X scratch" % (kind, n, hidden, byte), clean, got)


# ---- 2. the norm stack ------------------------------------------------------------------------------------------------------

SIZES = [1, 2, 3, 17, 40, 128, 5]                   # 196 rows
SIZES_526 = SIZES + [130, 200]                      # rows_per 2
SIZES_1036 = SIZES_526 + [250, 260]                 # rows_per 3
STACKS = [(c, h, "196") for c in (1, 2, 8) for h in (35, 80, 128)] + [(35, 35, "196"), (2, 35, "526"), (8, 35, "1036")]
_SIZES = {"196": SIZES, "526": SIZES_526, "1036": SIZES_1036}


@pytest.mark.parametrize("c_in,hidden,rows", STACKS, ids=["c%d-h%d-n%s" % t for t in STACKS])
def test_sage_norm_stack(c_in, hidden, rows):
    from gnn_hex_amd import ops
    key = (c_in, hidden, rows)
    if key not in _stacks:
        _stacks[key] = stack_oracle("norm", c_in, hidden, _SIZES[rows])
    o = _stacks[key]
    assert o["ok"], "%s: %s" % (key, o["text"])
    x, ei, n = o["x"], o["ei"], o["x"].shape[0]
    assert n == int(rows) and _rows_per(n) == {"196": 1, "526": 2, "1036": 3}[rows]
    padded = c_in == hidden
    dev = copy.deepcopy(o["m"]).cuda()
    xd = x.cuda().requires_grad_(padded)
    y = ops.sage_norm_stack(xd, ops.GraphStructure(ei.cuda(), n), c_in, hidden, list(dev.convs), list(dev.norms))
    ((y * o["r"].cuda()).sum() * o["scale"] / n).backward()
    torch.cuda.synchronize()
    tag = "norm stack c_in %d hidden %d rows %d (seed %d)" % (c_in, hidden, n, o["seed"])
    ey = _abs("2. norm stack", "y", tag, "y", y, o["y32"], o["y64"])
    names, ps = stack_params(dev)
    worst = (0.0, 0.0, "")
    for i, (name, p, a32, a64) in enumerate(zip(names, ps, o["g32"], o["g64"])):
        assert p.grad is not None and tuple(p.grad.shape) == tuple(a64.shape), name
        worst = max(worst, _rel("2. norm stack", "gradient", tag, name, p.grad, a32, a64) + (name,))
        if i in (0, 2) and not padded:                  # the raw first layer: every feature column against its own norm
            for k in range(c_in):
                _rel("2. norm stack", "layer-0 column", tag, "%s[:, %d]" % (name, k), p.grad[:, k], a32[:, k], a64[:, k])
    text = ""
    if padded:
        assert xd.grad is not None and tuple(xd.grad.shape) == tuple(x.shape)
        text = "; dx rel %.3g (oracle32 %.3g)" % _rel("2. norm stack", "dx", tag, "dx", xd.grad, o["dx32"], o["dx64"])
    print("%s: |y-y64| %.3g (oracle32 %.3g); worst gradient tensor %s rel %.3g (oracle32 %.3g)%s"
          % (tag, ey[0], ey[1], worst[2], worst[0], worst[1], text))


# ---- 3. the two model families ------------------------------------------------------------------------------------------------

BODY, HEAD = 3, 2
BOARDS = {35: [11, 11, 11, 11, 11, 10, 10, 10, 10], 110: [5, 7, 9, 7]}      # 517 / 522 rows (maker / breaker), 132 / 122
OTHER_BOARDS = {35: [9, 11, 7, 5], 110: [7, 6, 8]}           # the batch whose statistics the cache protocol stores
MODES = [("default", {}), ("advantages_only", {"advantages_only": True})]


def _model_batch(sizes, maker):
    x, ei, bv, ptr = batch_tensors("D1", sizes, maker=maker)
    sel, tgt = sel_and_targets(ptr)
    return (x, ei, bv, ptr), sel, tgt


def _model_figures(margin, q64, g64):
    spread = (q64.max() - q64.min()).item()
    gmax = min(g.abs().max().item() for g in g64.values() if g is not None)
    ok = margin >= MARGIN and spread >= 0.5 and gmax >= 1e-2
    return ok, "Q spread %.3g (>= 0.5), smallest |g|max %.3g (>= 1e-2), smallest |ReLU input| / rms %.3g (>= 2^-16)" % (spread, gmax, margin)


def _f64(batch):
    return (batch[0].double(),) + tuple(batch[1:])


def _model_oracle(family, hidden, maker):
    """Fresh statistics, train mode, both modes at one weight seed."""
    key = (family, hidden, maker)
    if key not in _models:
        batch, sel, tgt = _model_batch(BOARDS[hidden], maker)
        for seed in range(SEEDS):
            ref = norm_model_ref(family, BODY, hidden, seed).train()
            ref64, res64, texts, margins = copy.deepcopy(ref).double(), {}, {}, {}
            for mode, kw in MODES:
                margin, res = norm_model_margin(ref64, maker, lambda: model_step(ref64, _f64(batch), sel, tgt.double(), **kw))
                ok, texts[mode] = _model_figures(margin, res[0], res[2])
                if not ok:
                    break
                res64[mode], margins[mode] = res, margin
            if len(res64) == len(MODES):
                break
        else:
            raise AssertionError("%s: no weight seed below %d meets the oracle conditions" % (key, SEEDS))
        res32 = {mode: model_step(ref, batch, sel, tgt, **kw) for mode, kw in MODES}
        for mode, _ in MODES:
            print("oracle %s hidden %d maker %s %s, %d rows: weight seed %d; %s" % (family, hidden, maker, mode, batch[0].shape[0], seed, texts[mode]))
        _models[key] = dict(ref=ref, seed=seed, batch=batch, sel=sel, tgt=tgt, res64=res64, res32=res32, texts=texts, margins=margins)
    o = _models[key]
    for mode, _ in MODES:
        assert _model_figures(o["margins"][mode], o["res64"][mode][0], o["res64"][mode][2])[0], o["texts"][mode]
    return o


def _check_model(family, tag, ref, got, r32, r64):
    q, acts, g = got
    assert tuple(q.shape) == tuple(r64[0].shape) and tuple(acts.shape) == tuple(r64[1].shape)
    eq = _abs(family, "Q", tag, "Q", q, r32[0], r64[0])
    ea = _abs(family, "final_conv_acts", tag, "final_conv_acts", acts, r32[1], r64[1])
    names = [k for k, _ in ref.named_parameters()]
    assert sorted(g) == sorted(names) and sorted(r64[2]) == sorted(names)
    live = [k for k in names if r64[2][k] is not None]
    assert any("after_embed_norm" in k for k in live) and any("mean_scale" in k for k in live) == ("two_headed" in family and "modern" not in family)
    for k in names:
        if r64[2][k] is None:
            assert g[k] is None or float(g[k].abs().max()) == 0.0, k
    first = (live.index("gnn.convs.0.lin_l.weight"), live.index("gnn.convs.0.lin_r.weight"))
    worst, worst_col = check_grads(tag, live, [g[k] for k in live], [r32[2][k] for k in live], [r64[2][k] for k in live], 2, first=first)
    worst_norm = (0.0, 0.0, "")
    for k in live:
        r = rel_bound(tag, k, g[k], r32[2][k], r64[2][k])
        _note(family, "norm parameter" if "norm" in k else "gradient", r[0], r[1], 2e-3)
        if "norm" in k:
            worst_norm = max(worst_norm, r + (k,))
    print("%s: |Q-Q64| %.3g (oracle32 %.3g); |acts-acts64| %.3g (oracle32 %.3g); worst gradient tensor %s rel %.3g (oracle32 %.3g); worst "
          "norm parameter %s rel %.3g (oracle32 %.3g); worst layer-0 column %s rel %.3g (oracle32 %.3g)"
          % (tag, eq[0], eq[1], ea[0], ea[1], worst[2], worst[0], worst[1], worst_norm[2], worst_norm[0], worst_norm[1],
             worst_col[2], worst_col[0], worst_col[1]))


MODEL_CASES = [(h, m) for h in (35, 110) for m in (True, False)]
MODEL_IDS = ["h%d-%s" % (h, "maker" if m else "breaker") for h, m in MODEL_CASES]


@pytest.mark.parametrize("mode", [0, 1], ids=[m for m, _ in MODES])
@pytest.mark.parametrize("family", ["modern_two_headed", "two_headed"])
@pytest.mark.parametrize("hidden,maker", MODEL_CASES, ids=MODEL_IDS)
def test_model_with_fresh_statistics(hidden, maker, family, mode):
    o = _model_oracle(family, hidden, maker)
    n = o["batch"][0].shape[0]
    assert (hidden == 35) == (_rows_per(n) == 2) and (hidden == 35) == (512 < n <= 530), n
    hip = norm_model_hip(family, o["ref"], BODY, hidden).train()
    assert hip.after_embed_norm is not None and len(hip.gnn.norms) == BODY and len(hip.maker_head.gnn.norms) == HEAD
    name, kw = MODES[mode]
    got = model_step(hip, tuple(t.cuda() for t in o["batch"]), o["sel"].cuda(), o["tgt"].cuda(), **kw)
    torch.cuda.synchronize()
    tag = "%s hidden %d maker %s %s %d rows (seed %d)" % (family, hidden, maker, name, n, o["seed"])
    _check_model("3. " + family, tag, o["ref"], got, o["res32"][name], o["res64"][name])


def _norms_of(model, maker):
    head = model.maker_head if maker else model.breaker_head
    return [("gnn.norms.%d" % i, m) for i, m in enumerate(model.gnn.norms)] + \
           [("head.gnn.norms.%d" % i, m) for i, m in enumerate(head.gnn.norms)]


def _cache_protocol(model, maker, batch_a, batch_b, sel, tgt):
    """eval mode: a set_cache forward on batch a, then a forward and backward on batch b with the cached statistics:
    (Q of a, [(name, mean_cache, var_cache)], model_step's result on b)."""
    model.eval()
    with torch.no_grad():
        qa = model(*batch_a, set_cache=True).detach().reshape(-1)
    caches = [(k, m.mean_cache.detach().clone(), m.var_cache.detach().clone()) for k, m in _norms_of(model, maker)]
    return qa, caches, model_step(model, batch_b, sel, tgt)


def _cache_oracle(hidden, maker):
    key = (hidden, maker)
    if key not in _caches:
        batch_a = _model_batch(OTHER_BOARDS[hidden], maker)[0]
        batch_b, sel, tgt = _model_batch(BOARDS[hidden], maker)
        for seed in range(SEEDS):
            ref = norm_model_ref("two_headed", BODY, hidden, seed)
            ref64 = copy.deepcopy(ref).double()
            margin, res64 = norm_model_margin(ref64, maker, lambda: _cache_protocol(ref64, maker, _f64(batch_a), _f64(batch_b), sel, tgt.double()))
            ok, text = _model_figures(margin, res64[2][0], res64[2][2])
            spread_a = (res64[0].max() - res64[0].min()).item()
            if ok and spread_a >= 0.5:
                break
        else:
            raise AssertionError("%s: no weight seed below %d meets the oracle conditions" % (key, SEEDS))
        text += ", Q spread of the set_cache batch %.3g (>= 0.5)" % spread_a
        print("oracle two_headed cache protocol hidden %d maker %s, %d then %d rows: weight seed %d; %s"
              % (hidden, maker, batch_a[0].shape[0], batch_b[0].shape[0], seed, text))
        res32 = _cache_protocol(copy.deepcopy(ref), maker, batch_a, batch_b, sel, tgt)
        _caches[key] = dict(ref=ref, seed=seed, batch_a=batch_a, batch_b=batch_b, sel=sel, tgt=tgt, res64=res64, res32=res32, text=text,
                            margin=margin, spread_a=spread_a)
    o = _caches[key]
    assert o["spread_a"] >= 0.5 and _model_figures(o["margin"], o["res64"][2][0], o["res64"][2][2])[0], o["text"]
    return o


@pytest.mark.parametrize("hidden,maker", MODEL_CASES, ids=MODEL_IDS)
def test_two_headed_cache_protocol(hidden, maker):
    o = _cache_oracle(hidden, maker)
    hip = norm_model_hip("two_headed", o["ref"], BODY, hidden)
    qa, caches, got = _cache_protocol(hip, maker, tuple(t.cuda() for t in o["batch_a"]), tuple(t.cuda() for t in o["batch_b"]),
                                      o["sel"].cuda(), o["tgt"].cuda())
    torch.cuda.synchronize()
    head = hip.maker_head if maker else hip.breaker_head
    assert hip.gnn.has_cache and head.gnn.has_cache and not hip.training
    family = "3. two_headed, cached"
    tag = "two_headed cache protocol hidden %d maker %s (seed %d)" % (hidden, maker, o["seed"])
    (qa64, c64, r64), (qa32, c32, r32) = o["res64"], o["res32"]
    ea = _abs(family, "Q", tag, "Q of the set_cache forward", qa, qa32, qa64)
    assert [k for k, _, _ in caches] == [k for k, _, _ in c64] and len(caches) == BODY + HEAD
    wm, wv = (0.0, 0.0), (0.0, 0.0)
    for (k, mean, var), (_, mean32, var32), (_, mean64, var64) in zip(caches, c32, c64):
        assert tuple(mean.shape) == tuple(mean64.shape) == (1, hidden) and tuple(var.shape) == (1, hidden)
        wm = max(wm, _abs(family, "mean", tag, k + ".mean_cache", mean, mean32, mean64))
        wv = max(wv, _rel(family, "var", tag, k + ".var_cache", var, var32, var64))
    print("%s: |Q-Q64| of the set_cache forward %.3g (oracle32 %.3g); worst |mean_cache - mean64| %.3g (oracle32 %.3g); worst var_cache rel "
          "%.3g (oracle32 %.3g)" % ((tag,) + ea + wm + wv))
    _check_model(family, tag, o["ref"], got, r32, r64)
