"""fp32 stride-1 conv trio (fconv.hip) and the fp32 linear head (linear.hip
templated on the activation type).

First order is held to a DERIVED bound against the exact-input float64
oracle (tests/_oracle.py, ``widen`` on every input, nothing rounded): an
n-term fp32 chain in any order, split sums included, satisfies

    |err| <= (n + 2) * 2^-24 * sum |a||b|

with sum |a||b| taken from the oracle on absolute values and n = 9C + 1
(y), 9F (dx), NB*Ho*Wo (dw, db), K (linear fwd), ways (linear dx), M
(linear dw, db).  The bound is loose at long reductions, so the same shapes
also run on small integers, where every product and partial sum is exact in
fp32 and the results must EQUAL the oracle: that is what catches a dropped
or doubled term.

fconv_wgrad sizes its K chunk for ~3072 blocks, so a chunk is one 32-position
K-step unless positions * ceil(9C/64) * T exceeds 98304: the nine shapes of
the issue span many chunks (97 at (3,7,21,21,48,48,1)) but never run the K
loop twice.  The MULTI_STEP shapes do, which is what every workload shape
does: the carried (wo, ho, img) decode, the register prefetch feeding a
second staging and db accumulated across steps.  ``_wgrad_ksteps`` mirrors
the launcher's sizing and the tests assert the step count, so a retuned
launcher cannot quietly take the coverage away.

Second order (the three scenarios of tests/test_tconv_shapes_gpu.py) is
compared with the same composition on the float64 oracle ops at rtol 1e-4,
atol 1e-5 * max|ref| — the scale of the project's fp32 tests."""

import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

import _oracle as orc
from howtotrainyourmamlpytorch_amd import ops
from howtotrainyourmamlpytorch_amd.ops import hip_autograd

EPS = 2.0 ** -24


def dev():
    return torch.device("cuda", 0)


def _id(s):
    return "x".join(map(str, s))


# (T, NB, H, W, C, F, pad)
SHAPES = [
    (2, 3, 11, 9, 48, 48, 1),    # odd, non-square
    (2, 3, 12, 11, 64, 64, 0),   # maximum channels, dgrad at pad' = 2
    (2, 3, 7, 7, 8, 8, 1),       # smallest aligned shape
    (2, 5, 14, 14, 1, 64, 1),    # first layer; dx at Co = 1
    (2, 5, 14, 14, 3, 48, 1),    # ... and Co = 3
    (1, 2, 3, 3, 16, 32, 0),     # Ho = Wo = 1: two reduction positions in wgrad
    (3, 7, 21, 21, 48, 48, 1),   # M = 3087: several M tiles, ragged last
    (2, 3, 10, 10, 16, 48, 1),   # C != F: a swapped repack fails
    (2, 3, 9, 9, 5, 5, 1),       # K = 45: no alignment anywhere
]

# several K-steps per wgrad chunk, ragged last step, Wo not dividing 32
MULTI_STEP = [
    (8, 20, 21, 21, 48, 48, 1),   # chunk 192 = 6 steps; row and image carries
    (16, 30, 23, 22, 5, 6, 1),    # chunk 96 = 3 steps; scalar gathers (C, F % 4 != 0)
    (8, 1500, 3, 3, 16, 16, 1),   # chunk 128 = 4 steps; a step spans 3 images
]
SHAPES = SHAPES + MULTI_STEP


def _wgrad_ksteps(shape):
    """K-steps per chunk as fconv_wgrad's launcher sizes them."""
    T, NB, H, W, C, F, pad = shape
    pos = NB * (H + 2 * pad - 2) * (W + 2 * pad - 2)
    gridx = (9 * C + 63) // 64
    want = max(1, 3072 // (gridx * T))
    kchunk = max(32, -(-(-(-pos // want)) // 32) * 32)
    return kchunk // 32, pos % kchunk


def test_multi_step_shapes_run_the_wgrad_k_loop_more_than_once():
    assert [_wgrad_ksteps(s) for s in MULTI_STEP] == [(6, 180), (3, 12), (4, 60)]
    # ragged last K-step in the last chunk, and Wo does not divide the step
    for s in MULTI_STEP:
        assert _wgrad_ksteps(s)[1] % 32 != 0 and 32 % (s[3] + 2 * s[6] - 2) != 0


def _mk(shape, integers):
    T, NB, H, W, C, F, pad = shape
    g = torch.Generator().manual_seed(sum(shape))
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    if integers:
        def ri(*s):
            return torch.randint(-3, 4, s, generator=g).float()
        return ri(T, NB, H, W, C), ri(T, F, C, 3, 3) * 0.25, ri(T, F), \
            ri(T, NB, Ho, Wo, F)
    return (torch.randn(T, NB, H, W, C, generator=g),
            torch.randn(T, F, C, 3, 3, generator=g).mul(0.1),
            torch.randn(T, F, generator=g),
            torch.randn(T, NB, Ho, Wo, F, generator=g))


def _oracle_all(x, w, b, dy, pad):
    """(y, dx, dw, db) of the float64 oracle for float64 CPU inputs."""
    xo, wo, bo = (t.clone().requires_grad_(True) for t in (x, w, b))
    yo = orc.conv3x3(xo, wo, bo, 1, pad)
    return (yo.detach(),) + torch.autograd.grad(yo, (xo, wo, bo), dy)


def _kernel_all(x, w, b, dy, pad):
    xg = x.to(dev()).requires_grad_(True)
    wg = w.to(dev()).requires_grad_(True)
    bg = b.to(dev()).requires_grad_(True)
    y = ops.task_conv3x3(xg, wg, bg, stride=1, padding=pad)
    return (y.detach(),) + torch.autograd.grad(y, (xg, wg, bg), dy.to(dev()))


def _assert_bounded(got, ref, mag, n, name):
    """|got - ref| <= (n + 2) 2^-24 mag, elementwise."""
    assert got.dtype == torch.float32, (name, got.dtype)
    got = orc.widen(got)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    worst = orc._report(name, (got - ref).abs(), (n + 2) * EPS * mag)
    assert worst <= 1.0, f"{name}: err/bound {worst:.3f} (n={n})"


# ---------------------------------------------------------------------------
# 1. dispatch
# ---------------------------------------------------------------------------
def test_fp32_dispatch_reaches_the_kernels(monkeypatch):
    ext = ops.hip_ext()
    for name in ("fconv_mm", "fconv_repack", "fconv_wgrad"):
        assert hasattr(ext, name), name
    monkeypatch.delenv("MAML355_FCONV", raising=False)
    x, w, b, dy = _mk((2, 3, 7, 7, 8, 8, 1), False)

    hip_autograd._FALLBACK_WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        y, dx, dw, db = _kernel_all(x, w, b, dy, 1)
    assert not [r for r in rec if "grouped-ATen composition" in str(r.message)]
    for t in (y, dx, dw, db):
        assert t.dtype == torch.float32

    # the linear head reaches lin_fwd with fp32 activations
    calls = []
    real = ext.lin_fwd

    def spy(xx, *a):
        calls.append(xx.dtype)
        return real(xx, *a)

    monkeypatch.setattr(ext, "lin_fwd", spy)
    g = torch.Generator().manual_seed(1)
    lx = torch.randn(2, 9, 64, generator=g).to(dev())
    lw = torch.randn(2, 5, 64, generator=g).to(dev())
    lb = torch.randn(2, 5, generator=g).to(dev())
    ly = ops.task_linear(lx, lw, lb)
    assert calls == [torch.float32] and ly.dtype == torch.float32

    # MAML355_FCONV=0: the grouped-ATen composition and torch.bmm are back
    monkeypatch.setenv("MAML355_FCONV", "0")
    hip_autograd._FALLBACK_WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        y0 = ops.task_conv3x3(x.to(dev()), w.to(dev()), b.to(dev()),
                              stride=1, padding=1)
    assert [r for r in rec if "grouped-ATen composition" in str(r.message)]
    torch.testing.assert_close(y0, y, rtol=1e-4, atol=1e-4)
    calls.clear()
    ly0 = ops.task_linear(lx, lw, lb)
    assert calls == []
    torch.testing.assert_close(ly0, ly, rtol=1e-4, atol=1e-4)
    hip_autograd._FALLBACK_WARNED.clear()


def test_fp32_return_stats_yields_empty_sums():
    x, w, b, _ = _mk((2, 3, 7, 7, 8, 8, 1), False)
    y, sums = ops.task_conv3x3(x.to(dev()), w.to(dev()), b.to(dev()),
                               stride=1, padding=1, return_stats=True)
    assert y.dtype == torch.float32 and sums.numel() == 0


# ---------------------------------------------------------------------------
# 2. first order under the derived bound; 3. exact integers
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_fconv_first_order_within_derived_bound(shape):
    T, NB, H, W, C, F, pad = shape
    x, w, b, dy = _mk(shape, False)
    y, dx, dw, db = _kernel_all(x, w, b, dy, pad)
    xo, wo, bo, dyo = map(orc.widen, (x, w, b, dy))
    yo, dxo, dwo, dbo = _oracle_all(xo, wo, bo, dyo, pad)
    my, mdx, mdw, mdb = _oracle_all(xo.abs(), wo.abs(), bo.abs(), dyo.abs(), pad)
    pos = NB * (H + 2 * pad - 2) * (W + 2 * pad - 2)
    _assert_bounded(y, yo, my, 9 * C + 1, "y")
    _assert_bounded(dx, dxo, mdx, 9 * F, "dx")
    _assert_bounded(dw, dwo, mdw, pos, "dw")
    _assert_bounded(db, dbo, mdb, pos, "db")


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_fconv_exact_on_small_integers(shape):
    pad = shape[-1]
    x, w, b, dy = _mk(shape, True)
    got = _kernel_all(x, w, b, dy, pad)
    want = _oracle_all(*map(orc.widen, (x, w, b, dy)), pad)
    for name, g_, r_ in zip(("y", "dx", "dw", "db"), got, want):
        assert g_.dtype == torch.float32, name
        assert torch.equal(orc.widen(g_), r_), \
            f"{name}: max|diff| {(orc.widen(g_) - r_).abs().max().item():.3e}"


# ---------------------------------------------------------------------------
# 4. second order against the same composition on the float64 oracle
# ---------------------------------------------------------------------------
class _Orc:
    @staticmethod
    def task_conv3x3(x, w, b=None, stride=1, padding=1):
        return orc.conv3x3(x, w, b, stride, padding)

    @staticmethod
    def task_linear(x, w, b=None):
        return orc.linear(x, w, b)


def _close2(got, ref, name):
    got, ref = orc.widen(got), ref.detach()
    atol = 1e-5 * ref.abs().max().item()
    worst = orc._report(name, (got - ref).abs(), atol + 1e-4 * ref.abs())
    assert worst <= 1.0, f"{name}: err/bound {worst:.3f}"


def _inner_outer(opmod, x_, w_, b_, pad):
    """The inner step updates w AND b from their grads, so the outer
    backward reaches the wgrad Function with a grad for the fused db."""
    y = opmod.task_conv3x3(x_, w_, b_, stride=1, padding=pad)
    gw, gb = torch.autograd.grad((y ** 2).mean(), (w_, b_), create_graph=True)
    y2 = opmod.task_conv3x3(x_, w_ - 0.1 * gw, b_ - 0.1 * gb, stride=1,
                            padding=pad)
    return torch.autograd.grad((y2 ** 2).mean(), (w_, b_))


def _through_input(opmod, x_, w_, pad):
    """create_graph through dgrad: _FConvDgradFn.backward (fwd + wgrad)."""
    y = opmod.task_conv3x3(x_, w_, None, stride=1, padding=pad)
    (gx,) = torch.autograd.grad((y ** 2).mean(), (x_,), create_graph=True)
    return torch.autograd.grad((gx ** 2).sum(), (x_, w_))


SECOND = [(2, 2, 8, 8, 48, 48, 1), (2, 2, 9, 7, 16, 32, 0),
          (2, 2, 9, 8, 16, 32, 1)]


@pytest.mark.parametrize("shape", SECOND, ids=_id)
def test_fconv_second_order_with_updated_bias(shape):
    pad = shape[-1]
    x, w, b, _ = _mk(shape, False)
    gw, gb = _inner_outer(ops, x.to(dev()), w.to(dev()).requires_grad_(True),
                          b.to(dev()).requires_grad_(True), pad)
    gwo, gbo = _inner_outer(_Orc, orc.widen(x), orc.widen(w).requires_grad_(True),
                            orc.widen(b).requires_grad_(True), pad)
    assert gw.dtype == torch.float32 and gb.dtype == torch.float32
    _close2(gw, gwo, "outer gw")
    _close2(gb, gbo, "outer gb")


@pytest.mark.parametrize("shape", SECOND, ids=_id)
def test_fconv_second_order_through_input(shape):
    pad = shape[-1]
    x, w, _, _ = _mk(shape, False)
    gx, gw = _through_input(ops, x.to(dev()).requires_grad_(True),
                            w.to(dev()).requires_grad_(True), pad)
    gxo, gwo = _through_input(_Orc, orc.widen(x).requires_grad_(True),
                              orc.widen(w).requires_grad_(True), pad)
    _close2(gx, gxo, "gx")
    _close2(gw, gwo, "gw")


def test_linear_fp32_second_order_through_weight_and_bias_grads():
    """A loss on gw and gb: _LinWgradFn.backward with a grad for the fused
    bias gradient, fp32 instantiation."""
    T, M, K, ways = 3, 17, 200, 5
    g = torch.Generator().manual_seed(21)
    x = torch.randn(T, M, K, generator=g)
    w = torch.randn(T, ways, K, generator=g).mul(0.1)
    b = torch.randn(T, ways, generator=g)

    def run(opmod, x_, w_, b_):
        y = opmod.task_linear(x_, w_, b_)
        gw, gb = torch.autograd.grad((y ** 2).mean(), (w_, b_), create_graph=True)
        return torch.autograd.grad((gw ** 2).sum() + (gb ** 2).sum(), (w_, b_))

    sw, sb = run(ops, x.to(dev()), w.to(dev()).requires_grad_(True),
                 b.to(dev()).requires_grad_(True))
    swo, sbo = run(_Orc, orc.widen(x), orc.widen(w).requires_grad_(True),
                   orc.widen(b).requires_grad_(True))
    assert sw.dtype == torch.float32 and sb.dtype == torch.float32
    _close2(sw, swo, "sw")
    _close2(sb, sbo, "sb")


# ---------------------------------------------------------------------------
# 5. repeatability, without MAML355_DETERMINISTIC
# ---------------------------------------------------------------------------
def test_fconv_kernels_bitwise_repeatable(monkeypatch):
    monkeypatch.delenv("MAML355_DETERMINISTIC", raising=False)
    shape = (3, 7, 21, 21, 48, 48, 1)
    x, w, b, dy = (t.to(dev()) for t in _mk(shape, False))
    ext = ops.hip_ext()
    wp = ext.fconv_repack(w, False)
    y1 = ext.fconv_mm(x, wp, b, 1, 21, 21)
    y2 = ext.fconv_mm(x, wp, b, 1, 21, 21)
    assert torch.equal(y1, y2)
    dw1, db1 = ext.fconv_wgrad(dy, x, 1, True)
    dw2, db2 = ext.fconv_wgrad(dy, x, 1, True)
    assert torch.equal(dw1, dw2) and torch.equal(db1, db2)


# ---------------------------------------------------------------------------
# 6. fp32 linear head
# ---------------------------------------------------------------------------
def _lin_all(opmod, x, w, b, dy):
    x_, w_, b_ = (t.requires_grad_(True) for t in (x, w, b))
    y = opmod.task_linear(x_, w_, b_)
    return (y.detach(),) + torch.autograd.grad(y, (x_, w_, b_), dy)


@pytest.mark.parametrize("integers", [False, True], ids=["random", "integers"])
@pytest.mark.parametrize("shape", [(2, 9, 64, 5), (2, 7, 1200, 20)], ids=_id)
def test_linear_fp32_matches_oracle(shape, integers):
    T, M, K, ways = shape
    g = torch.Generator().manual_seed(sum(shape))
    if integers:
        def mk(*s):
            return torch.randint(-3, 4, s, generator=g).float()
        x, w, b, dy = mk(T, M, K), mk(T, ways, K) * 0.25, mk(T, ways), mk(T, M, ways)
    else:
        x, w, b, dy = (torch.randn(T, M, K, generator=g),
                       torch.randn(T, ways, K, generator=g).mul(0.1),
                       torch.randn(T, ways, generator=g),
                       torch.randn(T, M, ways, generator=g))
    got = _lin_all(ops, *(t.to(dev()) for t in (x, w, b, dy)))
    wide = [orc.widen(t) for t in (x, w, b, dy)]
    want = _lin_all(_Orc, *[t.clone() for t in wide])
    for g_ in got:
        assert g_.dtype == torch.float32
    if integers:
        for name, g_, r_ in zip(("y", "dx", "dw", "db"), got, want):
            assert torch.equal(orc.widen(g_), r_), name
        return
    mag = _lin_all(_Orc, *[t.abs() for t in wide])
    for name, g_, r_, m_, n in zip(("y", "dx", "dw", "db"), got, want, mag,
                                   (K, ways, M, M)):
        _assert_bounded(g_, r_, m_, n, name)
