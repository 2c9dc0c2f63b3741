"""Stride-1 conv trio (tconv.hip, dconv.hip) brought to the standard of
tests/test_sconv_gpu.py: odd / non-square / 1x1 sizes, pad 0, C != F, the
first-layer and scalar-staging routes, second order through an updated
bias and through the input, wgrad v2 in its w-tiled and NSUB=2 regimes,
the conv-epilogue BN statistics, and the linear head's fused bias grad.

First-order results are compared with the exact-input float64 oracle
(tests/_oracle.py): the oracle sees the bf16 activations and upstream grads
widened and the weights rounded to bf16 as the GEMM repack rounds them (not
rounded for dconv_fwd, which reads fp32 weights).  bf16 results: one bf16
ulp + 1e-2; fp32 results (dw, db, sums): rtol 1e-4, atol 1e-2.  Composed
second-order results round intermediates to bf16 and use the figures of
tests/test_sconv_gpu.py against ``ops.reference``."""

import pytest
import torch

pytestmark = pytest.mark.gpu

import _oracle as orc
from howtotrainyourmamlpytorch_amd import ops
from howtotrainyourmamlpytorch_amd.ops import hip_autograd
from howtotrainyourmamlpytorch_amd.ops import reference as ref

A_CONV = 1e-2


def dev():
    return torch.device("cuda", 0)


def _id(s):
    return "x".join(map(str, s))


def _mk(T, NS, H, W, C, F, pad, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, NS, H, W, C, generator=g).to(torch.bfloat16)
    w = torch.randn(T, F, C, 3, 3, generator=g).mul(0.1)
    b = torch.randn(T, F, generator=g)
    return x, w, b


def _mk_dy(T, NS, H, W, C, F, pad, seed=0):
    g = torch.Generator().manual_seed(seed + 1)
    return torch.randn(T, NS, H + 2 * pad - 2, W + 2 * pad - 2, F,
                       generator=g).to(torch.bfloat16)


def _close(a, r, rtol, atol_rel, floor=1.0):
    scale = r.abs().max().item()
    torch.testing.assert_close(a, r, rtol=rtol, atol=atol_rel * max(scale, floor))


def _oracle_grads(x, dy, pad, w=None, F=None):
    """(dx, dw, db) of the stride-1 conv for upstream dy in float64.  dw and
    db do not depend on w; dx uses the bf16-rounded w of the dgrad repack."""
    T, C = x.shape[0], x.shape[4]
    xo = orc.widen(x).requires_grad_(True)
    wo = (orc.round_bf16(w) if w is not None
          else torch.zeros(T, F, C, 3, 3, dtype=orc.F64)).requires_grad_(True)
    bo = torch.zeros(T, wo.shape[1], dtype=orc.F64, requires_grad=True)
    yo = orc.conv3x3(xo, wo, bo, 1, pad)
    return torch.autograd.grad(yo, (xo, wo, bo), orc.widen(dy))


# (T, NB, H, W, C, F, pad): each the smallest reaching one failure mode
SHAPES = [
    (2, 3, 11, 9, 48, 48, 1),    # odd, non-square
    (2, 3, 12, 11, 64, 64, 0),   # dgrad with pad' = 2
    (2, 3, 7, 7, 8, 8, 1),       # v2 at Ci = 8: K9 = 72, a mostly-zero 2nd K step
    (2, 3, 7, 7, 8, 16, 1),      # the dconv route at C = 8
    (2, 5, 14, 14, 1, 64, 1),    # first layer; dx runs v2 dgrad at Co = 1
    (2, 5, 14, 14, 3, 48, 1),    # ... and Co = 3
    (1, 2, 3, 3, 16, 32, 0),     # Ho = Wo = 1
    (3, 7, 21, 21, 48, 48, 1),   # M = 3087: thirteen 256-row tiles, ragged last
    (2, 3, 10, 10, 16, 48, 1),   # C != F: a swapped repack fails
    (2, 3, 9, 9, 5, 5, 1),       # scalar staging (C, F not multiples of 8)
]


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_tconv_fwd_and_first_order_match_oracle(shape):
    T, NB, H, W, C, F, pad = shape
    x, w, b = _mk(*shape, seed=sum(shape))
    dy = _mk_dy(*shape, seed=sum(shape))
    xg = x.to(dev()).requires_grad_(True)
    wg = w.to(dev()).requires_grad_(True)
    bg = b.to(dev()).requires_grad_(True)
    y = ops.task_conv3x3(xg, wg, bg, stride=1, padding=pad)
    dx, dw, db = torch.autograd.grad(y, (xg, wg, bg), dy.to(dev()))

    # dconv_fwd reads the fp32 weights unrounded; the GEMM kernels round
    w_fwd = orc.widen(w) if hip_autograd._dconv_ok(C, F) else orc.round_bf16(w)
    yo = orc.conv3x3(orc.widen(x), w_fwd, orc.widen(b), 1, pad)
    dxo, dwo, dbo = _oracle_grads(x, dy, pad, w=w)

    assert y.shape == yo.shape and y.dtype == torch.bfloat16
    assert dx.shape == x.shape and dx.dtype == torch.bfloat16
    assert dw.shape == w.shape and dw.dtype == torch.float32
    assert db.shape == b.shape and db.dtype == torch.float32
    orc.assert_bf16_close(y, yo, A_CONV, name="y")
    orc.assert_bf16_close(dx, dxo, A_CONV, name="dx")
    orc.assert_f32_close(dw, dwo, "dw")
    orc.assert_f32_close(db, dbo, "db")


# ---------------------------------------------------------------------------
# second order, as the inner loop does it
# ---------------------------------------------------------------------------
def _inner_outer(opmod, x_, w_, b_, stride, pad):
    """The inner step updates w AND b from their grads, so the outer
    backward reaches the wgrad Function with a grad for the fused db."""
    y = opmod.task_conv3x3(x_, w_, b_, stride=stride, padding=pad)
    loss = (y.float() ** 2).mean()
    gw, gb = torch.autograd.grad(loss, (w_, b_), create_graph=True)
    w2, b2 = w_ - 0.1 * gw, b_ - 0.1 * gb
    y2 = opmod.task_conv3x3(x_, w2.to(w_.dtype), b2.to(b_.dtype),
                            stride=stride, padding=pad)
    return torch.autograd.grad((y2.float() ** 2).mean(), (w_, b_))


@pytest.mark.parametrize("shape", [(2, 2, 8, 8, 48, 48, 1),
                                   (2, 2, 9, 7, 16, 32, 0)], ids=_id)
def test_tconv_second_order_with_updated_bias(shape):
    T, NB, H, W, C, F, pad = shape
    x, w, b = _mk(*shape, seed=3)
    wg = w.to(dev()).requires_grad_(True)
    bg = b.to(dev()).requires_grad_(True)
    gw, gb = _inner_outer(ops, x.to(dev()), wg, bg, 1, pad)
    wr = w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True)
    gwr, gbr = _inner_outer(ref, x.float(), wr, br, 1, pad)
    _close(gw.cpu(), gwr, 8e-2, 5e-2, floor=1e-3)
    _close(gb.cpu(), gbr, 8e-2, 5e-2, floor=1e-3)


def test_tconv_second_order_through_input():
    """create_graph through dgrad: the grad of ||dx||^2 w.r.t. x and w
    exercises _ConvDgradFn.backward (fwd + wgrad kernels)."""
    shape = (2, 2, 9, 8, 16, 32, 1)
    pad = shape[-1]
    x, w, _ = _mk(*shape, seed=9)

    def run(opmod, x_, w_):
        y = opmod.task_conv3x3(x_, w_, None, stride=1, padding=pad)
        (gx,) = torch.autograd.grad((y.float() ** 2).mean(), (x_,),
                                    create_graph=True)
        return torch.autograd.grad((gx.float() ** 2).sum(), (x_, w_))

    gx, gw = run(ops, x.to(dev()).requires_grad_(True),
                 w.to(dev()).requires_grad_(True))
    gxr, gwr = run(ref, x.float().requires_grad_(True),
                   w.clone().requires_grad_(True))
    _close(gx.float().cpu(), gxr, 8e-2, 5e-2, floor=1e-3)
    _close(gw.cpu(), gwr, 8e-2, 5e-2, floor=1e-3)


def test_linear_second_order_through_weight_and_bias_grads():
    """A loss on gw and gb: _LinWgradFn.backward with a grad for the fused
    bias gradient."""
    T, M, K, ways = 3, 17, 200, 5
    g = torch.Generator().manual_seed(21)
    x = torch.randn(T, M, K, generator=g).to(torch.bfloat16)
    w = torch.randn(T, ways, K, generator=g).mul(0.1)
    b = torch.randn(T, ways, generator=g)

    def run(opmod, x_, w_, b_):
        y = opmod.task_linear(x_, w_, b_)
        loss = (y.float() ** 2).mean()
        gw, gb = torch.autograd.grad(loss, (w_, b_), create_graph=True)
        return torch.autograd.grad((gw ** 2).sum() + (gb ** 2).sum(), (w_, b_))

    sw, sb = run(ops, x.to(dev()), w.to(dev()).requires_grad_(True),
                 b.to(dev()).requires_grad_(True))
    swr, sbr = run(ref, x.float(), w.clone().requires_grad_(True),
                   b.clone().requires_grad_(True))
    _close(sw.cpu(), swr, 8e-2, 5e-2, floor=1e-3)
    _close(sb.cpu(), sbr, 8e-2, 5e-2, floor=1e-3)


# ---------------------------------------------------------------------------
# wgrad v2 against the oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 2, 6, 84, 3, 48, 1),
                                   (1, 2, 6, 84, 48, 48, 1),
                                   (1, 2, 5, 70, 16, 32, 0)], ids=_id)
def test_wgrad_v2_w_tiled_transposes_match_oracle(shape):
    """Wo > 64 with Wo % 8 != 0: dyt_pad_kernel / xt_pad_kernel take a second
    64-wide w tile with a ragged end."""
    T, NB, H, W, C, F, pad = shape
    assert W + 2 * pad - 2 > 64 and (W + 2 * pad - 2) % 8 != 0
    x, _, _ = _mk(*shape, seed=sum(shape))
    dy = _mk_dy(*shape, seed=sum(shape))
    dw, db = ops.hip_ext().tconv_wgrad_v2(dy.to(dev()), x.to(dev()), pad, True)
    _, dwo, dbo = _oracle_grads(x, dy, pad, F=F)
    assert dw.shape == (T, F, C, 3, 3)
    orc.assert_f32_close(dw, dwo, "dw")
    orc.assert_f32_close(db, dbo, "db")


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "deterministic"])
@pytest.mark.parametrize("shape", [(2, 3, 14, 14, 8, 16, 1),     # 9C = 72
                                   (2, 3, 14, 14, 48, 48, 1)],   # 9C = 432
                         ids=_id)
def test_wgrad_v2_nsub2_forced_matches_oracle(shape, det, monkeypatch):
    """The NSUB=2 template (128 columns per block) with 9C not a multiple
    of 128: the last block's second sub-block is nearly empty (72) or
    ragged (432 = 3*128 + 48)."""
    T, NB, H, W, C, F, pad = shape
    monkeypatch.setenv("MAML355_WGRAD_NSUB", "2")
    if det:
        monkeypatch.setenv("MAML355_DETERMINISTIC", "1")
    else:
        monkeypatch.delenv("MAML355_DETERMINISTIC", raising=False)
    x, _, _ = _mk(*shape, seed=sum(shape))
    dy = _mk_dy(*shape, seed=sum(shape))
    ext = ops.hip_ext()
    dw, db = ext.tconv_wgrad_v2(dy.to(dev()), x.to(dev()), pad, True)
    _, dwo, dbo = _oracle_grads(x, dy, pad, F=F)
    orc.assert_f32_close(dw, dwo, "dw")
    orc.assert_f32_close(db, dbo, "db")
    if det:
        dw2, db2 = ext.tconv_wgrad_v2(dy.to(dev()), x.to(dev()), pad, True)
        assert (dw == dw2).all().item() and (db == db2).all().item()


def test_wgrad_v2_nsub2_natural_selection_matches_oracle(monkeypatch):
    """Kr = 2*256*256 = 131072 and 9C = 72 > 64: the launcher picks NSUB=2
    by itself, and ops.task_conv3x3 dispatches to v2 (>= 30000 positions).
    Measured on an MI355X at max|dw| = 1165: v1 max|err| 7.3e-4 to 1.0e-3
    (atomic order varies), v2 1.0e-3; db: v1 5.5e-4, v2 3.6e-4.

    At this reduction length the 1e-2 absolute figure (set for ~7000 terms)
    does not apply as such: the v1 kernel's own error against the oracle on
    the same inputs is measured first, bounded by the figure scaled with the
    square root of the length, and v2 is allowed four times v1's error."""
    for k in ("MAML355_WGRAD_NSUB", "MAML355_DETERMINISTIC", "MAML355_WGRAD_V2",
              "MAML355_DCONV_WGRAD"):
        monkeypatch.delenv(k, raising=False)
    shape = (1, 2, 256, 256, 8, 16, 1)
    T, NB, H, W, C, F, pad = shape
    x, w, b = _mk(*shape, seed=77)
    dy = _mk_dy(*shape, seed=77)
    wg = w.to(dev()).requires_grad_(True)
    bg = b.to(dev()).requires_grad_(True)
    y = ops.task_conv3x3(x.to(dev()), wg, bg, stride=1, padding=pad)
    dw, db = torch.autograd.grad(y, (wg, bg), dy.to(dev()))
    dw1, db1 = ops.hip_ext().tconv_wgrad(dy.to(dev()), x.to(dev()), pad, True)
    dw2, db2 = ops.hip_ext().tconv_wgrad_v2(dy.to(dev()), x.to(dev()), pad, True)
    _, dwo, dbo = _oracle_grads(x, dy, pad, F=F)

    def err(a, r):
        return (a.cpu().double() - r).abs().max().item()

    e1w, e1b = err(dw1, dwo), err(db1, dbo)
    e2w, e2b = err(dw, dwo), err(db, dbo)
    print(f"K=131072: v1 max|err| dw={e1w:.3e} db={e1b:.3e}; "
          f"v2 max|err| dw={e2w:.3e} db={e2b:.3e}; max|dw|={dwo.abs().max().item():.1f}")
    atol = orc.F32_ATOL * (NB * H * W / 7000.0) ** 0.5
    orc.assert_close(dw1, dwo, orc.F32_RTOL, atol, name="v1 dw")
    orc.assert_close(db1, dbo, orc.F32_RTOL, atol, name="v1 db")
    assert e2w <= 4 * e1w, (e2w, e1w)
    assert e2b <= 4 * max(e1b, e1w), (e2b, e1b)
    # the autograd route did land on v2 (atomics: equal to accumulation order)
    torch.testing.assert_close(dw, dw2, rtol=1e-4, atol=atol)


def test_wgrad_autograd_dispatch_to_v2_matches_oracle(monkeypatch):
    """32000 positions: past the 30000-position dispatch to v2, below the
    NSUB=2 threshold, Wo = 80 > 64."""
    for k in ("MAML355_WGRAD_NSUB", "MAML355_DETERMINISTIC", "MAML355_WGRAD_V2",
              "MAML355_DCONV_WGRAD"):
        monkeypatch.delenv(k, raising=False)
    shape = (1, 5, 80, 80, 8, 16, 1)
    T, NB, H, W, C, F, pad = shape
    x, w, b = _mk(*shape, seed=78)
    dy = _mk_dy(*shape, seed=78)
    wg = w.to(dev()).requires_grad_(True)
    bg = b.to(dev()).requires_grad_(True)
    y = ops.task_conv3x3(x.to(dev()), wg, bg, stride=1, padding=pad)
    dw, db = torch.autograd.grad(y, (wg, bg), dy.to(dev()))
    _, dwo, dbo = _oracle_grads(x, dy, pad, F=F)
    orc.assert_f32_close(dw, dwo, "dw")
    orc.assert_f32_close(db, dbo, "db")


# ---------------------------------------------------------------------------
# conv-epilogue BN statistics and the sums input of the fused BN+act+pool
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("v2", [False, True], ids=["v1", "v2"])
@pytest.mark.parametrize("shape", [(3, 7, 14, 14, 48, 48, 1),
                                   (2, 3, 11, 9, 16, 24, 1)], ids=_id)
def test_conv_epilogue_stats_feed_fused_bn(shape, v2):
    """with_stats=True of tconv_mm / tconv_mm_v2 and the ``sums`` input of the
    fused BN+act+pool.

    The pooled output with ``sums`` is NOT within one bf16 ulp + 1e-5 of the
    ``sums=None`` output, and a correct kernel cannot be: the epilogue sums
    are those of the unrounded conv output, ``sums=None`` measures the
    bf16-rounded one.  Measured on an MI355X, in units of that tolerance:
    kernel against kernel 6.32 (14x14, 48 channels) and 3.21 (11x9, 24
    channels); the float64 oracle evaluated with the two sets of statistics
    is itself 6.31 and 2.57 apart.  So each result is held to the bf16
    tolerance against its own oracle, and the two results against each other
    to the sum of both tolerances and the oracles' distance."""
    T, NB, H, W, C, F, pad = shape
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    M = NB * Ho * Wo
    ext = ops.hip_ext()
    x, w, b = _mk(*shape, seed=sum(shape))
    xg, wg, bg = x.to(dev()), w.to(dev()), b.to(dev())
    if v2:
        y, sums = ext.tconv_mm_v2(xg, ext.tconv_repack_v2(wg, False), bg, pad,
                                  Ho, Wo, F, True)
    else:
        y, sums = ext.tconv_mm(xg, ext.tconv_repack(wg, False), bg, pad,
                               Ho, Wo, True)
    # sums of the UNROUNDED output, bias included
    vo = orc.conv3x3(orc.widen(x), orc.round_bf16(w), orc.widen(b), 1, pad)
    want = torch.stack([vo.sum(dim=(1, 2, 3)), (vo ** 2).sum(dim=(1, 2, 3))], 1)
    assert sums.shape == (T, 2, F)
    orc.assert_f32_close(sums, want, "epilogue sums")

    g = torch.Generator().manual_seed(5)
    gamma = (torch.rand(F, generator=g) + 0.5).to(dev())
    beta = torch.randn(F, generator=g).to(dev())
    yp, mean, var = ops.task_bn_act_pool(y, gamma, beta, sums=sums)
    y0, mean0, var0 = ops.task_bn_act_pool(y, gamma, beta)

    # mean / var are the ones the sums imply (E[x^2] - mean^2 in fp32)
    s = orc.widen(sums)
    m_imp = s[:, 0] / M
    ex2 = s[:, 1] / M
    orc.assert_close(mean, m_imp, 1e-6, 1e-6, name="mean from sums")
    verr = (orc.widen(var) - (ex2 - m_imp ** 2)).abs()
    assert (verr <= 8 * 2.0 ** -24 * ex2).all().item(), verr.max().item()

    # the pooled output is the oracle's for those statistics ...
    a = torch.nn.functional.leaky_relu(
        (orc.widen(y) - m_imp.view(T, 1, 1, 1, F))
        * torch.rsqrt(ex2 - m_imp ** 2 + 1e-5).view(T, 1, 1, 1, F)
        * orc.widen(gamma) + orc.widen(beta), 0.01)
    o_sums = orc.pool2x2(a)[0]
    orc.assert_bf16_close(yp, o_sums, 1e-5, name="pooled (sums)")
    # ... and the sums=None result is the oracle's for the statistics of
    # the ROUNDED conv output, which is what that path measures
    o_none = orc.bn_act_pool(orc.widen(y), orc.widen(gamma), orc.widen(beta))[0]
    orc.assert_bf16_close(y0, o_none, 1e-5, name="pooled (sums=None)")
    # The two results against each other: each within the bf16 tolerance of
    # its oracle, the oracles apart by what the statistics differ.
    gap = (o_sums - o_none).abs()
    tol = orc.BF16_ULP * o_none.abs() + 1e-5
    err = (orc.widen(yp) - orc.widen(y0)).abs()
    print(f"sums vs sums=None: kernel max err/tol={(err / tol).max().item():.2f} "
          f"oracle max gap/tol={(gap / tol).max().item():.2f}")
    assert (err <= tol + orc.BF16_ULP * o_sums.abs() + 1e-5 + gap).all().item()

    # sums of the wrong size are ignored: the sums=None result exactly
    bad = torch.zeros(T, 2, F + 8, device=dev())
    yb, meanb, varb = ops.task_bn_act_pool(y, gamma, beta, sums=bad)
    assert (yb == y0).all().item()
    assert (meanb == mean0).all().item() and (varb == var0).all().item()
