"""GPU tests for the stride-2 MFMA conv trio (sconv.hip: fwd / parity
dgrad / wgrad) against the fp32 CPU reference, including the composed
double-backward paths of second-order MAML.  Tolerances are the stride-1
trio's (tests/test_tconv_gpu.py): K per output is the same 9*C."""

import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

from howtotrainyourmamlpytorch_amd import ops
from howtotrainyourmamlpytorch_amd.ops import hip_autograd
from howtotrainyourmamlpytorch_amd.ops import reference as ref


def dev():
    return torch.device("cuda", 0)


def _mk(T=2, NS=3, H=12, W=12, C=48, F=48, pad=1, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(T, NS, H, W, C, generator=g).to(dev(), torch.bfloat16)
    w = torch.randn(T, F, C, 3, 3, generator=g).mul(0.1).to(dev())
    b = torch.randn(T, F, generator=g).to(dev())
    return x, w, b


def _close(a, r, rtol, atol_rel, floor=1.0):
    scale = r.abs().max().item()
    torch.testing.assert_close(a, r, rtol=rtol, atol=atol_rel * max(scale, floor))


# (T, NB, H, W, C, F, pad): each the smallest reaching one failure mode
SHAPES = [
    (2, 3, 12, 12, 48, 48, 1),   # even size, baseline
    (2, 3, 11, 9, 48, 48, 1),    # odd, non-square: bottom/right tap reads iy = H
    (2, 3, 12, 11, 64, 64, 0),   # pad 0: input row 11 unused -> dx row == 0
    (2, 3, 7, 7, 8, 8, 1),       # one N tile, smallest vector channel count
    (2, 5, 14, 14, 1, 64, 1),    # first-layer channel counts
    (2, 5, 14, 14, 3, 48, 1),
    (1, 2, 3, 3, 16, 32, 0),     # Ho = Wo = 1, C != F
    (3, 7, 21, 21, 48, 48, 1),   # M = 847: several M tiles, ragged parities
    (2, 3, 10, 10, 16, 48, 1),   # C != F: a swapped repack fails
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sconv_fwd_and_first_order_match_reference(shape):
    T, NB, H, W, C, F, pad = shape
    x, w, b = _mk(T, NB, H, W, C, F, pad, seed=sum(shape))
    x.requires_grad_(True); w.requires_grad_(True); b.requires_grad_(True)
    y = ops.task_conv3x3(x, w, b, stride=2, padding=pad)

    xr = x.detach().float().cpu().requires_grad_(True)
    wr = w.detach().cpu().requires_grad_(True)
    br = b.detach().cpu().requires_grad_(True)
    yr = ref.task_conv3x3(xr, wr, br, stride=2, padding=pad)
    assert y.shape == yr.shape
    assert y.dtype == torch.bfloat16
    _close(y.detach().float().cpu(), yr.detach(), 3e-2, 3e-2)

    gout = torch.randn_like(y)
    dx, dw, db = torch.autograd.grad(y, (x, w, b), gout)
    dxr, dwr, dbr = torch.autograd.grad(yr, (xr, wr, br), gout.float().cpu())
    assert dx.shape == x.shape and dw.shape == w.shape and db.shape == b.shape
    assert dw.dtype == torch.float32 and db.dtype == torch.float32
    _close(dx.float().cpu(), dxr, 5e-2, 3e-2)
    _close(dw.cpu(), dwr, 5e-2, 3e-2)
    _close(db.cpu(), dbr, 5e-2, 3e-2)
    if pad == 0 and H % 2 == 0:
        # the trailing input row is touched by no output: exactly zero
        assert (dxr[:, :, H - 1] == 0).all().item()
        assert (dx[:, :, H - 1] == 0).all().item()


@pytest.mark.parametrize("shape", [(2, 2, 8, 8, 48, 48, 1),
                                   (2, 2, 9, 7, 48, 48, 0)],
                         ids=lambda s: "x".join(map(str, s)))
def test_sconv_second_order_matches_reference(shape):
    """The MAML pattern: grad of (a function of the first-order grads)."""
    T, NB, H, W, C, F, pad = shape
    x, w, b = _mk(T, NB, H, W, C, F, pad, seed=3)
    w.requires_grad_(True); b.requires_grad_(True)

    def inner_outer(opmod, x_, w_, b_):
        y = opmod.task_conv3x3(x_, w_, b_, stride=2, padding=pad)
        loss = (y.float() ** 2).mean()
        gw, = torch.autograd.grad(loss, (w_,), create_graph=True)
        w2 = w_ - 0.1 * gw
        y2 = opmod.task_conv3x3(x_, w2.to(w_.dtype), b_, stride=2, padding=pad)
        outer = (y2.float() ** 2).mean()
        return torch.autograd.grad(outer, (w_, b_))

    gw, gb = inner_outer(ops, x, w, b)
    xr = x.detach().float().cpu()
    wr = w.detach().cpu().requires_grad_(True)
    br = b.detach().cpu().requires_grad_(True)
    gwr, gbr = inner_outer(ref, xr, wr, br)
    for a, r in ((gw.cpu(), gwr), (gb.cpu(), gbr)):
        _close(a, r, 8e-2, 5e-2, floor=1e-3)


@pytest.mark.parametrize("shape", [(2, 2, 8, 8, 48, 48, 1),
                                   (2, 2, 9, 7, 16, 32, 0)],
                         ids=lambda s: "x".join(map(str, s)))
def test_sconv_second_order_with_updated_bias(shape):
    """As the inner loop does it: the inner step updates w AND b, so the
    outer backward reaches _SConvWgradFn.backward with a grad for the
    fused bias gradient (the ``gdb is not None`` branch)."""
    T, NB, H, W, C, F, pad = shape
    x, w, b = _mk(T, NB, H, W, C, F, pad, seed=4)
    w.requires_grad_(True); b.requires_grad_(True)

    def inner_outer(opmod, x_, w_, b_):
        y = opmod.task_conv3x3(x_, w_, b_, stride=2, padding=pad)
        loss = (y.float() ** 2).mean()
        gw, gb = torch.autograd.grad(loss, (w_, b_), create_graph=True)
        w2, b2 = w_ - 0.1 * gw, b_ - 0.1 * gb
        y2 = opmod.task_conv3x3(x_, w2.to(w_.dtype), b2.to(b_.dtype),
                                stride=2, padding=pad)
        outer = (y2.float() ** 2).mean()
        return torch.autograd.grad(outer, (w_, b_))

    gw, gb = inner_outer(ops, x, w, b)
    xr = x.detach().float().cpu()
    wr = w.detach().cpu().requires_grad_(True)
    br = b.detach().cpu().requires_grad_(True)
    gwr, gbr = inner_outer(ref, xr, wr, br)
    for a, r in ((gw.cpu(), gwr), (gb.cpu(), gbr)):
        _close(a, r, 8e-2, 5e-2, floor=1e-3)


def test_sconv_second_order_through_input():
    """create_graph through dgrad: the grad of ||dx||^2 w.r.t. w and the
    upstream grad exercises _SConvDgradFn.backward (fwd + wgrad kernels)."""
    T, NB, H, W, C, F, pad = 2, 2, 9, 8, 16, 32, 1
    x, w, _ = _mk(T, NB, H, W, C, F, pad, seed=9)
    x.requires_grad_(True); w.requires_grad_(True)

    def run(opmod, x_, w_):
        y = opmod.task_conv3x3(x_, w_, None, stride=2, padding=pad)
        (gx,) = torch.autograd.grad((y.float() ** 2).mean(), (x_,),
                                    create_graph=True)
        return torch.autograd.grad((gx.float() ** 2).sum(), (x_, w_))

    gx, gw = run(ops, x, w)
    xr = x.detach().float().cpu().requires_grad_(True)
    wr = w.detach().cpu().requires_grad_(True)
    gxr, gwr = run(ref, xr, wr)
    _close(gx.float().cpu(), gxr, 8e-2, 5e-2, floor=1e-3)
    _close(gw.cpu(), gwr, 8e-2, 5e-2, floor=1e-3)


def test_sconv_wgrad_k_split_and_deterministic(monkeypatch):
    """Reduction length 6*32*32 = 6144 (> one 4096 chunk): atomic fast path
    against the oracle; the deterministic path bitwise repeatable and equal
    to the fast path to accumulation-order tolerance."""
    monkeypatch.delenv("MAML355_DETERMINISTIC", raising=False)
    T, NB, H, W, C, F, pad = 2, 6, 64, 64, 48, 48, 1
    x, w, b = _mk(T, NB, H, W, C, F, pad, seed=5)
    w.requires_grad_(True); b.requires_grad_(True)
    y = ops.task_conv3x3(x, w, b, stride=2, padding=pad)
    assert y.shape[1] * y.shape[2] * y.shape[3] == 6144
    gout = torch.randn_like(y)
    dw, db = torch.autograd.grad(y, (w, b), gout)
    wr = w.detach().cpu().requires_grad_(True)
    br = b.detach().cpu().requires_grad_(True)
    yr = ref.task_conv3x3(x.float().cpu(), wr, br, stride=2, padding=pad)
    dwr, dbr = torch.autograd.grad(yr, (wr, br), gout.float().cpu())
    _close(dw.cpu(), dwr, 5e-2, 3e-2)
    _close(db.cpu(), dbr, 5e-2, 3e-2)

    ext = ops.hip_ext()
    dw_a, db_a = ext.sconv_wgrad(gout, x, pad, True)
    monkeypatch.setenv("MAML355_DETERMINISTIC", "1")
    dw_d, db_d = ext.sconv_wgrad(gout, x, pad, True)
    dw_d2, db_d2 = ext.sconv_wgrad(gout, x, pad, True)
    assert (dw_d == dw_d2).all().item()
    assert (db_d == db_d2).all().item()
    torch.testing.assert_close(dw_a, dw_d, rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(db_a, db_d, rtol=1e-4, atol=1e-3)


def test_stride2_runs_on_kernels_without_fallback_warning():
    ext = ops.hip_ext()
    assert hasattr(ext, "sconv_fwd") and hasattr(ext, "sconv_dgrad")
    assert hasattr(ext, "sconv_wgrad") and hasattr(ext, "sconv_repack")
    x, w, b = _mk()

    hip_autograd._FALLBACK_WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        ops.task_conv3x3(x, w, b, stride=2, padding=1)
        y, sums = ops.task_conv3x3(x, w, b, stride=2, padding=1,
                                   return_stats=True)
    assert not [r for r in rec if "grouped-ATen composition" in str(r.message)]
    assert sums is None or sums.numel() == 0

    # the fallback policy is unchanged: fp32 input still warns, loudly
    hip_autograd._FALLBACK_WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        ops.task_conv3x3(x.float(), w, b, stride=2, padding=1)
    assert [r for r in rec if "grouped-ATen composition" in str(r.message)]
    hip_autograd._FALLBACK_WARNED.clear()


def test_stride1_routing_unchanged_bitwise():
    """Regression guard: the stride-1 dispatch still lands on the v2 kernel
    with bit-identical output."""
    ext = ops.hip_ext()
    x, w, b = _mk()
    y = ops.task_conv3x3(x, w, b, stride=1, padding=1)
    wp = ext.tconv_repack_v2(w, False)
    y2 = ext.tconv_mm_v2(x, wp, b, 1, 12, 12, 48, False)[0]
    assert (y == y2).all().item()
