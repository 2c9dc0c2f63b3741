"""Transpose-free wgrad (wgrad_nt.hip, ``tconv_wgrad_v3``) against the exact-
input float64 oracle (tests/_oracle.py): fp32 results at rtol 1e-4, atol 1e-2
(``orc.assert_f32_close``), in the atomic mode and under
MAML355_DETERMINISTIC=1, where a second call must be bitwise equal.  The
index arithmetic the kernel runs on is walked on the CPU by
tests/test_wgrad_nt_addr.py; here the same shapes run on the GPU."""

import pytest
import torch

pytestmark = pytest.mark.gpu

import _oracle as orc
from howtotrainyourmamlpytorch_amd import ops
from howtotrainyourmamlpytorch_amd.ops import reference as ref

_ENV = ("MAML355_WGRAD_NSUB", "MAML355_DETERMINISTIC", "MAML355_WGRAD_V2",
        "MAML355_WGRAD_V3", "MAML355_DCONV_WGRAD")


def dev():
    return torch.device("cuda", 0)


def _id(s):
    return "x".join(map(str, s))


def _mk(T, NB, H, W, C, F, pad, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, NB, H, W, C, generator=g).to(torch.bfloat16)
    w = torch.randn(T, F, C, 3, 3, generator=g).mul(0.1)
    b = torch.randn(T, F, generator=g)
    dy = torch.randn(T, NB, H + 2 * pad - 2, W + 2 * pad - 2, F,
                     generator=g).to(torch.bfloat16)
    return x, w, b, dy


def _oracle_grads(x, dy, pad, F):
    """(dw, db) of the stride-1 conv for upstream dy in float64; neither
    depends on w."""
    T, C = x.shape[0], x.shape[4]
    xo = orc.widen(x)
    wo = torch.zeros(T, F, C, 3, 3, dtype=orc.F64, requires_grad=True)
    bo = torch.zeros(T, F, dtype=orc.F64, requires_grad=True)
    yo = orc.conv3x3(xo, wo, bo, 1, pad)
    return torch.autograd.grad(yo, (wo, bo), orc.widen(dy))


def _set_env(monkeypatch, det, nsub=None):
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    if det:
        monkeypatch.setenv("MAML355_DETERMINISTIC", "1")
    if nsub is not None:
        monkeypatch.setenv("MAML355_WGRAD_NSUB", str(nsub))


def _check(shape, det, with_bias=True):
    T, NB, H, W, C, F, pad = shape
    x, _, _, dy = _mk(*shape, seed=sum(shape))
    ext = ops.hip_ext()
    dyg, xg = dy.to(dev()), x.to(dev())
    dw, db = ext.tconv_wgrad_v3(dyg, xg, pad, with_bias)
    dwo, dbo = _oracle_grads(x, dy, pad, F)
    assert dw.shape == (T, F, C, 3, 3) and dw.dtype == torch.float32
    assert db.shape == (T, F) and db.dtype == torch.float32
    orc.assert_f32_close(dw, dwo, "dw")
    if with_bias:
        orc.assert_f32_close(db, dbo, "db")
    if det:
        dw2, db2 = ext.tconv_wgrad_v3(dyg, xg, pad, with_bias)
        assert (dw == dw2).all().item() and (db == db2).all().item()


# (T, NB, H, W, C, F, pad): each the smallest reaching one failure mode
SHAPES = [
    (2, 3, 11, 9, 48, 48, 1),    # odd, non-square; K = 297 ragged; 432 cols
    (2, 3, 12, 11, 64, 64, 0),   # pad 0; 9C = 576: column-sum bias; 4 m-tiles
    (2, 3, 7, 7, 8, 16, 1),      # tap changes every 8 columns
    (2, 3, 7, 7, 8, 8, 1),       # F below one 16-wide block
    (2, 5, 14, 14, 3, 48, 1),    # first layer: channel pad 3 -> 8
    (2, 5, 14, 14, 1, 64, 1),    # ... and 1 -> 8
    (1, 2, 3, 3, 16, 32, 0),     # Ho = Wo = 1: K = 2, under one read block
    (2, 3, 5, 5, 16, 16, 1),     # a 64-row tile spans 12 lines, crosses images
    (1, 2, 6, 84, 48, 48, 1),    # a tile shorter than one line, Wo % 8 != 0
    (3, 7, 21, 21, 48, 48, 1),   # many K-chunks per task, ragged last chunk
]


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "deterministic"])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_wgrad_v3_matches_oracle(shape, det, monkeypatch):
    _set_env(monkeypatch, det)
    _check(shape, det)


def test_wgrad_v3_without_bias(monkeypatch):
    _set_env(monkeypatch, False)
    _check((2, 3, 11, 9, 48, 48, 1), False, with_bias=False)


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "deterministic"])
@pytest.mark.parametrize("nsub", [1, 2])
@pytest.mark.parametrize("shape", [(2, 3, 14, 14, 48, 48, 1),    # 9C = 432
                                   (2, 3, 14, 14, 8, 16, 1),     # 9C = 72
                                   (2, 5, 14, 14, 3, 48, 1)],    # padded C
                         ids=_id)
def test_wgrad_v3_forced_block_width(shape, nsub, det, monkeypatch):
    """128-column blocks (NSUB=2) with a ragged last block (432 = 3*128 + 48)
    or a nearly empty second half (72), and 64-column blocks on the same.
    The launcher's own choice depends on T * K and is 64 columns at every
    shape of this file; the first layer at workload size runs 128."""
    _set_env(monkeypatch, det, nsub=nsub)
    _check(shape, det)


@pytest.mark.parametrize("shape", [
    (3, 7, 21, 21, 48, 48, 1),     # below 30 000 positions: v1's sums
    (2, 5, 14, 14, 3, 48, 1),      # ... first layer (v1 stages C = 3 scalar)
    (2, 3, 12, 11, 64, 64, 0),     # ... 9C = 576, F = 64
    (1, 2, 126, 126, 8, 16, 1),    # 31 752 positions, Wo % 8 != 0: v2's sums
    (1, 5, 80, 80, 3, 48, 1),      # 32 000 positions, first layer: v2's sums
], ids=_id)
def test_wgrad_v3_deterministic_keeps_the_old_routings_bits(shape, monkeypatch):
    """Under MAML355_DETERMINISTIC=1 v3 performs the fp32 operations of the
    routing it replaces — v2 from 30 000 positions up (reduction index with
    lines padded to 8, v2's K-chunks), v1 below — so dw and db are bitwise
    what the parent computed, and a deterministic run of a whole workload
    does not move."""
    _set_env(monkeypatch, True)
    T, NB, H, W, C, F, pad = shape
    x, _, _, dy = _mk(*shape, seed=sum(shape))
    ext = ops.hip_ext()
    dyg, xg = dy.to(dev()), x.to(dev())
    dw3, db3 = ext.tconv_wgrad_v3(dyg, xg, pad, True)
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    old = ext.tconv_wgrad_v2 if NB * Ho * Wo >= 30000 else ext.tconv_wgrad
    dwo, dbo = old(dyg, xg, pad, True)
    assert (dw3 == dwo).all().item(), (dw3 - dwo).abs().max().item()
    assert (db3 == dbo).all().item(), (db3 - dbo).abs().max().item()


def test_wgrad_dispatch(monkeypatch):
    """A supported shape reaches v3 through autograd (bitwise, deterministic
    mode); an unsupported one (C = F = 5) still takes the old route."""
    _set_env(monkeypatch, True)
    shape = (2, 3, 11, 9, 48, 48, 1)
    pad = shape[-1]
    x, w, b, dy = _mk(*shape, seed=5)
    wg = w.to(dev()).requires_grad_(True)
    bg = b.to(dev()).requires_grad_(True)
    y = ops.task_conv3x3(x.to(dev()), wg, bg, stride=1, padding=pad)
    dw, db = torch.autograd.grad(y, (wg, bg), dy.to(dev()))
    dw3, db3 = ops.hip_ext().tconv_wgrad_v3(dy.to(dev()), x.to(dev()), pad, True)
    assert (dw == dw3).all().item() and (db == db3).all().item()

    shape = (2, 3, 9, 9, 5, 5, 1)
    T, NB, H, W, C, F, pad = shape
    x, w, b, dy = _mk(*shape, seed=6)
    wg = w.to(dev()).requires_grad_(True)
    bg = b.to(dev()).requires_grad_(True)
    y = ops.task_conv3x3(x.to(dev()), wg, bg, stride=1, padding=pad)
    dw, db = torch.autograd.grad(y, (wg, bg), dy.to(dev()))
    dwo, dbo = _oracle_grads(x, dy, pad, F)
    orc.assert_f32_close(dw, dwo, "dw")
    orc.assert_f32_close(db, dbo, "db")
    with pytest.raises(RuntimeError):
        ops.hip_ext().tconv_wgrad_v3(dy.to(dev()), x.to(dev()), pad, True)


def _inner_outer(opmod, x_, w_, b_, pad):
    """The inner step updates w AND b from their grads, so the outer
    backward reaches the wgrad Function with a grad for the fused db."""
    y = opmod.task_conv3x3(x_, w_, b_, stride=1, padding=pad)
    loss = (y.float() ** 2).mean()
    gw, gb = torch.autograd.grad(loss, (w_, b_), create_graph=True)
    w2, b2 = w_ - 0.1 * gw, b_ - 0.1 * gb
    y2 = opmod.task_conv3x3(x_, w2.to(w_.dtype), b2.to(b_.dtype),
                            stride=1, padding=pad)
    return torch.autograd.grad((y2.float() ** 2).mean(), (w_, b_))


def _close(a, r, rtol, atol_rel, floor=1.0):
    scale = r.abs().max().item()
    torch.testing.assert_close(a, r, rtol=rtol, atol=atol_rel * max(scale, floor))


def test_wgrad_v3_second_order(monkeypatch):
    """Second order through the default routing (v3 for wgrad), with the
    tolerances tests/test_tconv_shapes_gpu.py uses for this composition."""
    _set_env(monkeypatch, False)
    shape = (2, 2, 8, 8, 48, 48, 1)
    pad = shape[-1]
    x, w, b, _ = _mk(*shape, seed=3)
    wg = w.to(dev()).requires_grad_(True)
    bg = b.to(dev()).requires_grad_(True)
    gw, gb = _inner_outer(ops, x.to(dev()), wg, bg, pad)
    wr = w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True)
    gwr, gbr = _inner_outer(ref, x.float(), wr, br, pad)
    _close(gw.cpu(), gwr, 8e-2, 5e-2, floor=1e-3)
    _close(gb.cpu(), gbr, 8e-2, 5e-2, floor=1e-3)
