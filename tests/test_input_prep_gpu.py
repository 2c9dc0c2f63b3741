"""The first layer's input prepared once (``conv_input_prep``): the NHWC
tensor must be the permute-copy the classifier made at every call, the
8-channel tensor must be what ``nt_chpad8_kernel`` makes of it inside
``tconv_wgrad_v3``, and wgrad v3 fed the pre-padded tensor must give the
bits it gives when it pads for itself.  All comparisons are ``torch.equal``:
the kernels only move values.

Grid: C in {1, 3} x (H, W) in {(5, 7), (8, 8)} (odd and even extents, a row
count that is no multiple of anything), T = 2, NS = 3."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from howtotrainyourmamlpytorch_amd import ops
from howtotrainyourmamlpytorch_amd.ops import hip_autograd

T, NS, F = 2, 3, 16
GRID = [(c, h, w) for c in (1, 3) for (h, w) in ((5, 7), (8, 8))]


def dev():
    return torch.device("cuda", 0)


def _id(s):
    return "x".join(map(str, s))


def _images(C, H, W):
    g = torch.Generator().manual_seed(100 * C + 10 * H + W)
    return torch.randn(T, NS, C, H, W, generator=g).to(torch.bfloat16).to(dev())


@pytest.mark.parametrize("chw", GRID, ids=_id)
def test_layouts(chw):
    C, H, W = chw
    x = _images(C, H, W)
    ext = ops.hip_ext()
    nhwc, xpad = ext.conv_input_prep(x)
    want = x.permute(0, 1, 3, 4, 2).contiguous()
    assert nhwc.shape == (T, NS, H, W, C) and nhwc.dtype == torch.bfloat16
    assert nhwc.is_contiguous() and xpad.is_contiguous()
    assert torch.equal(nhwc, want)
    want_pad = ext.tconv_chpad8(want)
    assert xpad.shape == want_pad.shape == (T, NS, H, W, 8)
    # bit patterns: the pad lanes are +0.0, the rest the image's own bits
    assert torch.equal(xpad.view(torch.int16), want_pad.view(torch.int16))
    assert torch.equal(xpad[..., :C], want) and not xpad[..., C:].any()


@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("chw", GRID, ids=_id)
def test_wgrad_v3_prepadded(monkeypatch, chw, pad):
    C, H, W = chw
    monkeypatch.setenv("MAML355_DETERMINISTIC", "1")
    for k in ("MAML355_WGRAD_NSUB", "MAML355_WGRAD_V2", "MAML355_WGRAD_V3"):
        monkeypatch.delenv(k, raising=False)
    x = _images(C, H, W)
    ext = ops.hip_ext()
    nhwc, xpad = ext.conv_input_prep(x)
    g = torch.Generator().manual_seed(7)
    dy = torch.randn(T, NS, H + 2 * pad - 2, W + 2 * pad - 2, F,
                     generator=g).to(torch.bfloat16).to(dev())
    dw0, db0 = ext.tconv_wgrad_v3(dy, nhwc, pad, True)
    dw1, db1 = ext.tconv_wgrad_v3(dy, nhwc, pad, True, xpad)
    assert dw0.abs().max().item() > 0
    assert torch.equal(dw0, dw1) and torch.equal(db0, db1)


@pytest.mark.parametrize("chw", GRID, ids=_id)
def test_conv_layer_uses_prepared_pair(monkeypatch, chw):
    """Through ops.task_conv3x3 at both derivative orders: the prepared pair
    reaches wgrad v3 (no pad pass runs), and y, dw, db and the second-order
    gradient keep their bits."""
    C, H, W = chw
    monkeypatch.setenv("MAML355_DETERMINISTIC", "1")
    for k in ("MAML355_INPUT_PREP", "MAML355_NO_DCONV", "MAML355_WGRAD_V3",
              "MAML355_DCONV_WGRAD"):
        monkeypatch.delenv(k, raising=False)
    x = _images(C, H, W)
    g = torch.Generator().manual_seed(5)
    w = torch.randn(T, F, C, 3, 3, generator=g).mul(0.2).to(dev())
    b = torch.randn(T, F, generator=g).to(dev())

    ext = ops.hip_ext()
    pads = []
    real = ext.tconv_wgrad_v3

    def spy(dy, xx, p, wb, xpad=None):
        pads.append(xpad is not None)
        return real(dy, xx, p, wb, xpad)
    monkeypatch.setattr(ext, "tconv_wgrad_v3", spy)

    def run(prepared):
        wg, bg = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        if prepared is None:
            y = ops.task_conv3x3(x.permute(0, 1, 3, 4, 2), wg, bg, 1, 1)
        else:
            y = ops.task_conv3x3(prepared.nhwc, wg, bg, 1, 1,
                                 xpad=prepared.xpad)
        dw, db = torch.autograd.grad((y.float() ** 2).sum(), (wg, bg),
                                     create_graph=True)
        d2w, = torch.autograd.grad((dw ** 2).sum() + (db ** 2).sum(), wg)
        return [t.detach() for t in (y, dw, db, d2w)]

    monkeypatch.setenv("MAML355_INPUT_PREP", "0")
    assert ops.prepare_conv_input(x, F) is None
    want = run(None)
    assert pads and not any(pads)
    del pads[:]
    monkeypatch.delenv("MAML355_INPUT_PREP")
    prepared = ops.prepare_conv_input(x, F)
    assert isinstance(prepared, hip_autograd.PreparedInput)
    got = run(prepared)
    assert pads and all(pads), "a wgrad call padded the input itself"
    for name, a, c in zip(("y", "dw", "db", "d2w"), want, got):
        assert torch.equal(a, c), name


def test_not_prepared_elsewhere():
    """Paths without the kernels take their input as before."""
    x = _images(3, 8, 8)
    assert ops.prepare_conv_input(x.float(), F) is None          # fp32
    assert ops.prepare_conv_input(x, F, stride=2) is None        # stride 2
    assert ops.prepare_conv_input(x.cpu(), F) is None            # CPU
    assert ops.prepare_conv_input(x, 24) is None                 # no dconv F
    x8 = torch.zeros(T, NS, 8, 8, 8, dtype=torch.bfloat16, device=dev())
    assert ops.prepare_conv_input(x8, F) is None                 # C = 8
