"""Wide backbones' first layer (wdconv.hip): a bf16 image with C in {1, 3}
and no gradient into 8-aligned 65..256 filters, stride 1 and 2, reached
through ``ops.task_conv3x3`` and ``ops.prepare_conv_input``.

First order against the exact-input float64 oracle (tests/_oracle.py) with
the figures of tests/test_wconv_gpu.py: the oracle sees the bf16 image
widened and the weights rounded to bf16 as the repack rounds them; y one bf16
ulp + 1e-2, dw and db (fp32) rtol 1e-4, atol 1e-2.  The same shapes run on
small integers, where every partial sum is exact in fp32 and the results
must EQUAL the oracle: that catches a dropped, doubled or mis-ordered k.
Second order and the model level use tests/test_wconv_gpu.py's scenarios and
thresholds."""

import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

import _oracle as orc
from howtotrainyourmamlpytorch_amd import ops
from howtotrainyourmamlpytorch_amd.config import get_args
from howtotrainyourmamlpytorch_amd.meta.engine import MAMLFewShotClassifier
from howtotrainyourmamlpytorch_amd.ops import hip_autograd
from howtotrainyourmamlpytorch_amd.ops import reference as ref

# (T, NB, H, W, C, F, pad, stride): each the smallest reaching one failure mode
SHAPES = [
    (2, 3, 7, 7, 3, 72, 1, 1),      # just past 64, ragged last channel group
    (2, 5, 14, 14, 3, 128, 1, 1),
    (1, 2, 9, 8, 1, 96, 0, 1),      # C = 1, pad 0, non-square
    (1, 2, 5, 5, 3, 256, 1, 1),     # F at the cap
    (2, 3, 3, 3, 3, 80, 0, 1),      # Ho = Wo = 1
    (1, 7, 21, 20, 3, 72, 1, 1),    # 12 chunks of 13 lines crossing images, 2 per block
    (2, 3, 7, 7, 3, 72, 1, 2),      # odd H, last row reads iy = H
    (1, 2, 8, 8, 1, 96, 0, 2),      # even H, pad 0: an input row nobody reads
    (1, 5, 28, 28, 1, 128, 1, 2),
    (1, 3, 3, 3, 3, 80, 1, 2),
]
BIG = (1, 7, 21, 20, 3, 72, 1, 1)


def dev():
    return torch.device("cuda", 0)


def _id(s):
    return "x".join(map(str, s))


def _mk(shape, integers=False):
    """(x bf16, w fp32, b fp32, dy bf16) on the CPU."""
    T, NB, H, W, C, F, pad, s = shape
    g = torch.Generator().manual_seed(sum(shape))
    Ho, Wo = (H + 2 * pad - 3) // s + 1, (W + 2 * pad - 3) // s + 1
    if integers:
        def ri(*sz):
            return torch.randint(-3, 4, sz, generator=g).float()
        x, w, b, dy = (ri(T, NB, H, W, C), ri(T, F, C, 3, 3) * 0.25, ri(T, F),
                       ri(T, NB, Ho, Wo, F))
    else:
        x, w, b, dy = (torch.randn(T, NB, H, W, C, generator=g),
                       torch.randn(T, F, C, 3, 3, generator=g).mul(0.1),
                       torch.randn(T, F, generator=g),
                       torch.randn(T, NB, Ho, Wo, F, generator=g))
    return x.to(torch.bfloat16), w, b, dy.to(torch.bfloat16)


def _both(shape, integers):
    """Kernel (y, dw, db) and the float64 oracle's; the image has no grad."""
    x, w, b, dy = _mk(shape, integers)
    pad, s = shape[-2:]
    wg, bg = (t.to(dev()).requires_grad_(True) for t in (w, b))
    y = ops.task_conv3x3(x.to(dev()), wg, bg, stride=s, padding=pad)
    got = (y.detach(),) + torch.autograd.grad(y, (wg, bg), dy.to(dev()))
    wo, bo = (t.requires_grad_(True) for t in (orc.round_bf16(w), orc.widen(b)))
    yo = orc.conv3x3(orc.widen(x), wo, bo, s, pad)
    want = (yo.detach(),) + torch.autograd.grad(yo, (wo, bo), orc.widen(dy))
    return got, want


@pytest.fixture
def spy(monkeypatch):
    """Counts the calls of the new forward on the extension."""
    ext = ops.hip_ext()
    calls, real = [], ext.wdconv_fwd
    monkeypatch.setattr(ext, "wdconv_fwd",
                        lambda *a: calls.append(a[3:]) or real(*a))
    return calls


@pytest.mark.parametrize("stride", [1, 2])
def test_wide_first_layer_dispatches_to_wdconv(monkeypatch, spy, stride):
    for k in ("MAML355_WDCONV", "MAML355_WCONV", "MAML355_SWCONV",
              "MAML355_INPUT_PREP"):
        monkeypatch.delenv(k, raising=False)
    images = torch.randn(2, 3, 3, 9, 10).to(torch.bfloat16).to(dev())
    w = torch.randn(2, 96, 3, 3, 3).mul(0.1).to(dev()).requires_grad_(True)
    prepared = ops.prepare_conv_input(images, 96, stride=stride)
    assert isinstance(prepared, hip_autograd.PreparedInput)
    assert prepared.nhwc.shape == (2, 3, 9, 10, 3)
    assert prepared.xpad.shape == (2, 3, 9, 10, 8)
    hip_autograd._FALLBACK_WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        yk = ops.task_conv3x3(prepared.nhwc, w, None, stride=stride, padding=1,
                              xpad=prepared.xpad)
        (dw,) = torch.autograd.grad(yk, w, torch.ones_like(yk))
    assert not [r for r in rec if "grouped-ATen composition" in str(r.message)]
    assert spy == [(96, 1, stride)]
    assert yk.dtype == torch.bfloat16 and dw.shape == w.shape

    # A/B against the pad-to-8 route, without a bias (see test_wconv_gpu.py)
    monkeypatch.setenv("MAML355_WDCONV", "0")
    assert ops.prepare_conv_input(images, 96, stride=stride) is None
    y0 = ops.task_conv3x3(prepared.nhwc, w, None, stride=stride, padding=1)
    assert len(spy) == 1
    orc.assert_bf16_close(y0.detach(), orc.widen(yk.detach()), 1e-2,
                          name="pad-to-8 y")


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_wdconv_first_order_matches_oracle(shape, spy):
    (y, dw, db), (yo, dwo, dbo) = _both(shape, integers=False)
    assert len(spy) == 1 and y.dtype == torch.bfloat16
    orc.assert_bf16_close(y, yo, 1e-2, name="y")
    orc.assert_f32_close(dw, dwo, "dw")
    orc.assert_f32_close(db, dbo, "db")


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_wdconv_exact_on_small_integers(shape):
    (y, dw, db), (yo, dwo, dbo) = _both(shape, integers=True)
    assert torch.equal(y.cpu(), yo.to(torch.bfloat16))
    assert torch.equal(dw.cpu(), dwo.float())
    assert torch.equal(db.cpu(), dbo.float())


def _close(a, r, rtol, atol_rel, floor=1.0):
    scale = r.abs().max().item()
    torch.testing.assert_close(a, r, rtol=rtol, atol=atol_rel * max(scale, floor))


def _inner_outer(opmod, x_, w_, b_, pad, s):
    """The inner step updates w AND b from their grads, so the outer backward
    runs fwd on gw and reaches the wgrad Function with a grad for db."""
    y = opmod.task_conv3x3(x_, w_, b_, stride=s, padding=pad)
    gw, gb = torch.autograd.grad((y.float() ** 2).mean(), (w_, b_),
                                 create_graph=True)
    y2 = opmod.task_conv3x3(x_, (w_ - 0.1 * gw).to(w_.dtype),
                            (b_ - 0.1 * gb).to(b_.dtype), stride=s, padding=pad)
    return torch.autograd.grad((y2.float() ** 2).mean(), (w_, b_))


@pytest.mark.parametrize("shape", [(2, 2, 8, 8, 3, 136, 1, 1),
                                   (2, 2, 9, 7, 1, 72, 0, 2)], ids=_id)
def test_wdconv_second_order(shape, spy):
    x, w, b, _ = _mk(shape)
    pad, s = shape[-2:]
    got = _inner_outer(ops, x.to(dev()), w.to(dev()).requires_grad_(True),
                       b.to(dev()).requires_grad_(True), pad, s)
    want = _inner_outer(ref, x.float(), w.clone().requires_grad_(True),
                        b.clone().requires_grad_(True), pad, s)
    assert len(spy) == 3    # y, y2, and fwd on gw in the outer backward
    for a, r in zip(got, want):
        _close(a.float().cpu(), r, 8e-2, 5e-2, floor=1e-3)


def test_image_that_requires_grad_keeps_the_pad_route(spy):
    shape = (2, 3, 7, 7, 3, 72, 1, 1)
    x, w, b, dy = _mk(shape)
    xg, wg = (t.to(dev()).requires_grad_(True) for t in (x, w))
    y = ops.task_conv3x3(xg, wg, b.to(dev()), stride=1, padding=1)
    (dx,) = torch.autograd.grad(y, xg, dy.to(dev()))
    xo = orc.widen(x).requires_grad_(True)
    yo = orc.conv3x3(xo, orc.round_bf16(w), orc.widen(b), 1, 1)
    (dxo,) = torch.autograd.grad(yo, xo, orc.widen(dy))
    assert not spy
    orc.assert_bf16_close(dx, dxo, 1e-2, name="dx")


@pytest.mark.parametrize("W, fits", [(453, True), (454, False)])
def test_image_too_wide_for_the_lds_keeps_the_pad_route(spy, W, fits):
    """Three staged rows of (W + 2) * 3 elements fit the 4096-element buffer
    up to W = 453; past it the layer runs as before, on the pad-to-8 route."""
    shape = (1, 1, 3, W, 3, 72, 1, 1)
    images = torch.zeros(1, 1, 3, 3, W, dtype=torch.bfloat16, device=dev())
    assert (ops.prepare_conv_input(images, 72) is not None) == fits
    (y, dw, db), (yo, dwo, dbo) = _both(shape, integers=True)
    assert len(spy) == int(fits)
    assert torch.equal(y.cpu(), yo.to(torch.bfloat16))
    assert torch.equal(dw.cpu(), dwo.float())


def test_wdconv_is_bitwise_repeatable():
    x, w, b, _ = (t.to(dev()) for t in _mk(BIG))
    ext = ops.hip_ext()
    wp = ext.wdconv_repack(w)
    y1, y2 = (ext.wdconv_fwd(x, wp, b, 72, 1, 1) for _ in range(2))
    assert torch.equal(y1, y2)


# ---------------------------------------------------------------------------
# model level: tests/test_wconv_gpu.py's 96-filter, 3-stage, 14x15 second-order
# engine, pooled and strided, against the CPU fp32 engine at its thresholds
# ---------------------------------------------------------------------------
def _engine_grad(device, max_pooling):
    args = get_args([
        "--batch_size", "2", "--num_classes_per_set", "3",
        "--num_samples_per_class", "2", "--num_target_samples", "2",
        "--image_height", "14", "--image_width", "15", "--image_channels", "1",
        "--cnn_num_filters", "96", "--num_stages", "3",
        "--number_of_training_steps_per_iter", "2",
        "--max_pooling", str(max_pooling),
        "--second_order", "True", "--first_order_to_second_order_epoch", "-1",
        "--seed", "11", "--compute_dtype", "bf16", "--fp32_support_pass", "False",
    ])
    torch.manual_seed(0)
    model = MAMLFewShotClassifier(im_shape=(2, 1, 14, 15), device=device, args=args)
    assert model.classifier.max_pooling == max_pooling
    g = torch.Generator().manual_seed(9)
    xs = torch.randn(2, 3, 2, 1, 14, 15, generator=g)
    xt = torch.randn(2, 3, 2, 1, 14, 15, generator=g)
    ys = torch.arange(3).view(1, 3, 1).expand(2, 3, 2).contiguous()
    losses, _ = model.train_forward_prop((xs, xt, ys, ys.clone()), epoch=1)
    grad = torch.autograd.grad(losses["loss"], model.classifier.theta)[0]
    return float(losses["loss"].detach()), grad.detach().float().cpu()


@pytest.mark.parametrize("max_pooling", [True, False])
def test_wide_backbone_first_layer_close_to_cpu(monkeypatch, spy, max_pooling):
    for k in ("MAML355_WDCONV", "MAML355_WCONV", "MAML355_SWCONV"):
        monkeypatch.delenv(k, raising=False)
    loss_c, gc = _engine_grad(torch.device("cpu"), max_pooling)
    hip_autograd._FALLBACK_WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        loss_g, gg = _engine_grad(dev(), max_pooling)
    assert not [r for r in rec if "grouped-ATen composition" in str(r.message)]
    assert spy and all(c == (96, 1, 1 if max_pooling else 2) for c in spy)
    ops.disable_hip_kernels()
    try:
        loss_t, gt = _engine_grad(dev(), max_pooling)
    finally:
        ops.enable_hip_kernels()
    rel_kernel = ((gg - gc).norm() / gc.norm()).item()
    rel_torch = ((gt - gc).norm() / gc.norm()).item()
    cos = torch.nn.functional.cosine_similarity(gg.flatten(), gc.flatten(),
                                                dim=0).item()
    print(f"96-filter backbone (max_pooling={max_pooling}): loss cpu "
          f"{loss_c:.6f} kernel {loss_g:.6f} torch-bf16 {loss_t:.6f}; "
          f"rel_kernel {rel_kernel:.4f} rel_torch {rel_torch:.4f} cos {cos:.5f}")
    assert abs(loss_c - loss_g) < 3e-2
    assert cos > 0.95, f"cosine {cos:.5f}"
    assert rel_kernel <= 1.25 * rel_torch, (rel_kernel, rel_torch)
