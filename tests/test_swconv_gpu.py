"""Wide-channel bf16 stride-2 conv trio (swconv.hip): 8-aligned channels with
max(C, F) in 65..256, reached through ``ops.task_conv3x3(..., stride=2)``.

Pattern and figures of tests/test_wconv_gpu.py: first order against the
exact-input float64 oracle (bf16 activations widened, weights rounded to bf16
as the repack rounds them; y, dx: one bf16 ulp + 1e-2; dw, db: fp32 figures),
the same shapes on small integers where every fp32 partial sum is exact and
the results must EQUAL the oracle (a dropped, doubled or mis-parity tap
shows), second order against ``ops.reference`` in fp32, bitwise
repeatability, and a 96-filter strided backbone against the CPU fp32 engine
with the thresholds of tests/test_strided_backbone_gpu.py."""

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

# (T, NB, H, W, C, F, pad): each the smallest reaching one failure mode
SHAPES = [
    (2, 3, 7, 7, 72, 72, 1),      # just past 64; ragged column tile; odd H: tap reads iy = H
    (2, 3, 12, 11, 128, 128, 0),  # one full column tile; p = 0, even H: input row 11 untouched
    (1, 2, 6, 5, 136, 256, 0),    # two column tiles, 2nd ragged on dgrad
    (1, 2, 5, 5, 256, 80, 1),     # C at the cap, C > F: a swapped repack fails
    (2, 5, 14, 14, 3, 128, 1),    # first layer via pad-to-8; dx sliced back to 3
    (1, 2, 3, 3, 96, 72, 0),      # Ho = Wo = 1: three parity classes with one tap row
    (2, 7, 21, 21, 72, 72, 1),    # Ho = 11, M = 847: ragged last row tile, unequal classes
    (1, 3, 60, 60, 72, 72, 1),    # wgrad: 2700 positions in 3 chunks of 928, last 844
]
BIG = (2, 7, 21, 21, 72, 72, 1)
FALLBACK = "grouped-ATen composition"


def dev():
    return torch.device("cuda", 0)


def _id(s):
    return "x".join(map(str, s))


def _mk(shape, integers=False):
    """(x bf16, w fp32, b fp32, dy bf16) on the CPU."""
    T, NB, H, W, C, F, pad = shape
    g = torch.Generator().manual_seed(sum(shape))
    Ho, Wo = (H + 2 * pad - 3) // 2 + 1, (W + 2 * pad - 3) // 2 + 1
    if integers:
        def ri(*s):
            return torch.randint(-3, 4, s, generator=g).float()
        x, w, b, dy = (ri(T, NB, H, W, C), ri(T, F, C, 3, 3) * 0.25, ri(T, F),
                       ri(T, NB, Ho, Wo, F))
    else:
        x, w, b, dy = (torch.randn(T, NB, H, W, C, generator=g),
                       torch.randn(T, F, C, 3, 3, generator=g).mul(0.1),
                       torch.randn(T, F, generator=g),
                       torch.randn(T, NB, Ho, Wo, F, generator=g))
    return x.to(torch.bfloat16), w, b, dy.to(torch.bfloat16)


def _both(shape, integers):
    """Kernel (y, dx, dw, db) and the float64 oracle's for the same inputs."""
    x, w, b, dy = _mk(shape, integers)
    pad = shape[-1]
    xg, wg, bg = (t.to(dev()).requires_grad_(True) for t in (x, w, b))
    y = ops.task_conv3x3(xg, wg, bg, stride=2, padding=pad)
    got = (y.detach(),) + torch.autograd.grad(y, (xg, wg, bg), dy.to(dev()))
    xo, wo, bo = (t.requires_grad_(True)
                  for t in (orc.widen(x), orc.round_bf16(w), orc.widen(b)))
    yo = orc.conv3x3(xo, wo, bo, 2, pad)
    want = (yo.detach(),) + torch.autograd.grad(yo, (xo, wo, bo), orc.widen(dy))
    return got, want


def test_wide_strided_conv_dispatches_to_the_kernels(monkeypatch):
    ext = ops.hip_ext()
    assert all(hasattr(ext, n) for n in ("swconv_fwd", "swconv_dgrad", "swconv_wgrad"))
    x, w, b, dy = _mk(SHAPES[0])
    monkeypatch.delenv("MAML355_SWCONV", raising=False)
    hip_autograd._FALLBACK_WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        xg, wg, bg = (t.to(dev()).requires_grad_(True) for t in (x, w, b))
        y = ops.task_conv3x3(xg, wg, bg, stride=2, padding=1)
        dx, dw, db = torch.autograd.grad(y, (xg, wg, bg), dy.to(dev()))
    assert not [r for r in rec if FALLBACK in str(r.message)]
    assert y.dtype == dx.dtype == torch.bfloat16
    assert dw.dtype == db.dtype == torch.float32

    # without a bias: the fallback rounds the convolution to bf16 BEFORE it
    # adds its bias (see the note in tests/test_wconv_gpu.py)
    yk = ops.task_conv3x3(x.to(dev()), w.to(dev()), None, stride=2, padding=1)
    monkeypatch.setenv("MAML355_SWCONV", "0")
    hip_autograd._FALLBACK_WARNED.clear()
    with pytest.warns(UserWarning, match="channels > 64"):
        y0 = ops.task_conv3x3(x.to(dev()), w.to(dev()), None, stride=2, padding=1)
    orc.assert_bf16_close(y0, orc.widen(yk), 1e-2, name="fallback y")


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_swconv_first_order_matches_oracle(shape):
    (y, dx, dw, db), (yo, dxo, dwo, dbo) = _both(shape, integers=False)
    assert y.dtype == torch.bfloat16 and dx.dtype == torch.bfloat16
    orc.assert_bf16_close(y, yo, 1e-2, name="y")
    orc.assert_bf16_close(dx, dxo, 1e-2, name="dx")
    orc.assert_f32_close(dw, dwo, "dw")
    orc.assert_f32_close(db, dbo, "db")
    if shape == (2, 3, 12, 11, 128, 128, 0):
        # no output touches input row 11; dx is allocated uninitialised
        assert dxo[..., 11, :, :].abs().max() == 0
        assert torch.equal(dx[..., 11, :, :], torch.zeros_like(dx[..., 11, :, :]))


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_swconv_exact_on_small_integers(shape):
    (y, dx, dw, db), (yo, dxo, dwo, dbo) = _both(shape, integers=True)
    assert torch.equal(y.cpu(), yo.to(torch.bfloat16))
    assert torch.equal(dx.cpu(), dxo.to(torch.bfloat16))
    assert torch.equal(dw.cpu(), dwo.float())
    assert torch.equal(db.cpu(), dbo.float())


def _close(a, r, rtol, atol_rel, floor=1.0):
    scale = r.abs().max().item()
    torch.testing.assert_close(a, r, rtol=rtol, atol=atol_rel * max(scale, floor))


def _inner_outer(opmod, x_, w_, b_, pad):
    """The inner step updates w AND b from their grads, so the outer
    backward reaches the wgrad Function with a grad for the fused db."""
    y = opmod.task_conv3x3(x_, w_, b_, stride=2, padding=pad)
    gw, gb = torch.autograd.grad((y.float() ** 2).mean(), (w_, b_),
                                 create_graph=True)
    y2 = opmod.task_conv3x3(x_, (w_ - 0.1 * gw).to(w_.dtype),
                            (b_ - 0.1 * gb).to(b_.dtype), stride=2, padding=pad)
    return torch.autograd.grad((y2.float() ** 2).mean(), (w_, b_))


def _through_input(opmod, x_, w_, pad):
    """create_graph through dgrad: _ConvDgradFn.backward (fwd + wgrad)."""
    y = opmod.task_conv3x3(x_, w_, None, stride=2, padding=pad)
    (gx,) = torch.autograd.grad((y.float() ** 2).mean(), (x_,), create_graph=True)
    return torch.autograd.grad((gx.float() ** 2).sum(), (x_, w_))


@pytest.mark.parametrize("shape", [(2, 2, 8, 8, 72, 136, 1),
                                   (2, 2, 10, 7, 136, 72, 0)], ids=_id)
def test_swconv_second_order(shape):
    x, w, b, _ = _mk(shape)
    pad = shape[-1]
    got = _inner_outer(ops, x.to(dev()), w.to(dev()).requires_grad_(True),
                       b.to(dev()).requires_grad_(True), pad)
    want = _inner_outer(ref, x.float(), w.clone().requires_grad_(True),
                        b.clone().requires_grad_(True), pad)
    got += _through_input(ops, x.to(dev()).requires_grad_(True),
                          w.to(dev()).requires_grad_(True), pad)
    want += _through_input(ref, x.float().requires_grad_(True),
                           w.clone().requires_grad_(True), pad)
    for a, r in zip(got, want):
        _close(a.float().cpu(), r, 8e-2, 5e-2, floor=1e-3)


@pytest.mark.parametrize("det", [None, "1"], ids=["default", "deterministic"])
def test_swconv_kernels_are_bitwise_repeatable(monkeypatch, det):
    if det is None:
        monkeypatch.delenv("MAML355_DETERMINISTIC", raising=False)
    else:
        monkeypatch.setenv("MAML355_DETERMINISTIC", det)
    x, w, b, dy = (t.to(dev()) for t in _mk(BIG))
    ext = ops.hip_ext()
    wp, wpf = ext.wconv_repack(w, False), ext.wconv_repack(w, True)
    y1, y2 = (ext.swconv_fwd(x, wp, b, 1) for _ in range(2))
    dx1, dx2 = (ext.swconv_dgrad(dy, wpf, 1, 21, 21) for _ in range(2))
    (dw1, db1), (dw2, db2) = (ext.swconv_wgrad(dy, x, 1, True) for _ in range(2))
    assert torch.equal(y1, y2) and torch.equal(dx1, dx2)
    assert torch.equal(dw1, dw2) and torch.equal(db1, db2)


# ---------------------------------------------------------------------------
# model level: the engine of tests/test_strided_backbone_gpu.py at 96 filters
# (max_pooling=False, 14x15 image, 3 stages, second order, bf16), against the
# CPU fp32 engine with that test's thresholds
# ---------------------------------------------------------------------------
def _engine_grad(device):
    args = get_args([
        "--batch_size", "2", "--num_classes_per_set", "3",
        "--num_samples_per_class", "2", "--num_target_samples", "2",
        "--image_height", "14", "--image_width", "15", "--image_channels", "1",
        "--cnn_num_filters", "96", "--num_stages", "3",
        "--number_of_training_steps_per_iter", "2", "--max_pooling", "False",
        "--second_order", "True", "--first_order_to_second_order_epoch", "-1",
        "--seed", "11", "--compute_dtype", "bf16", "--fp32_support_pass", "False",
    ])
    torch.manual_seed(0)
    model = MAMLFewShotClassifier(im_shape=(2, 1, 14, 15), device=device, args=args)
    assert not model.classifier.max_pooling
    g = torch.Generator().manual_seed(9)
    xs = torch.randn(2, 3, 2, 1, 14, 15, generator=g)
    xt = torch.randn(2, 3, 2, 1, 14, 15, generator=g)
    ys = torch.arange(3).view(1, 3, 1).expand(2, 3, 2).contiguous()
    losses, _ = model.train_forward_prop((xs, xt, ys, ys.clone()), epoch=1)
    grad = torch.autograd.grad(losses["loss"], model.classifier.theta)[0]
    return float(losses["loss"].detach()), grad.detach().float().cpu()


def test_wide_strided_backbone_kernels_close_to_cpu(monkeypatch):
    monkeypatch.delenv("MAML355_SWCONV", raising=False)
    loss_c, gc = _engine_grad(torch.device("cpu"))
    hip_autograd._FALLBACK_WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        loss_g, gg = _engine_grad(dev())
    assert not [r for r in rec if FALLBACK in str(r.message)]
    ops.disable_hip_kernels()
    try:
        loss_t, gt = _engine_grad(dev())
    finally:
        ops.enable_hip_kernels()
    rel_kernel = ((gg - gc).norm() / gc.norm()).item()
    rel_torch = ((gt - gc).norm() / gc.norm()).item()
    cos = torch.nn.functional.cosine_similarity(gg.flatten(), gc.flatten(),
                                                dim=0).item()
    print(f"96-filter strided backbone: loss cpu {loss_c:.6f} kernel {loss_g:.6f} "
          f"torch-bf16 {loss_t:.6f}; rel_kernel {rel_kernel:.4f} "
          f"rel_torch {rel_torch:.4f} cos {cos:.5f}")
    assert abs(loss_c - loss_g) < 3e-2
    assert cos > 0.95, f"cosine {cos:.5f}"
    assert rel_kernel <= 1.25 * rel_torch, (rel_kernel, rel_torch)
