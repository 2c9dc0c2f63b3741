"""Wide-channel fp32 conv trio (wfconv.hip): stride 1, any C and F in 1..256
with max(C, F) > 64, reached through ``ops.task_conv3x3``.

The checks are tests/test_fconv_gpu.py's at wide channels.  First order is
held to the DERIVED bound against the exact-input float64 oracle
(tests/_oracle.py): an n-term fp32 chain in any order, split sums included,
satisfies |err| <= (n + 2) * 2^-24 * sum |a||b|, with sum |a||b| from the
oracle on absolute values and n = 9C + 1 (y), 9F (dx), NB*Ho*Wo (dw, db); the
bound does not loosen with width.  The same shapes run on small integers,
where every partial sum is exact in fp32 (at C = 256 |y| <= 9*256*9 quarter
units, far below 2^24) and the results must EQUAL the oracle.  Second order
is compared with the same composition on the float64 oracle ops at that
file's fp32 figures, rtol 1e-4 and atol 1e-5 * max|ref|."""

import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

import _oracle as orc
from howtotrainyourmamlpytorch_amd import ops
from howtotrainyourmamlpytorch_amd.config import get_args
from howtotrainyourmamlpytorch_amd.meta.engine import MAMLFewShotClassifier
from howtotrainyourmamlpytorch_amd.ops import hip_autograd

EPS = 2.0 ** -24

# (T, NB, H, W, C, F, pad): each the smallest reaching one failure mode
SHAPES = [
    (2, 3, 7, 7, 72, 72, 1),      # just past 64; ragged column tile; K9 = 648: K tail
    (2, 3, 9, 8, 128, 128, 1),    # one full 128-column block; non-square
    (1, 2, 6, 5, 136, 256, 0),    # two column blocks; dgrad 2 x 80, 2nd ragged; pad' = 2
    (1, 2, 5, 5, 256, 80, 1),     # C at the cap, C > F: a swapped repack fails
    (2, 5, 14, 14, 3, 96, 1),     # first layer: scalar gather, one K-step, dgrad Co = 3
    (2, 5, 14, 14, 1, 72, 1),     # ... and Co = 1
    (1, 2, 3, 3, 96, 72, 0),      # Ho = Wo = 1
    (1, 2, 6, 6, 70, 66, 1),      # nothing 4-aligned at wide channels
    (2, 7, 21, 21, 72, 72, 1),    # M = 3087: many row tiles, ragged last
    (1, 3, 30, 30, 72, 72, 1),    # wgrad: 3 chunks of 928, the last 844 long
]
BIG = (2, 7, 21, 21, 72, 72, 1)
SECOND = [(2, 2, 8, 8, 72, 136, 1), (2, 2, 9, 7, 136, 72, 0)]


def dev():
    return torch.device("cuda", 0)


def _id(s):
    return "x".join(map(str, s))


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


def _fallback_warnings(rec):
    return [r for r in rec if "grouped-ATen composition" in str(r.message)]


# ---------------------------------------------------------------------------
# 1. dispatch
# ---------------------------------------------------------------------------
def test_wide_fp32_dispatch_reaches_the_kernels(monkeypatch):
    monkeypatch.delenv("MAML355_WFCONV", raising=False)
    monkeypatch.delenv("MAML355_FCONV", raising=False)
    x, w, b, dy = _mk(SHAPES[0], False)
    hip_autograd._FALLBACK_WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        y, dx, dw, db = _kernel_all(x, w, b, dy, 1)
    assert not _fallback_warnings(rec)
    for t in (y, dx, dw, db):
        assert t.dtype == torch.float32

    monkeypatch.setenv("MAML355_WFCONV", "0")
    hip_autograd._FALLBACK_WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        y0 = ops.task_conv3x3(x.to(dev()), w.to(dev()), b.to(dev()),
                              stride=1, padding=1)
    assert _fallback_warnings(rec)
    torch.testing.assert_close(y0, y, rtol=1e-4, atol=1e-4)
    hip_autograd._FALLBACK_WARNED.clear()


def test_wide_fp32_return_stats_yields_empty_sums():
    x, w, b, _ = _mk(SHAPES[0], False)
    y, sums = ops.task_conv3x3(x.to(dev()), w.to(dev()), b.to(dev()),
                               stride=1, padding=1, return_stats=True)
    assert y.dtype == torch.float32 and sums.numel() == 0


def test_wgrad_plan_cuts_three_chunks_with_a_ragged_last():
    assert list(ops.hip_ext().wfconv_wgrad_plan(1, 3, 30, 30, 72, 72)) == [928, 3]


# ---------------------------------------------------------------------------
# 2. first order under the derived bound; 3. exact integers
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_wfconv_first_order_within_derived_bound(shape):
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
def test_wfconv_exact_on_small_integers(shape):
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
    """A loss on y differentiated through x: fwd's backward under
    create_graph, then the dgrad Function's own backward (fwd + wgrad)."""
    y = opmod.task_conv3x3(x_, w_, None, stride=1, padding=pad)
    (gx,) = torch.autograd.grad((y ** 2).mean(), (x_,), create_graph=True)
    return torch.autograd.grad((gx ** 2).sum(), (x_, w_))


def _through_dgrad(opmod, x_, w_, pad):
    """A loss on gw differentiated through x and w: the wgrad Function's
    backward (fwd + dgrad) on top of the dgrad of the first backward."""
    y = opmod.task_conv3x3(x_, w_, None, stride=1, padding=pad)
    (gw,) = torch.autograd.grad((y ** 2).mean(), (w_,), create_graph=True)
    return torch.autograd.grad((gw ** 2).sum(), (x_, w_))


@pytest.mark.parametrize("shape", SECOND, ids=_id)
def test_wfconv_second_order_with_updated_bias(shape):
    pad = shape[-1]
    x, w, b, _ = _mk(shape, False)
    gw, gb = _inner_outer(ops, x.to(dev()), w.to(dev()).requires_grad_(True),
                          b.to(dev()).requires_grad_(True), pad)
    gwo, gbo = _inner_outer(_Orc, orc.widen(x), orc.widen(w).requires_grad_(True),
                            orc.widen(b).requires_grad_(True), pad)
    assert gw.dtype == torch.float32 and gb.dtype == torch.float32
    _close2(gw, gwo, "outer gw")
    _close2(gb, gbo, "outer gb")


@pytest.mark.parametrize("scenario", [_through_input, _through_dgrad],
                         ids=["input", "dgrad"])
@pytest.mark.parametrize("shape", SECOND, ids=_id)
def test_wfconv_second_order_through(shape, scenario):
    pad = shape[-1]
    x, w, _, _ = _mk(shape, False)
    gx, gw = scenario(ops, x.to(dev()).requires_grad_(True),
                      w.to(dev()).requires_grad_(True), pad)
    gxo, gwo = scenario(_Orc, orc.widen(x).requires_grad_(True),
                        orc.widen(w).requires_grad_(True), pad)
    _close2(gx, gxo, "gx")
    _close2(gw, gwo, "gw")


# ---------------------------------------------------------------------------
# 5. repeatability, without MAML355_DETERMINISTIC
# ---------------------------------------------------------------------------
def test_wfconv_kernels_bitwise_repeatable(monkeypatch):
    monkeypatch.delenv("MAML355_DETERMINISTIC", raising=False)
    x, w, b, dy = (t.to(dev()) for t in _mk(BIG, False))
    ext = ops.hip_ext()
    wp = ext.fconv_repack(w, False)
    y1, y2 = (ext.wfconv_mm(x, wp, b, 1, 21, 21) for _ in range(2))
    assert torch.equal(y1, y2)
    (dw1, db1), (dw2, db2) = (ext.wfconv_wgrad(dy, x, 1, True) for _ in range(2))
    assert torch.equal(dw1, dw2) and torch.equal(db1, db2)


# ---------------------------------------------------------------------------
# 6. model level: the 96-filter, 3-stage, 14x15 engine of
# tests/test_wconv_gpu.py in fp32, second order
# ---------------------------------------------------------------------------
def _engine_args(h, w, *more):
    return get_args([
        "--batch_size", "2", "--num_classes_per_set", "3",
        "--num_samples_per_class", "2", "--num_target_samples", "2",
        "--image_height", str(h), "--image_width", str(w),
        "--image_channels", "1", "--cnn_num_filters", "96", "--num_stages", "3",
        "--number_of_training_steps_per_iter", "2",
        "--second_order", "True", "--first_order_to_second_order_epoch", "-1",
        "--seed", "11", *more])


def _episode(h, w):
    g = torch.Generator().manual_seed(9)
    xs = torch.randn(2, 3, 2, 1, h, w, generator=g)
    xt = torch.randn(2, 3, 2, 1, h, w, generator=g)
    ys = torch.arange(3).view(1, 3, 1).expand(2, 3, 2).contiguous()
    return xs, xt, ys, ys.clone()


def _engine_grad(device):
    args = _engine_args(14, 15, "--compute_dtype", "fp32",
                        "--fp32_support_pass", "False")
    torch.manual_seed(0)
    model = MAMLFewShotClassifier(im_shape=(2, 1, 14, 15), device=device, args=args)
    losses, _ = model.train_forward_prop(_episode(14, 15), epoch=1)
    grad = torch.autograd.grad(losses["loss"], model.classifier.theta)[0]
    return float(losses["loss"].detach()), grad.detach().float().cpu()


def test_wide_fp32_backbone_kernels_close_to_cpu(monkeypatch):
    """Measured on an MI355X: loss cpu 2.8302569, kernel 2.8302584, fallback
    2.8302584; theta-gradient rel-L2 against the CPU 5.10e-06 on the kernels
    and 4.40e-06 on the grouped-ATen fallback (ratio 1.16).  With one serial
    accumulation chain per output and per bias-gradient column the kernels
    measured 9.26e-06; the chains are now closed every 256 terms."""
    monkeypatch.delenv("MAML355_WFCONV", raising=False)
    loss_c, gc = _engine_grad(torch.device("cpu"))
    hip_autograd._FALLBACK_WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        loss_g, gg = _engine_grad(dev())
    assert not _fallback_warnings(rec)
    monkeypatch.setenv("MAML355_WFCONV", "0")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loss_f, gf = _engine_grad(dev())
    hip_autograd._FALLBACK_WARNED.clear()
    rel_kernel = ((gg - gc).norm() / gc.norm()).item()
    rel_fallback = ((gf - gc).norm() / gc.norm()).item()
    print(f"96-filter fp32 backbone: loss cpu {loss_c:.7f} kernel {loss_g:.7f} "
          f"fallback {loss_f:.7f}; rel_kernel {rel_kernel:.3e} "
          f"rel_fallback {rel_fallback:.3e}")
    assert abs(loss_c - loss_g) < 1e-4
    assert rel_kernel <= 1.25 * rel_fallback, (rel_kernel, rel_fallback)


def _train_theta():
    args = _engine_args(28, 28, "--compute_dtype", "bf16",
                        "--fp32_support_pass", "True")
    torch.manual_seed(0)
    model = MAMLFewShotClassifier(im_shape=(2, 1, 28, 28), device=dev(), args=args)
    batch = tuple(t.to(dev()) for t in _episode(28, 28))
    for _ in range(3):
        model.run_train_iter(batch, epoch=0)
    return model.classifier.theta.detach().clone()


def test_fp32_support_pass_at_96_filters_is_bitwise_repeatable(monkeypatch):
    monkeypatch.delenv("MAML355_WFCONV", raising=False)
    monkeypatch.setenv("MAML355_DETERMINISTIC", "1")
    hip_autograd._FALLBACK_WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        a, b = _train_theta(), _train_theta()
    assert not _fallback_warnings(rec)
    assert torch.equal(a, b)
