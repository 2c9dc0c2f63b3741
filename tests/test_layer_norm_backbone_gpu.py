"""End-to-end GPU check of the layer-norm backbone: conv + LayerNorm with
its learnable elementwise bias + leaky-ReLU (+ max pool, or stride-2 convs
and the global average pool) + linear head, second order, entirely on the
HIP kernels.  Image 14x15, 8 filters, 3 stages: the layer norm sees
14x15x8, 7x7x8, 3x3x8 with max pooling and 7x8x8, 4x4x8, 2x2x8 without
(even, odd and non-square sizes)."""

import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

from howtotrainyourmamlpytorch_amd import ops
from howtotrainyourmamlpytorch_amd.config import get_args
from howtotrainyourmamlpytorch_amd.data import SyntheticEpisodeStream
from howtotrainyourmamlpytorch_amd.meta.engine import MAMLFewShotClassifier
from howtotrainyourmamlpytorch_amd.ops import hip_autograd
from howtotrainyourmamlpytorch_amd.ops import reference as ref

H, W = 14, 15
STAGES = 3
LN_SIZES = {True: [(14, 15), (7, 7), (3, 3)], False: [(7, 8), (4, 4), (2, 2)]}


def dev():
    return torch.device("cuda", 0)


def _engine_build(device, max_pooling, inner, compute_dtype="bf16"):
    args = get_args([
        "--batch_size", "2", "--num_classes_per_set", "3",
        "--num_samples_per_class", "2", "--num_target_samples", "2",
        "--image_height", str(H), "--image_width", str(W),
        "--image_channels", "1",
        "--cnn_num_filters", "8", "--num_stages", str(STAGES),
        "--number_of_training_steps_per_iter", "2",
        "--max_pooling", str(max_pooling),
        "--norm_layer", "layer_norm",
        "--enable_inner_loop_optimizable_bn_params", str(inner),
        "--second_order", "True",
        "--first_order_to_second_order_epoch", "-1",
        "--seed", "11", "--compute_dtype", compute_dtype,
        "--fp32_support_pass", "False",
    ])
    torch.manual_seed(0)
    model = MAMLFewShotClassifier(im_shape=(2, 1, H, W), device=device, args=args)
    cls = model.classifier
    assert cls.max_pooling == max_pooling and cls.inner_loop_bn_params == inner
    # the same fixed non-zero biases in every build: the bias path carries signal
    g = torch.Generator().manual_seed(21)
    with torch.no_grad():
        for i, (ho, wo) in enumerate(LN_SIZES[max_pooling]):
            b = cls.ln_bias(i)
            assert b.shape == (ho, wo, 8)
            b.copy_(0.5 * torch.randn(ho, wo, 8, generator=g))
    return args, model


def _engine_batch():
    g = torch.Generator().manual_seed(9)
    xs = torch.randn(2, 3, 2, 1, H, W, generator=g)
    xt = torch.randn(2, 3, 2, 1, H, W, generator=g)
    ys = torch.arange(3).view(1, 3, 1).expand(2, 3, 2).contiguous()
    yt = ys.clone()
    return (xs, xt, ys, yt)


def _meta_params(model):
    cls = model.classifier
    ps = [cls.theta]
    if not cls.inner_loop_bn_params:
        ps += [getattr(cls, f"ln_bias_{i}") for i in range(STAGES)]
    return ps


def _meta_grad(model, batch):
    """Loss and the meta-gradient over theta and the ln_bias_* parameters,
    flattened into one vector."""
    losses, _ = model.train_forward_prop(batch, epoch=1)
    gs = torch.autograd.grad(losses["loss"], _meta_params(model))
    return (float(losses["loss"].detach()),
            torch.cat([g.detach().float().reshape(-1).cpu() for g in gs]))


_ORACLES = {}


def _oracle(max_pooling, inner):
    """CPU fp32 loss and meta-gradient, computed once per variant."""
    key = (max_pooling, inner)
    if key not in _ORACLES:
        _, m_cpu = _engine_build(torch.device("cpu"), max_pooling, inner)
        _ORACLES[key] = _meta_grad(m_cpu, _engine_batch())
    return _ORACLES[key]


class _Forbidden(AssertionError):
    pass


def _forbid_composition(monkeypatch):
    def raiser(*a, **k):
        raise _Forbidden("ops.reference.task_layer_norm_act reached on the kernel path")
    monkeypatch.setattr(ref, "task_layer_norm_act", raiser)


@pytest.mark.parametrize("inner", [False, True], ids=["meta_bias", "inner_bias"])
@pytest.mark.parametrize("max_pooling", [True, False], ids=["pooled", "strided"])
def test_layer_norm_backbone_kernels_close_to_cpu(max_pooling, inner, monkeypatch):
    """Fallback-free, the torch composition of the layer norm never reached,
    loss within 3e-2 of the CPU fp32 oracle, meta-gradient (theta and
    ln_bias_*) cosine > 0.95, and rel-L2 of the kernel path no worse than
    1.25x the all-torch bf16 GPU path against the same oracle (the kernel
    path keeps fp32 accumulators and rounds to bf16 less often; 25% covers
    summation-order differences on a quantity of order 0.2).

    Measured on MI355X (also in profiles/README.md), loss cpu / kernel,
    rel_kernel, rel_torch, cosine:
      pooled  meta bias   1.168629 / 1.170877  0.0625  0.0609  0.99805
      pooled  inner bias  1.173967 / 1.176699  0.0589  0.0569  0.99827
      strided meta bias   1.105285 / 1.105274  0.0726  0.0792  0.99736
      strided inner bias  1.105197 / 1.105221  0.0722  0.0769  0.99739"""
    loss_c, gc = _oracle(max_pooling, inner)
    batch = _engine_batch()

    # all-torch bf16 GPU path first, while the composition is still allowed
    ops.disable_hip_kernels()
    try:
        _, m_torch = _engine_build(dev(), max_pooling, inner)
        loss_t, gt = _meta_grad(m_torch, batch)
    finally:
        ops.enable_hip_kernels()

    hip_autograd._FALLBACK_WARNED.clear()
    with monkeypatch.context() as mp:
        _forbid_composition(mp)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            _, m_gpu = _engine_build(dev(), max_pooling, inner)
            loss_g, gg = _meta_grad(m_gpu, batch)
    fell_back = [str(r.message) for r in rec
                 if "grouped-ATen composition" in str(r.message)]
    assert not fell_back, fell_back

    assert gg.shape == gc.shape == gt.shape
    rel_kernel = ((gg - gc).norm() / gc.norm()).item()
    rel_torch = ((gt - gc).norm() / gc.norm()).item()
    cos = torch.nn.functional.cosine_similarity(gg, gc, dim=0).item()
    print(f"layer-norm backbone pooled={max_pooling} inner={inner}: "
          f"loss cpu {loss_c:.6f} kernel {loss_g:.6f} torch-bf16 {loss_t:.6f}; "
          f"rel_kernel {rel_kernel:.4f} rel_torch {rel_torch:.4f} cos {cos:.5f}")
    assert abs(loss_c - loss_g) < 3e-2
    assert cos > 0.95, f"cosine {cos:.5f}"
    assert rel_kernel <= 1.25 * rel_torch, \
        f"rel_kernel {rel_kernel:.4f} > 1.25 * rel_torch {rel_torch:.4f}"


def test_layer_norm_backbone_fp32_compute(monkeypatch):
    """--compute_dtype fp32, pooled: the fp32 layer-norm kernels are reached
    (the composition is forbidden for the run) and the loss matches the CPU
    fp32 engine to 1e-3."""
    loss_c, _ = _oracle(True, False)
    calls = []
    ext = ops.hip_ext()
    real = ext.ln_act_fwd

    def spy(x, *a):
        calls.append(x.dtype)
        return real(x, *a)

    monkeypatch.setattr(ext, "ln_act_fwd", spy)
    _forbid_composition(monkeypatch)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")      # fp32 convs are a composition
        _, m_gpu = _engine_build(dev(), True, False, compute_dtype="fp32")
        loss_g, gg = _meta_grad(m_gpu, _engine_batch())
    assert calls and all(d == torch.float32 for d in calls), calls
    assert torch.isfinite(gg).all().item()
    print(f"layer-norm backbone fp32: loss cpu {loss_c:.6f} gpu {loss_g:.6f}")
    assert abs(loss_c - loss_g) < 1e-3


def _run_once():
    torch.manual_seed(123)
    args = get_args([
        "--batch_size", "4",
        "--num_classes_per_set", "5",
        "--num_samples_per_class", "1",
        "--num_target_samples", "3",
        "--image_height", "28", "--image_width", "28", "--image_channels", "1",
        "--cnn_num_filters", "48",
        "--norm_layer", "layer_norm",
        "--number_of_training_steps_per_iter", "3",
        "--number_of_evaluation_steps_per_iter", "3",
        "--second_order", "True",
        "--first_order_to_second_order_epoch", "-1",
        "--total_epochs", "5",
        "--seed", "7",
        "--dataset_name", "synthetic",
    ])
    model = MAMLFewShotClassifier(im_shape=(2, 1, 28, 28), device=dev(), args=args)
    stream = SyntheticEpisodeStream(args)
    for batch in stream.get_train_batches(3):
        model.run_train_iter(batch, epoch=0)
    torch.cuda.synchronize()
    cls = model.classifier
    return [cls.theta.detach().clone()] + [
        getattr(cls, f"ln_bias_{i}").detach().clone() for i in range(cls.num_stages)]


def test_layer_norm_backbone_bitwise_deterministic(monkeypatch):
    """Two identical 3-iteration runs: theta and every ln_bias_* bitwise
    equal (28x28, 48 filters; stage 0 is 28*28*48 = 37632 >= the split
    threshold, so both the split and the single-workgroup kernels run)."""
    monkeypatch.setenv("MAML355_DETERMINISTIC", "1")
    _forbid_composition(monkeypatch)
    hip_autograd._FALLBACK_WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        r1 = _run_once()
    assert not [r for r in rec if "grouped-ATen composition" in str(r.message)]
    r2 = _run_once()
    assert any(b.abs().max().item() > 0 for b in r1[1:]), "ln_bias never moved"
    for a, b in zip(r1, r2):
        assert torch.isfinite(a).all().item()
        diff = (a - b).abs().max().item()
        assert torch.equal(a, b), f"deterministic runs differ: max |delta| = {diff:e}"
