"""End-to-end GPU check of the strided (max_pooling=False) backbone:
stride-2 conv trio + BN/act + global average pool + linear head, second
order, entirely on the HIP kernels.  Image 14x15 so H goes 14->7->4->2 and
W goes 15->8->4->2 (even, odd and non-square sizes in one net)."""

import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

from howtotrainyourmamlpytorch_amd import ops
from howtotrainyourmamlpytorch_amd.config import get_args
from howtotrainyourmamlpytorch_amd.data import SyntheticEpisodeStream
from howtotrainyourmamlpytorch_amd.meta.engine import MAMLFewShotClassifier
from howtotrainyourmamlpytorch_amd.ops import hip_autograd

H, W = 14, 15


def dev():
    return torch.device("cuda", 0)


def _engine_build(device, compute_dtype="bf16"):
    args = get_args([
        "--batch_size", "2", "--num_classes_per_set", "3",
        "--num_samples_per_class", "2", "--num_target_samples", "2",
        "--image_height", str(H), "--image_width", str(W),
        "--image_channels", "1",
        "--cnn_num_filters", "8", "--num_stages", "3",
        "--number_of_training_steps_per_iter", "2",
        "--max_pooling", "False",
        "--second_order", "True",
        "--first_order_to_second_order_epoch", "-1",
        "--seed", "11", "--compute_dtype", compute_dtype,
        "--fp32_support_pass", "False",
    ])
    torch.manual_seed(0)
    return args, MAMLFewShotClassifier(im_shape=(2, 1, H, W),
                                       device=device, args=args)


def _engine_batch():
    g = torch.Generator().manual_seed(9)
    xs = torch.randn(2, 3, 2, 1, H, W, generator=g)
    xt = torch.randn(2, 3, 2, 1, H, W, generator=g)
    ys = torch.arange(3).view(1, 3, 1).expand(2, 3, 2).contiguous()
    yt = ys.clone()
    return (xs, xt, ys, yt)


def _theta_grad(model, batch):
    losses, _ = model.train_forward_prop(batch, epoch=1)
    g = torch.autograd.grad(losses["loss"], model.classifier.theta)[0]
    return float(losses["loss"].detach()), g


@pytest.fixture(scope="module")
def oracle():
    """CPU fp32 loss and meta-gradient, computed once for the module."""
    _, m_cpu = _engine_build(torch.device("cpu"))
    assert not m_cpu.classifier.max_pooling
    assert m_cpu.classifier.final_spatial == (2, 2)
    loss_c, gc = _theta_grad(m_cpu, _engine_batch())
    return loss_c, gc.detach().clone()


def test_strided_backbone_kernels_close_to_cpu(oracle):
    """Fallback-free, loss within 3e-2 of the CPU fp32 oracle, meta-gradient
    cosine > 0.95, and rel-L2 of the kernel path no worse than 1.25x the
    all-torch bf16 GPU path against the same oracle (the kernel path keeps
    fp32 accumulators and rounds to bf16 less often; 25% covers
    summation-order differences on a quantity of order 0.2).

    Measured on MI355X: rel_kernel 0.0978, rel_torch 0.0983, cosine
    0.9952, loss 1.12707 vs oracle 1.12779 (also in profiles/README.md)."""
    loss_c, gc = oracle
    batch = _engine_batch()

    hip_autograd._FALLBACK_WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        _, m_gpu = _engine_build(dev())
        loss_g, gg = _theta_grad(m_gpu, batch)
    fell_back = [str(r.message) for r in rec
                 if "grouped-ATen composition" in str(r.message)]
    assert not fell_back, fell_back

    ops.disable_hip_kernels()
    try:
        _, m_torch = _engine_build(dev())
        loss_t, gt = _theta_grad(m_torch, batch)
    finally:
        ops.enable_hip_kernels()

    gg, gt = gg.float().cpu(), gt.float().cpu()
    rel_kernel = ((gg - gc).norm() / gc.norm()).item()
    rel_torch = ((gt - gc).norm() / gc.norm()).item()
    cos = torch.nn.functional.cosine_similarity(gg.flatten(), gc.flatten(),
                                                dim=0).item()
    print(f"strided backbone: loss cpu {loss_c:.6f} kernel {loss_g:.6f} "
          f"torch-bf16 {loss_t:.6f}; rel_kernel {rel_kernel:.4f} "
          f"rel_torch {rel_torch:.4f} cos {cos:.5f}")
    assert abs(loss_c - loss_g) < 3e-2
    assert cos > 0.95, f"cosine {cos:.5f}"
    assert rel_kernel <= 1.25 * rel_torch, \
        f"rel_kernel {rel_kernel:.4f} > 1.25 * rel_torch {rel_torch:.4f}"


def _run_once():
    torch.manual_seed(123)
    args = get_args([
        "--batch_size", "4",
        "--num_classes_per_set", "5",
        "--num_samples_per_class", "1",
        "--num_target_samples", "3",
        "--image_height", "28", "--image_width", "28", "--image_channels", "1",
        "--cnn_num_filters", "48",
        "--max_pooling", "False",
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
    return model.classifier.theta.detach().clone()


def test_strided_backbone_bitwise_deterministic(monkeypatch):
    monkeypatch.setenv("MAML355_DETERMINISTIC", "1")
    hip_autograd._FALLBACK_WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        t1 = _run_once()
    assert not [r for r in rec if "grouped-ATen composition" in str(r.message)]
    t2 = _run_once()
    assert torch.isfinite(t1).all().item()
    diff = (t1 - t2).abs().max().item()
    assert (t1 == t2).all().item(), \
        f"deterministic runs differ: max |delta| = {diff:e}"
