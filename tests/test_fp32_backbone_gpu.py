"""The pooled backbone with fp32 activations on the gfx950 kernels:
``--compute_dtype fp32`` (the GPU oracle mode) against the CPU fp32 engine
at the figures of test_ops_gpu.py::test_engine_gpu_fp32_matches_cpu_tight,
with no grouped-ATen fallback, and ``--fp32_support_pass True`` bitwise
repeatable under MAML355_DETERMINISTIC=1."""

import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

from howtotrainyourmamlpytorch_amd.config import get_args
from howtotrainyourmamlpytorch_amd.data import SyntheticEpisodeStream
from howtotrainyourmamlpytorch_amd.meta.engine import MAMLFewShotClassifier
from howtotrainyourmamlpytorch_amd.ops import hip_autograd


def dev():
    return torch.device("cuda", 0)


def _fallbacks(rec):
    return [str(r.message) for r in rec
            if "grouped-ATen composition" in str(r.message)]


# the engine shapes of test_ops_gpu.py::_engine_build
def _engine_build(device, compute_dtype="bf16", fp32_support="False"):
    args = get_args([
        "--batch_size", "2", "--num_classes_per_set", "3",
        "--num_samples_per_class", "2", "--num_target_samples", "2",
        "--image_height", "14", "--image_width", "14", "--image_channels", "1",
        "--cnn_num_filters", "8", "--num_stages", "3",
        "--number_of_training_steps_per_iter", "2",
        "--seed", "11", "--compute_dtype", compute_dtype,
        "--fp32_support_pass", fp32_support,
    ])
    torch.manual_seed(0)
    return args, MAMLFewShotClassifier(im_shape=(2, 1, 14, 14),
                                       device=device, args=args)


def _engine_batch():
    g = torch.Generator().manual_seed(9)
    xs = torch.randn(2, 3, 2, 1, 14, 14, generator=g)
    xt = torch.randn(2, 3, 2, 1, 14, 14, generator=g)
    ys = torch.arange(3).view(1, 3, 1).expand(2, 3, 2).contiguous()
    yt = ys.clone()
    return (xs, xt, ys, yt)


def _theta_grad(model, batch):
    losses, _ = model.train_forward_prop(batch, epoch=1)
    g = torch.autograd.grad(losses["loss"], model.classifier.theta)[0]
    return float(losses["loss"].detach()), g


def test_fp32_engine_on_kernels_matches_cpu_without_fallback(monkeypatch):
    """--compute_dtype fp32 with the kernels ENABLED against the CPU fp32
    engine: loss within 1e-4, theta grad within rtol 1e-3 / atol 1e-5, and
    no conv left on the grouped-ATen composition."""
    monkeypatch.delenv("MAML355_FCONV", raising=False)
    batch = _engine_batch()
    _, m_cpu = _engine_build(torch.device("cpu"))
    loss_c, gc = _theta_grad(m_cpu, batch)
    hip_autograd._FALLBACK_WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        _, m_gpu = _engine_build(dev(), compute_dtype="fp32")
        loss_g, gg = _theta_grad(m_gpu, batch)
    diff = (gg.cpu() - gc).abs()
    print(f"fp32 engine on kernels: loss cpu {loss_c:.7f} gpu {loss_g:.7f} "
          f"|dloss|={abs(loss_c - loss_g):.3e}; theta grad max|diff|="
          f"{diff.max().item():.3e} worst diff/(1e-5+1e-3|ref|)="
          f"{(diff / (1e-5 + 1e-3 * gc.abs())).max().item():.3f}")
    assert not _fallbacks(rec), _fallbacks(rec)
    assert abs(loss_c - loss_g) < 1e-4
    torch.testing.assert_close(gg.cpu(), gc, rtol=1e-3, atol=1e-5)


def _train_args():
    return get_args([
        "--batch_size", "4",
        "--num_classes_per_set", "5",
        "--num_samples_per_class", "1",
        "--num_target_samples", "3",
        "--image_height", "28", "--image_width", "28", "--image_channels", "1",
        "--cnn_num_filters", "48",
        "--number_of_training_steps_per_iter", "3",
        "--number_of_evaluation_steps_per_iter", "3",
        "--second_order", "True",
        "--first_order_to_second_order_epoch", "-1",
        "--total_epochs", "5",
        "--seed", "7",
        "--dataset_name", "synthetic",
        "--fp32_support_pass", "True",
    ])


def _run_once():
    torch.manual_seed(123)
    args = _train_args()
    device = torch.device("cuda", 0)
    model = MAMLFewShotClassifier(im_shape=(2, 1, 28, 28), device=device, args=args)
    stream = SyntheticEpisodeStream(args)
    for batch in stream.get_train_batches(3):
        model.run_train_iter(batch, epoch=0)
    torch.cuda.synchronize()
    return model.classifier.theta.detach().clone()


def test_fp32_support_pass_bitwise_equal_under_deterministic_mode(monkeypatch):
    """Mixed precision (fp32 support chain, bf16 targets): theta after three
    iterations is bitwise equal between two runs, with no fallback."""
    monkeypatch.setenv("MAML355_DETERMINISTIC", "1")
    monkeypatch.delenv("MAML355_FCONV", raising=False)
    hip_autograd._FALLBACK_WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        t1 = _run_once()
        t2 = _run_once()
    assert not _fallbacks(rec), _fallbacks(rec)
    assert torch.isfinite(t1).all().item()
    diff = (t1 - t2).abs().max().item()
    assert torch.equal(t1, t2), f"deterministic runs differ: max |delta| = {diff:e}"
