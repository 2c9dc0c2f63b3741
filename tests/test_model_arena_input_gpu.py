"""Whole model: the one-launch arena gradient and the once-per-iteration
first-layer input (``MAML355_ARENA_SCATTER=1``, ``MAML355_INPUT_PREP=1``)
against the paths they replace (both ``=0``), under MAML355_DETERMINISTIC=1.  The 14x15,
8-filter, 3-stage, 2-inner-step second-order configuration of
tests/test_bn_pool_dbwd_gpu.py, and the same with 16 filters, the smallest
width whose first layer runs on the kernels that read the prepared input.
After two training iterations (the second starts from the theta the first
one's meta-gradient moved) theta's meta-gradient, theta itself and the
target logits must be ``torch.equal``.

The meta-gradient is taken as that test takes it (``train_forward_prop`` and
``autograd.grad`` w.r.t. theta), with a plain gradient step in between.

Known limit, older than these kernels: where a fast-weight arena collects
three gradient contributions (the LSLR pass-through, the support pass, the
previous step's target pass) autograd adds them in the order its nodes
become ready, and that order can move with the process's history of autograd
calls (two identical runs with both toggles off were seen to differ by
4 ulp in theta's gradient when one of them was the first model run of its
process; the logits never moved).  A fresh process with equal arguments
repeats itself, which is what the whole-run comparisons use."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from howtotrainyourmamlpytorch_amd import ops
from howtotrainyourmamlpytorch_amd.config import get_args
from howtotrainyourmamlpytorch_amd.meta.engine import MAMLFewShotClassifier

IH, IW = 14, 15
TOGGLES = ("MAML355_ARENA_SCATTER", "MAML355_INPUT_PREP")


def dev():
    return torch.device("cuda", 0)


def _two_iterations(filters):
    args = get_args([
        "--batch_size", "2", "--num_classes_per_set", "3",
        "--num_samples_per_class", "2", "--num_target_samples", "2",
        "--image_height", str(IH), "--image_width", str(IW),
        "--image_channels", "1",
        "--cnn_num_filters", str(filters), "--num_stages", "3",
        "--number_of_training_steps_per_iter", "2",
        "--max_pooling", "True",
        "--second_order", "True",
        "--first_order_to_second_order_epoch", "-1",
        "--seed", "11", "--compute_dtype", "bf16",
        "--fp32_support_pass", "False",
    ])
    torch.manual_seed(0)
    model = MAMLFewShotClassifier(im_shape=(2, 1, IH, IW), device=dev(),
                                  args=args)
    assert model.classifier.max_pooling
    g = torch.Generator().manual_seed(9)
    theta = model.classifier.theta
    grad = logits = None
    for _ in range(2):
        xs = torch.randn(2, 3, 2, 1, IH, IW, generator=g)
        xt = torch.randn(2, 3, 2, 1, IH, IW, generator=g)
        ys = torch.arange(3).view(1, 3, 1).expand(2, 3, 2).contiguous()
        losses, logits = model.train_forward_prop((xs, xt, ys, ys.clone()),
                                                  epoch=1)
        grad = torch.autograd.grad(losses["loss"], theta)[0]
        with torch.no_grad():
            theta.sub_(0.05 * grad)
    return grad.detach().clone(), theta.detach().clone(), logits.clone()


@pytest.mark.parametrize("filters", [8, 16])
def test_model_bits(monkeypatch, filters):
    calls = []
    ext = ops.hip_ext()
    for name in ("arena_scatter", "conv_input_prep"):
        def counted(*a, _real=getattr(ext, name), _name=name):
            calls.append(_name)
            return _real(*a)
        monkeypatch.setattr(ext, name, counted)
    monkeypatch.setenv("MAML355_DETERMINISTIC", "1")
    for k in TOGGLES:
        monkeypatch.setenv(k, "0")
    want = _two_iterations(filters)
    assert not calls
    for k in TOGGLES:
        monkeypatch.setenv(k, "1")
    got = _two_iterations(filters)
    assert "arena_scatter" in calls, "the native arena gradient did not run"
    # 8 filters have no direct first-layer kernel, so there that layer keeps
    # preparing its own input; with 16 the prepared pair must be in use
    assert ("conv_input_prep" in calls) == (filters == 16)
    for name, a, b in zip(("theta.grad", "theta", "logits"), want, got):
        assert torch.isfinite(a).all().item() and a.abs().max().item() > 0
        assert torch.equal(a, b), \
            f"{name}: max|delta|=" \
            f"{(a.double() - b.double()).abs().max().item():.3e}"
