"""GPU tests for the global-average-pool kernels (gavgpool.hip) and their
autograd wrappers.  Tolerance: the forward is ONE bf16 rounding of an
fp32-accumulated mean, so rtol = atol = 1e-2 (inside the 2e-2 the project
uses for the bf16 BN forward)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from howtotrainyourmamlpytorch_amd import ops
from howtotrainyourmamlpytorch_amd.ops import reference as ref

TOL = dict(rtol=1e-2, atol=1e-2)

# [T, NS, H, W, C]
SHAPES = [(2, 5, 2, 2, 48), (3, 7, 6, 6, 64), (2, 3, 4, 3, 8),
          (1, 1, 1, 1, 48), (2, 3, 3, 3, 5)]


def dev():
    return torch.device("cuda", 0)


def _x(shape, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dev(), torch.bfloat16)


def test_extension_has_gavgpool():
    ext = ops.hip_ext()
    assert hasattr(ext, "gavgpool_fwd") and hasattr(ext, "gavgpool_bwd")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gavgpool_fwd_bwd_match_reference(shape):
    T, NS, H, W, C = shape
    x = _x(shape, seed=sum(shape)).requires_grad_(True)
    y = ops.task_global_avgpool(x)
    yr = ref.task_global_avgpool(x.detach().float().cpu())
    assert y.shape == (T, NS, C) and y.dtype == torch.bfloat16
    torch.testing.assert_close(y.detach().float().cpu(), yr, **TOL)

    g = torch.randn_like(y)
    (dx,) = torch.autograd.grad(y, x, g)
    dxr = (g.float().cpu() / (H * W)).view(T, NS, 1, 1, C).expand(T, NS, H, W, C)
    assert dx.shape == x.shape
    torch.testing.assert_close(dx.float().cpu(), dxr, **TOL)

    # deterministic: fixed summation order -> two calls bitwise equal
    y2 = ops.task_global_avgpool(x)
    assert (y == y2).all().item()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gavgpool_double_backward_matches_reference(shape):
    """create_graph through the pool: the upstream grad g is a function of
    x (as in the second-order inner loop), so the second backward runs
    _GAvgPoolBwdFn.backward = the forward kernel on the incoming grad."""
    x = _x(shape, seed=1 + sum(shape))

    def run(opmod, x_):
        x_ = x_.requires_grad_(True)
        y = opmod.task_global_avgpool(x_)
        (gx,) = torch.autograd.grad((y.float() ** 2).sum(), x_, create_graph=True)
        (ggx,) = torch.autograd.grad((gx.float() ** 2).sum(), x_)
        return gx.detach(), ggx

    gx, ggx = run(ops, x.clone())
    gxr, ggxr = run(ref, x.float().cpu())
    torch.testing.assert_close(gx.float().cpu(), gxr, **TOL)
    torch.testing.assert_close(ggx.float().cpu(), ggxr, **TOL)


def test_dispatch_reaches_the_kernel(monkeypatch):
    """bf16 CUDA input goes through the extension, not ref.x.mean; fp32
    input stays on the reference."""
    ext = ops.hip_ext()
    x = _x((2, 5, 3, 2, 48), seed=4)
    direct = ext.gavgpool_fwd(x.reshape(10, 3, 2, 48)).view(2, 5, 48)

    def boom(_):
        raise AssertionError("reference avgpool called for bf16 CUDA input")

    monkeypatch.setattr(ref, "task_global_avgpool", boom)
    y = ops.task_global_avgpool(x)
    assert (y == direct).all().item()
    monkeypatch.undo()
    yf = ops.task_global_avgpool(x.float())
    assert yf.dtype == torch.float32
    torch.testing.assert_close(yf, x.float().mean(dim=(2, 3)))
