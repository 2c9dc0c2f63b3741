"""Exact-input float64 CPU oracle for the layer-norm kernels
(layernorm.hip), in the manner of tests/_oracle.py, whose ``widen``,
``assert_*``, ``near_zero``, ``share`` and ``MAX_EXCLUDED`` the layer-norm
tests use alongside this.

Differentiable by autograd at any order: the first and second backward
that the kernels evaluate in closed form are obtained here by
``torch.autograd.grad`` of this forward, never from those formulas."""

from __future__ import annotations

import torch
import torch.nn.functional as F

from _oracle import (F64, MAX_EXCLUDED, assert_bf16_close,  # noqa: F401
                     assert_close, assert_f32_close, near_zero, share, widen)


def ln_act(x, bias, eps=1e-5, slope=0.01, apply_act=True):
    """Per-image LayerNorm over (H, W, C), weight 1, elementwise bias, then
    leaky-ReLU.

    x: [T, NS, H, W, C]; bias: [H, W, C] (shared) or [T, H, W, C].
    Returns (y, mean [T, NS], rstd [T, NS], pre) with ``pre`` the
    pre-activation, which decides the leaky-ReLU side."""
    T, NS, H, W, C = x.shape
    mean = x.mean(dim=(2, 3, 4))
    var = x.var(dim=(2, 3, 4), unbiased=False)
    rstd = torch.rsqrt(var + eps)
    b = bias.reshape(1, 1, H, W, C) if bias.dim() == 3 else bias.reshape(T, 1, H, W, C)
    pre = (x - mean.view(T, NS, 1, 1, 1)) * rstd.view(T, NS, 1, 1, 1) + b
    y = F.leaky_relu(pre, negative_slope=slope) if apply_act else pre
    return y, mean, rstd, pre


def per_task_bias(bias, T):
    """[H, W, C] or [T, H, W, C] -> float64 [T, H, W, C] leaf, so that the
    gradient comes per task (the kernels' ``dbias_t``)."""
    b = widen(bias)
    if b.dim() == 3:
        b = b.unsqueeze(0).expand(T, -1, -1, -1)
    return b.clone().requires_grad_(True)
