"""Exact-input float64 CPU oracle for the backbone's kernels.

Every function here takes float64 CPU tensors and is differentiable by
autograd at any order.  A test feeds it *exactly the values the kernel
consumes* (``widen`` of the bf16 activations and upstream grads,
``round_bf16`` of the weights the GEMM kernels round in their repack, the
fp32 bias/gamma/beta widened), so what separates kernel and oracle is the
kernel's fp32 accumulation and its one output rounding — nothing else.

Layouts are the package's: activations ``[T, NS, H, W, C]``, conv weights
``[T, F, C, 3, 3]``, linear weights ``[T, ways, K]``.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

F64 = torch.float64
BF16_ULP = 2.0 ** -8          # spacing of bf16 relative to the value

# the tolerances of the issue: fp32 results of bf16 inputs (dw, db, sums,
# mean, var) — the figure test_wgrad_v2_matches_v1 uses
F32_RTOL, F32_ATOL = 1e-4, 1e-2


def widen(t: torch.Tensor) -> torch.Tensor:
    """The tensor's exact values as float64 on the CPU (a fresh leaf)."""
    return t.detach().to("cpu").to(F64)


def round_bf16(t: torch.Tensor) -> torch.Tensor:
    """Round to bf16 (as the GEMM repack kernels do) and widen."""
    return t.detach().to("cpu").to(torch.bfloat16).to(F64)


# ---------------------------------------------------------------------------
# ops
# ---------------------------------------------------------------------------
def conv3x3(x, w, b=None, stride=1, pad=1):
    """Task-batched 3x3 conv, one grouped float64 conv2d."""
    T, NS, H, W, C = x.shape
    Fo = w.shape[1]
    xg = x.permute(1, 0, 4, 2, 3).reshape(NS, T * C, H, W)
    wg = w.reshape(T * Fo, C, 3, 3)
    bg = b.reshape(T * Fo) if b is not None else None
    yg = F.conv2d(xg, wg, bg, stride=stride, padding=pad, groups=T)
    Ho, Wo = yg.shape[-2:]
    return yg.reshape(NS, T, Fo, Ho, Wo).permute(1, 0, 3, 4, 2).contiguous()


def linear(x, w, b=None):
    y = torch.bmm(x, w.transpose(1, 2))
    return y if b is None else y + b.unsqueeze(1)


def _affine(p, T, C):
    return p.view(1, 1, 1, 1, C) if p.dim() == 1 else p.view(T, 1, 1, 1, C)


def bn_act(x, gamma, beta, eps=1e-5, slope=0.01, apply_act=True):
    """Batch-statistics BN + leaky-ReLU.  Returns (y, mean, var, pre) with
    ``pre`` the pre-activation, which decides the leaky-ReLU side."""
    T, NS, H, W, C = x.shape
    mean = x.mean(dim=(1, 2, 3))
    var = x.var(dim=(1, 2, 3), unbiased=False)
    inv = torch.rsqrt(var + eps)
    pre = ((x - mean.view(T, 1, 1, 1, C)) * inv.view(T, 1, 1, 1, C)
           * _affine(gamma, T, C) + _affine(beta, T, C))
    y = F.leaky_relu(pre, negative_slope=slope) if apply_act else pre
    return y, mean, var, pre


def windows(x):
    """[T, NS, H, W, C] -> [T, NS, Ho, Wo, C, 4], the 2x2 windows in the
    kernels' order (0,0), (0,1), (1,0), (1,1); floor mode."""
    T, NS, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    win = x[:, :, :2 * Ho, :2 * Wo].reshape(T, NS, Ho, 2, Wo, 2, C)
    return win.permute(0, 1, 2, 4, 6, 3, 5).reshape(T, NS, Ho, Wo, C, 4)


def first_argmax(win):
    """Index of the first maximum along the last dim (ties: lowest index,
    the rule of both pool kernels)."""
    eq = win == win.max(dim=-1, keepdim=True).values
    first = eq & (eq.cumsum(dim=-1) == 1)
    return first.to(torch.uint8).argmax(dim=-1)


def pool2x2(x, arg=None):
    """2x2/2 max pool routed through ``arg`` (default: first maximum).
    Returns (y, arg); differentiable in x with the routing held fixed."""
    win = windows(x)
    if arg is None:
        arg = first_argmax(win.detach())
    y = torch.gather(win, -1, arg.long().unsqueeze(-1)).squeeze(-1)
    return y, arg


def bn_act_pool(x, gamma, beta, eps=1e-5, slope=0.01):
    """The fused op: pools the *unrounded* activation.
    Returns (y_pooled, mean, var, pre, arg)."""
    a, mean, var, pre = bn_act(x, gamma, beta, eps, slope, True)
    y, arg = pool2x2(a)
    return y, mean, var, pre, arg


# ---------------------------------------------------------------------------
# discrete decisions: what may legitimately flip between fp32 and fp64
# ---------------------------------------------------------------------------
ZERO_BAND = 1e-4
TIE_BAND = 1e-4
MAX_EXCLUDED = 1e-3


def near_zero(pre):
    """Elements whose leaky-ReLU side is within rounding of undecided."""
    return pre.detach().abs() < ZERO_BAND


def near_tied_windows(pre):
    """[T, NS, Ho, Wo, C] bool: windows whose two largest pre-activations
    differ by more than 0 and less than TIE_BAND.  Exact ties are NOT
    excluded — the first-index rule has to match there."""
    top = windows(pre.detach()).topk(2, dim=-1).values
    gap = top[..., 0] - top[..., 1]
    return (gap > 0) & (gap < TIE_BAND)


def expand_windows(wmask, H, W):
    """Window mask [T, NS, Ho, Wo, C] -> element mask [T, NS, H, W, C]
    (trailing odd row/column: False)."""
    T, NS, Ho, Wo, C = wmask.shape
    out = torch.zeros(T, NS, H, W, C, dtype=torch.bool)
    out[:, :, :2 * Ho, :2 * Wo] = (wmask.repeat_interleave(2, dim=2)
                                   .repeat_interleave(2, dim=3))
    return out


def share(mask) -> float:
    return mask.double().mean().item() if mask.numel() else 0.0


# ---------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------
def _report(name, err, bound):
    worst = (err / bound).max().item() if err.numel() else 0.0
    print(f"{name}: max|err|={err.max().item() if err.numel() else 0.0:.3e} "
          f"worst err/bound={worst:.3f}")
    return worst


def assert_bf16_close(got, ref, a, keep=None, name="value"):
    """|got - ref| <= 2^-8 |ref| + a: one bf16 ulp plus the absolute
    tolerance ``a``.  ``keep`` (bool, optional) selects the compared set."""
    got = got.detach().to("cpu").to(F64)
    ref = ref.detach()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = (got - ref).abs()
    bound = BF16_ULP * ref.abs() + a
    if keep is not None:
        err, bound = err[keep], bound[keep]
    worst = _report(name, err, bound)
    assert worst <= 1.0, f"{name}: err/bound {worst:.3f} (a={a})"


def assert_close(got, ref, rtol, atol, keep=None, name="value"):
    """|got - ref| <= atol + rtol |ref| against the float64 oracle."""
    got = got.detach().to("cpu").to(F64)
    ref = ref.detach().to(F64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = (got - ref).abs()
    bound = atol + rtol * ref.abs()
    if keep is not None:
        err, bound = err[keep], bound[keep]
    worst = _report(name, err, bound)
    assert worst <= 1.0, f"{name}: err/bound {worst:.3f} (rtol={rtol}, atol={atol})"


def assert_f32_close(got, ref, name="value"):
    assert got.dtype == torch.float32, (name, got.dtype)
    assert_close(got, ref, F32_RTOL, F32_ATOL, name=name)
