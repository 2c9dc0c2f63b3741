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


def softmax_ce(logits, labels):
    """Per-task mean of ``logsumexp - l[y]``: logits [T, M, ways], labels
    [T, M] (any integer type) -> [T]."""
    lse = torch.logsumexp(logits, dim=-1)
    ly = logits.gather(-1, labels.long().unsqueeze(-1)).squeeze(-1)
    return (lse - ly).mean(dim=1)


def lslr(arena, grad, lr_vec):
    """``arena - lr_vec * grad``: arena/grad [T, P], lr_vec [P]."""
    return arena - lr_vec.unsqueeze(0) * grad


def adam_step(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay=0.0,
              clamp=None):
    """One Adam step, pure: returns the new ``(p, m, v)``.  The gradient is
    clamped first, then the decay ``weight_decay * p`` is added — the order
    of adam.hip and ``ops.reference``.  Bias corrections in double."""
    if clamp is not None:
        g = g.clamp(-clamp, clamp)
    if weight_decay != 0.0:
        g = g + weight_decay * p
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    denom = (v / bc2).sqrt() + eps
    return p - (lr / bc1) * m / denom, m, v


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


# ---------------------------------------------------------------------------
# derived bounds of the head, loss and update kernels (fp32 arithmetic,
# unit roundoff EPS32 = 2^-24), all against the float64 functions above
# ---------------------------------------------------------------------------
EPS32 = 2.0 ** -24


def assert_within(got, ref, bound, name="value"):
    """|got - ref| <= bound elementwise, every element compared; a zero
    bound demands equality.  Returns the worst err/bound."""
    got = got.detach().to("cpu").to(F64)
    ref = ref.detach().to(F64)
    bound = bound.detach().to(F64).expand_as(ref)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = (got - ref).abs()
    exact = bound == 0
    assert (err[exact] == 0).all().item(), f"{name}: nonzero error at a zero bound"
    worst = _report(name, err[~exact], bound[~exact])
    assert worst <= 1.0, f"{name}: err/bound {worst:.3f}"
    return worst


def dot_bound(mag, n, ref=None):
    """An fp32 dot product of length n, summed in any order with or without
    fma: ``(n + 2) 2^-24 sum|a||b|`` (``mag`` is that sum).  With ``ref``
    the result is then rounded to bf16: one more ``2^-8 |ref|``."""
    bound = (n + 2) * EPS32 * mag
    return bound if ref is None else bound + BF16_ULP * ref.abs()


def assert_dot_bounded(got, ref, mag, n, name, bf16=False):
    assert got.dtype == (torch.bfloat16 if bf16 else torch.float32), (name, got.dtype)
    return assert_within(got, ref, dot_bound(mag, n, ref if bf16 else None),
                         f"{name} (n={n})")


CE_RTOL = CE_ATOL = 1e-5      # test_ce_fwd_bwd_and_create_graph's figures


def ce_loss_bound(ref, logits):
    """[T]: the N(0,1) figure plus the cancellation of ``log(se) + max -
    l[y]``, whose middle sum is rounded at the size of the logits:
    ``2^-23 max|logit|`` over the task."""
    return (CE_ATOL + CE_RTOL * ref.abs()
            + 2 * EPS32 * logits.detach().abs().amax(dim=(1, 2)))


def ce_prob_bound(ref, logits, bf16=False):
    """Anything linear in the softmax probabilities.  ``exp(v - max)`` is
    evaluated as ``exp2((v - max) * log2 e)``; the product's rounding is a
    relative error ``|v - max| 2^-24`` of the result, twice that with the
    constant's own: ``2^-23 max_row|logit - max| |ref|`` on top of the
    N(0,1) figure.  ``ref`` is [T, M, ways] (per row) or [T] (per task)."""
    lg = logits.detach()
    spread = lg.amax(dim=-1) - lg.amin(dim=-1)             # [T, M]
    spread = spread.unsqueeze(-1) if ref.dim() == 3 else spread.amax(dim=1)
    bound = CE_ATOL + (CE_RTOL + 2 * EPS32 * spread) * ref.abs()
    return bound + BF16_ULP * ref.abs() if bf16 else bound


def adam_bias_terms(beta1, beta2, step):
    """(d1, d2, e_bc) for ``1 - powf(beta, step)`` formed in fp32:
    ``d = beta^step (step + 2) 2^-24`` for the power plus ``2^-24 bc`` for
    the rounding of the subtraction — all that is left of the error once
    ``beta^step`` has dropped below ulp(1).  ``e_bc = d1/bc1 + d2/(2 bc2)``
    is the relative error they put on the step size."""
    out = []
    for beta in (beta1, beta2):
        bc = 1.0 - beta ** step
        out.append((beta ** step * (step + 2) * EPS32 + EPS32 * bc, bc))
    (d1, bc1), (d2, bc2) = out
    return d1, d2, d1 / bc1 + d2 / (2.0 * bc2)


def adam_bounds(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay=0.0,
                clamp=None):
    """Reference and bound of one fp32 Adam step on float64 copies of the
    kernel's own inputs.  Returns ``((p, m, v), (bound_p, bound_m,
    bound_v))``.

    With u = 2^-24 and G = |clamp(g)| + |weight_decay p| the magnitude of
    the gradient the moments see (x = 2 roundings on it with decay, 0
    without, when it is exact):
      m: (4 + x) u (|beta1 m0| + (1 - beta1) G)
      v: (5 + 2x) u (beta2 v0 + (1 - beta2) G^2)         (= 5 u ref without decay)
      p: u |ref| + dp_mag (e_bc + (8 + 2x) u + (5 + 2x)/2 u (v_mag/v - 1))
    where dp_mag = lr m_mag / (bc1 denom) is |dp| with the two terms of m
    taken by magnitude: where they cancel, the error of m is not small next
    to m itself.  The widening is per element: without decay, wherever
    beta1 m0 and (1 - beta1) g share a sign (m_mag = |m|, v_mag = v) these
    are exactly the plain ``4 u (..)``, ``5 u v`` and ``u |ref| + |dp|
    (e_bc + 8 u)``, which is the case for 53% of the elements of the tests'
    no-decay inputs.  Elsewhere the p bound grows with m_mag / |m|: on the
    tests' inputs up to 1440 times the plain one, at single elements where
    m cancels almost entirely.  The fp32 reference breaks the plain forms
    there (p by 14.8 at step 100000 from zero params, m by 1.57 under
    decay)."""
    ref = adam_step(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, clamp)
    x = 2 if weight_decay != 0.0 else 0
    gc = g.clamp(-clamp, clamp) if clamp is not None else g
    G = gc.abs() + abs(weight_decay) * p.abs()
    m_mag = (beta1 * m).abs() + (1.0 - beta1) * G
    v_mag = beta2 * v + (1.0 - beta2) * G * G
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    _, _, e_bc = adam_bias_terms(beta1, beta2, step)
    dp_mag = lr * m_mag / (bc1 * ((ref[2] / bc2).sqrt() + eps))
    rv = v_mag / ref[2].clamp_min(1e-300)
    bound_p = EPS32 * ref[0].abs() + dp_mag * (
        e_bc + (8 + 2 * x) * EPS32 + 0.5 * (5 + 2 * x) * EPS32 * (rv - 1.0))
    return ref, (bound_p, (4 + x) * EPS32 * m_mag, (5 + 2 * x) * EPS32 * v_mag)
