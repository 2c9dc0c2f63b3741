"""autograd.Function wrappers around the HIP/CDNA4 kernels.

Double-backward policy (second-order MAML needs ``create_graph=True``
through the inner-loop support forward):

* the conv trio (fwd/dgrad/wgrad) is mutually bilinear — each backward
  composes the other two kernels, so convs run on custom kernels at every
  derivative order.  There is one trio of Functions; a backend record
  (``_ConvBackend``) names the kernels behind it: bf16 stride 1
  (tconv.hip, wgrad_nt.hip, dconv.hip), bf16 stride 2 of the
  max_pooling=False backbone (sconv.hip) and fp32 stride 1 (fconv.hip);
* BN+act and softmax-CE make their *first backward* its own Function
  whose backward evaluates the analytic closed-form second derivative
  (bn_dbwd.hip / ce_dbwd) — also custom kernels at every order;
* LayerNorm+bias+act (layernorm.hip) follows the BN pattern: its first
  backward is its own Function, whose backward is the closed-form
  ``ln_act_dbwd`` kernel — custom kernels at every order, bf16 and fp32;
* LSLR update and maxpool are bilinear in their saved tensors — custom at
  every order; the global average pool is linear (backward = broadcast
  kernel, whose backward is the forward kernel again);
* the fused BN+act+pool op uses a single-pass fused backward when the
  backward itself is not being differentiated, and composes the
  individual Functions under create_graph.  What runs under those
  Functions' backwards is native: a gather kernel for the pool, one call
  for the BN double-backward (``MAML355_BNPOOL_DBWD=0`` restores the
  torch.gather glue, the tensor formula for d_gamma_t and the scalar sums
  kernel; both give the same bits).

fp32 activations (``--compute_dtype fp32``, ``--fp32_support_pass``): the
stride-1 convs take the fconv.hip backend (exact fp32 MFMA, unrounded
weights, ordered split-K wgrad) and the linear head runs on linear.hip's
fp32 instantiation, composed like its bf16 twin.  ``MAML355_FCONV=0``
restores the grouped-ATen conv and ``torch.bmm`` for A/B runs.

Convs with a stride other than 1 or 2, more than 64 channels, or fp32
compute at stride 2 fall back to the grouped-ATen composition, with a
warning.
"""

from __future__ import annotations

import collections
import os

import torch

from . import hip_ext
from . import reference as ref


def _ext():
    e = hip_ext()
    assert e is not None, "hip_autograd used without loaded extension"
    return e


def _dbwd_glue_off() -> bool:
    """The second-order BN / pool backward without ATen glue: the pool's
    double-backward gather is a kernel, the BN double-backward is one native
    call (vector sums, d_gamma_t finished in the reduce).  Every result
    keeps its bits.  MAML355_BNPOOL_DBWD=0 restores the torch.gather glue,
    the tensor formula for d_gamma_t and the scalar sums kernel (A/B)."""
    return os.environ.get("MAML355_BNPOOL_DBWD", "1") != "0"


# ---------------------------------------------------------------------------
# fused BN + leaky-ReLU
# ---------------------------------------------------------------------------
class _BNBwdFn(torch.autograd.Function):
    """The first backward of BN+act as its own Function: forward = fused
    bwd kernels; backward = the analytic double-backward kernels
    (bn_dbwd.hip).  This is what makes second-order MAML's create_graph
    pass run entirely on custom kernels."""

    @staticmethod
    def forward(ctx, x3, gamma, beta, u, mean, rstd, slope, act):
        dx, dgamma_t, dbeta_t = _ext().bn_act_bwd(
            u, x3, mean, rstd, gamma.float(), beta.float(), slope, act)
        ctx.save_for_backward(x3, gamma, beta, u, mean, rstd)
        ctx.slope, ctx.act = slope, act
        # absent grads stay None instead of zero-filled tensors
        ctx.set_materialize_grads(False)
        return dx, dgamma_t, dbeta_t

    @staticmethod
    def backward(ctx, gx, ggam_t, gbet_t):
        x3, gamma, beta, u, mean, rstd = ctx.saved_tensors
        T, M, C = x3.shape
        if gx is None:
            gx = torch.zeros_like(x3)
        if _dbwd_glue_off():
            # one native call: absent ggam_t / gbet_t read as zero inside,
            # d_gamma_t finished in the ordered reduce (same bits as the
            # tensor formula below)
            d_u, d_x, d_gamma_t, _ = _ext().bn_act_dbwd_full(
                x3, u, gx.contiguous(), mean, rstd, gamma.float(),
                beta.float(), ggam_t, gbet_t, ctx.slope, ctx.act)
        else:
            if ggam_t is None:
                ggam_t = torch.zeros(T, C, device=x3.device, dtype=torch.float32)
            if gbet_t is None:
                gbet_t = torch.zeros(T, C, device=x3.device, dtype=torch.float32)
            d_u, d_x, sums = _ext().bn_act_dbwd(
                x3, u, gx.contiguous(), mean, rstd, gamma.float(), beta.float(),
                ggam_t, gbet_t, ctx.slope, ctx.act)
            # d_gamma_t = rstd * M * (Gu - s1*G - s2*Gxh)   (means over M)
            s = sums / M   # [T,5,C] means: {0:s1, 1:s2, 2:G, 3:Gxh, 4:Gu}
            d_gamma_t = rstd * M * (s[:, 4] - s[:, 0] * s[:, 2] - s[:, 1] * s[:, 3])
        per_task = gamma.dim() == 2
        d_gamma = d_gamma_t if per_task else d_gamma_t.sum(0)
        return (d_x, d_gamma.to(gamma.dtype), None, d_u, None, None, None, None)


class _BNActFn(torch.autograd.Function):
    """x3 [T, M, C] -> (y, mean, var).  Fused kernels at every order."""

    @staticmethod
    def forward(ctx, x3, gamma, beta, eps, slope, act):
        y, mean, var, rstd = _ext().bn_act_fwd(x3, gamma.float(), beta.float(),
                                               eps, slope, act)
        ctx.save_for_backward(x3, mean, rstd, gamma, beta)
        ctx.eps, ctx.slope, ctx.act = eps, slope, act
        ctx.mark_non_differentiable(mean, var)
        return y, mean, var

    @staticmethod
    def backward(ctx, dy, dmean, dvar):
        x3, mean, rstd, gamma, beta = ctx.saved_tensors
        dx, dgamma_t, dbeta_t = _BNBwdFn.apply(
            x3, gamma, beta, dy.contiguous(), mean, rstd, ctx.slope, ctx.act)
        if gamma.dim() == 2:
            dgamma, dbeta = dgamma_t, dbeta_t
        else:
            dgamma, dbeta = dgamma_t.sum(0), dbeta_t.sum(0)
        return dx, dgamma.to(gamma.dtype), dbeta.to(beta.dtype), None, None, None


def task_bn_act(x, gamma, beta, eps=1e-5, negative_slope=0.01, apply_act=True):
    T, NS, H, W, C = x.shape
    x3 = x.reshape(T, NS * H * W, C).contiguous()
    y, mean, var = _BNActFn.apply(x3, gamma, beta, eps, negative_slope, apply_act)
    return y.view(T, NS, H, W, C), mean, var


class _BNActPoolFn(torch.autograd.Function):
    """Fused normalize+leakyReLU+2x2 maxpool FORWARD (one pass over the
    conv output instead of write+reread of the activation); the backward
    composes the existing differentiable pool-bwd and BN-bwd Functions, so
    second-order behavior is identical to the unfused pair.  (Running the
    fused backward kernels under create_graph as one Function of their own
    was tried: bitwise equal to the pair at the test shapes, but the
    deterministic benchmark's outputs moved after three steps, so the pair
    stays.)"""

    @staticmethod
    def forward(ctx, x5, gamma, beta, eps, slope, sums):
        y, mask, mean, var, rstd = _ext().bn_act_pool_fwd(
            x5, gamma.float(), beta.float(), eps, slope, sums)
        ctx.save_for_backward(x5, gamma, beta, mean, rstd, mask)
        ctx.slope = slope
        ctx.mark_non_differentiable(mean, var)
        return y, mean, var

    @staticmethod
    def backward(ctx, dy, dmean, dvar):
        x5, gamma, beta, mean, rstd, mask = ctx.saved_tensors
        T, NB, H, W, C = x5.shape
        Ho, Wo = H // 2, W // 2
        if torch.is_grad_enabled() or os.environ.get("MAML355_NO_BWDFUSE", "0") == "1":
            # create_graph (second-order inner loop): compose the
            # differentiable Functions (their backwards are native calls:
            # a gather kernel and bn_act_dbwd_full)
            da = _PoolBwdFn.apply(dy.contiguous().view(T * NB, Ho, Wo, C),
                                  mask.view(T * NB, Ho, Wo, C), H, W)
            dx, dgamma_t, dbeta_t = _BNBwdFn.apply(
                x5.view(T, NB * H * W, C), gamma, beta,
                da.view(T, NB * H * W, C), mean, rstd, ctx.slope, True)
            dx = dx.view(T, NB, H, W, C)
        else:
            # plain backward: fully fused (no da materialization)
            dx, dgamma_t, dbeta_t = _ext().bn_act_pool_bwd(
                dy.contiguous(), mask, x5, mean, rstd, gamma.float(),
                beta.float(), ctx.slope)
        if gamma.dim() == 2:
            dgamma, dbeta = dgamma_t, dbeta_t
        else:
            dgamma, dbeta = dgamma_t.sum(0), dbeta_t.sum(0)
        return (dx, dgamma.to(gamma.dtype),
                dbeta.to(beta.dtype), None, None, None)


def task_bn_act_pool(x, gamma, beta, eps=1e-5, negative_slope=0.01, sums=None):
    y, mean, var = _BNActPoolFn.apply(x.contiguous(), gamma, beta, eps,
                                      negative_slope, sums)
    return y, mean, var


# ---------------------------------------------------------------------------
# fused LayerNorm (per image, weight 1) + elementwise bias + leaky-ReLU
# ---------------------------------------------------------------------------
class _LNBwdFn(torch.autograd.Function):
    """The first backward of LN+act as its own Function: forward = the bwd
    kernels; backward = the analytic double-backward kernel.  The bias gets
    no gradient here (the leaky-ReLU side is held constant), as BN's beta
    gets none in ``_BNBwdFn``."""

    @staticmethod
    def forward(ctx, x, bias, u, mean, rstd, slope, act):
        dx, dbias_t = _ext().ln_act_bwd(u, x, mean, rstd, bias, slope, act)
        ctx.save_for_backward(x, bias, u, mean, rstd)
        ctx.slope, ctx.act = slope, act
        return dx, dbias_t

    @staticmethod
    def backward(ctx, gx, gb_t):
        x, bias, u, mean, rstd = ctx.saved_tensors
        d_u, d_x = _ext().ln_act_dbwd(x, u, gx.contiguous(), gb_t, mean, rstd,
                                      bias, ctx.slope, ctx.act)
        return d_x, None, d_u, None, None, None, None


class _LNActFn(torch.autograd.Function):
    """x [T, NS, H, W, C], bias fp32 [D] or [T, D] -> y.  Fused kernels at
    every order."""

    @staticmethod
    def forward(ctx, x, bias, eps, slope, act):
        y, mean, rstd = _ext().ln_act_fwd(x, bias, eps, slope, act)
        ctx.save_for_backward(x, bias, mean, rstd)
        ctx.slope, ctx.act = slope, act
        return y

    @staticmethod
    def backward(ctx, dy):
        x, bias, mean, rstd = ctx.saved_tensors
        dx, dbias_t = _LNBwdFn.apply(x, bias, dy.contiguous(), mean, rstd,
                                     ctx.slope, ctx.act)
        # shared bias: fold the per-task sums over T (outer-dim sum, ordered)
        dbias = dbias_t if bias.dim() == 2 else dbias_t.sum(0)
        return dx, dbias, None, None, None


def task_layer_norm_act(x, bias, eps=1e-5, negative_slope=0.01, apply_act=True):
    """bias: [H, W, C] (shared) or [T, H, W, C] (per-task fast weight)."""
    T, NS, H, W, C = x.shape
    D = H * W * C
    if bias.dim() == 3:
        b2 = bias.reshape(D)
    elif bias.dim() == 4:
        b2 = bias.reshape(T, D)
    else:
        raise ValueError("task_layer_norm_act: bias must be [H, W, C] or "
                         "[T, H, W, C], got %s" % (tuple(bias.shape),))
    return _LNActFn.apply(x.contiguous(), b2.float().contiguous(), eps,
                          negative_slope, apply_act)


# ---------------------------------------------------------------------------
# maxpool 2x2 — mask is fixed after forward, so backward (scatter) and
# double-backward (gather) are both linear custom kernels.
# ---------------------------------------------------------------------------
class _PoolBwdFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dy, mask, H, W):
        ctx.save_for_backward(mask)
        ctx.HW = (H, W)
        return _ext().maxpool2x2_bwd(dy, mask, H, W)

    @staticmethod
    def backward(ctx, ddx):
        (mask,) = ctx.saved_tensors
        # gather: d(dy) = ddx at the argmax positions == pool-forward of ddx
        # restricted to saved argmax — implemented by re-running fwd gather
        if mask.shape[-1] % 8 == 0 and _dbwd_glue_off():
            g = _ext().maxpool2x2_gather(ddx.contiguous(), mask)
        else:
            g = _gather_by_mask(ddx.contiguous(), mask)
        return g, None, None, None


def _gather_by_mask(x4, mask):
    # x4: [N, H, W, C]; mask: [N, Ho, Wo, C] -> [N, Ho, Wo, C]
    N, H, W, C = x4.shape
    Ho, Wo = mask.shape[1], mask.shape[2]
    win = x4[:, :2 * Ho, :2 * Wo, :].reshape(N, Ho, 2, Wo, 2, C)
    win = win.permute(0, 1, 3, 5, 2, 4).reshape(N, Ho, Wo, C, 4)
    return torch.gather(win, 4, mask.long().unsqueeze(-1)).squeeze(-1)


class _PoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x4):
        y, mask = _ext().maxpool2x2_fwd(x4)
        ctx.save_for_backward(mask)
        ctx.HW = (x4.shape[1], x4.shape[2])
        return y

    @staticmethod
    def backward(ctx, dy):
        (mask,) = ctx.saved_tensors
        H, W = ctx.HW
        return _PoolBwdFn.apply(dy.contiguous(), mask, H, W)


def task_maxpool2x2(x):
    T, NS, H, W, C = x.shape
    y = _PoolFn.apply(x.reshape(T * NS, H, W, C).contiguous())
    return y.view(T, NS, H // 2, W // 2, C)


# ---------------------------------------------------------------------------
# global average pool (max_pooling=False backbone) — linear: the backward
# is the broadcast kernel, and the backward of that is the forward kernel
# applied to the incoming grad.
# ---------------------------------------------------------------------------
class _GAvgPoolBwdFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dy, H, W):
        return _ext().gavgpool_bwd(dy, H, W)

    @staticmethod
    def backward(ctx, ddx):
        return _GAvgPoolFn.apply(ddx.contiguous()), None, None


class _GAvgPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x4):
        ctx.HW = (x4.shape[1], x4.shape[2])
        return _ext().gavgpool_fwd(x4)

    @staticmethod
    def backward(ctx, dy):
        H, W = ctx.HW
        return _GAvgPoolBwdFn.apply(dy.contiguous(), H, W)


def task_global_avgpool(x):
    T, NS, H, W, C = x.shape
    y = _GAvgPoolFn.apply(x.reshape(T * NS, H, W, C).contiguous())
    return y.view(T, NS, C)


# ---------------------------------------------------------------------------
# fused softmax-CE
# ---------------------------------------------------------------------------
class _CEBwdFn(torch.autograd.Function):
    """First backward of softmax-CE as a Function: forward = fused bwd
    kernel; backward = softmax-Jacobian double-backward kernel."""

    @staticmethod
    def forward(ctx, logits, gtask, probs, labels):
        ctx.save_for_backward(probs, labels, gtask)
        ctx.out_dtype = logits.dtype
        return _ext().ce_bwd(probs, labels, gtask.contiguous()).to(logits.dtype)

    @staticmethod
    def backward(ctx, gdl):
        probs, labels, gtask = ctx.saved_tensors
        d_logits, d_gtask = _ext().ce_dbwd(probs, labels, gdl.contiguous(),
                                           gtask.contiguous())
        return d_logits.to(ctx.out_dtype), d_gtask, None, None


class _CEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels):
        loss, probs = _ext().ce_fwd(logits, labels)
        ctx.save_for_backward(logits, probs, labels)
        return loss

    @staticmethod
    def backward(ctx, gtask):
        logits, probs, labels = ctx.saved_tensors
        return _CEBwdFn.apply(logits, gtask, probs, labels), None


def softmax_cross_entropy(logits, labels):
    return _CEFn.apply(logits.contiguous(), labels.contiguous())


# ---------------------------------------------------------------------------
# fused LSLR update — backward components are bilinear; custom at all orders
# ---------------------------------------------------------------------------
class _LSLRFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, arena, grad, lr_vec):
        ctx.save_for_backward(grad, lr_vec)
        return _ext().lslr_fwd(arena.contiguous(), grad, lr_vec)

    @staticmethod
    def backward(ctx, gout):
        grad, lr_vec = ctx.saved_tensors
        if torch.is_grad_enabled():
            dgrad = -lr_vec.unsqueeze(0) * gout
            dlr = -(gout * grad).sum(dim=0)
            return gout, dgrad, dlr
        dgrad, dlr = _ext().lslr_bwd(gout, grad, lr_vec)
        return gout, dgrad, dlr


def lslr_update(arena, grad, lr_vec):
    return _LSLRFn.apply(arena, grad.contiguous(), lr_vec.contiguous())


# ---------------------------------------------------------------------------
# conv trio — MFMA implicit GEMM.  The three ops (fwd, dgrad, wgrad) are
# mutually bilinear, so each backward is a composition of the other two:
# custom kernels at EVERY derivative order (second-order MAML's
# create_graph included), no torch fallback on the hot path.  The
# composition is written once; a backend record says which kernels run:
#   fwd(x, w, b, pad, want_stats) -> (y, sums or None)
#   dgrad(dy, w, pad, H, W) -> dx     (H, W explicit: under stride 2 two
#                                      input sizes share one Ho)
#   wgrad(dy, x, pad, with_bias) -> (dw, db)
# ---------------------------------------------------------------------------
_ConvBackend = collections.namedtuple("_ConvBackend", "fwd dgrad wgrad")


class _ConvFwdFn(torch.autograd.Function):
    """Returns (y, bn_sums): with want_stats the bf16 stride-1 epilogue
    accumulates the following BN's per-channel sum/sum-of-squares for free;
    the other backends return no sums (None)."""

    @staticmethod
    def forward(ctx, be, x, w, b, pad, want_stats):
        ctx.save_for_backward(x, w)
        ctx.be, ctx.pad = be, pad
        ctx.has_bias = b is not None
        y, sums = be.fwd(x, w, b, pad, want_stats)
        if sums is not None:
            ctx.mark_non_differentiable(sums)
        return y, sums

    @staticmethod
    def backward(ctx, dy, dsums):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[1]:
            dx = _ConvDgradFn.apply(ctx.be, dy, w, ctx.pad,
                                    x.shape[2], x.shape[3])
        if ctx.needs_input_grad[2]:
            want_bias = ctx.has_bias and ctx.needs_input_grad[3]
            dw, db = _ConvWgradFn.apply(ctx.be, dy, x, ctx.pad, want_bias)
            if not want_bias:
                db = None
        elif ctx.has_bias and ctx.needs_input_grad[3]:
            db = dy.float().sum(dim=(1, 2, 3))
        return None, dx, dw, db, None, None


def _conv_fwd(be, x, w, b, pad):
    return _ConvFwdFn.apply(be, x, w, b, pad, False)[0]


class _ConvDgradFn(torch.autograd.Function):
    """dx = dgrad(dy, w) for an input of size (H, W)."""

    @staticmethod
    def forward(ctx, be, dy, w, pad, H, W):
        ctx.save_for_backward(dy, w)
        ctx.be, ctx.pad = be, pad
        return be.dgrad(dy, w, pad, H, W)

    @staticmethod
    def backward(ctx, g):
        dy, w = ctx.saved_tensors
        g = g.contiguous()
        d_dy = d_w = None
        if ctx.needs_input_grad[1]:
            d_dy = _conv_fwd(ctx.be, g, w, None, ctx.pad)
        if ctx.needs_input_grad[2]:
            d_w = _ConvWgradFn.apply(ctx.be, dy, g, ctx.pad, False)[0]
        return None, d_dy, d_w, None, None, None


class _ConvWgradFn(torch.autograd.Function):
    """(dy, x) -> (dw, db); db is the fused bias gradient (sum of dy over
    positions) — the wgrad kernel already stages the dY tiles, so the
    reduction rides along instead of a separate big ATen sum."""

    @staticmethod
    def forward(ctx, be, dy, x, pad, with_bias):
        ctx.save_for_backward(dy, x)
        ctx.be, ctx.pad = be, pad
        dw, db = be.wgrad(dy, x, pad, with_bias)
        return dw, db

    @staticmethod
    def backward(ctx, gw, gdb):
        dy, x = ctx.saved_tensors
        d_dy = d_x = None
        if ctx.needs_input_grad[1]:
            if gw is not None:
                d_dy = _conv_fwd(ctx.be, x, gw.contiguous(), None, ctx.pad)
            if gdb is not None:
                T, F = gdb.shape
                add = gdb.view(T, 1, 1, 1, F).to(dy.dtype)
                d_dy = add.expand_as(dy).contiguous() if d_dy is None else d_dy + add
        if ctx.needs_input_grad[2] and gw is not None:
            d_x = _ConvDgradFn.apply(ctx.be, dy, gw.contiguous(), ctx.pad,
                                     x.shape[2], x.shape[3])
        return None, d_dy, d_x, None, None


# ---------------------------------------------------------------------------
# backend: bf16 stride 1 — tconv.hip / wgrad_nt.hip / dconv.hip
# ---------------------------------------------------------------------------
def _dconv_ok(ci: int, f: int) -> bool:
    """Direct VALU conv for small input-channel counts (the first layer's
    C in {1,3}); MAML355_NO_DCONV=1 reverts to the GEMM path for A/B."""
    return (ci <= 8 and f in (16, 32, 48, 64)
            and os.environ.get("MAML355_NO_DCONV", "0") != "1")


def _conv_v2_ok(ci: int) -> bool:
    """v2 (async global_load_lds staging, single-buffer default) needs
    8-aligned input channels.  Measured: SBUF v2 beats v1 at every
    flagship shape (conv1 192->222 TF, conv2 146->175, omniglot
    289->312); the 80 KB double-buffer variant (MAML355_CONV_V2_SBUF=0)
    loses to occupancy.  MAML355_CONV_V2=0 reverts to v1."""
    return ci % 8 == 0 and os.environ.get("MAML355_CONV_V2", "1") != "0"


def _wgrad_v3_ok(c: int, f: int) -> bool:
    """Transpose-free wgrad (wgrad_nt.hip): 8-aligned F <= 64, 8-aligned C
    or the first layer's C in {1, 3}.  It has no fixed-cost operand copies,
    so unlike v2 it needs no lower bound on the reduction length (measured
    at or ahead of v1 down to the smallest workload shapes,
    profiles/README.md, "wgrad v3").  MAML355_WGRAD_V3=0 restores the
    v2 / v1 routing."""
    return (f % 8 == 0 and f <= 64 and (c % 8 == 0 or c in (1, 3))
            and os.environ.get("MAML355_WGRAD_V3", "1") != "0")


def _tconv_fwd(x, w, b, pad, want_stats):
    H, W = x.shape[2], x.shape[3]
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    if _dconv_ok(x.shape[4], w.shape[1]):
        # first-layer shapes: direct VALU conv (im2col-MFMA wastes
        # >4x the MACs at K = 9..27)
        y = _ext().dconv_fwd(x, w, b, pad, Ho, Wo)
        return y, torch.empty(0, device=x.device, dtype=torch.float32)
    if _conv_v2_ok(x.shape[4]):
        wp = _ext().tconv_repack_v2(w, False)
        return _ext().tconv_mm_v2(x, wp, b, pad, Ho, Wo, w.shape[1],
                                  want_stats)
    wp = _ext().tconv_repack(w, False)
    return _ext().tconv_mm(x, wp, b, pad, Ho, Wo, want_stats)


def _tconv_dgrad(dy, w, pad, H, W):
    """The fwd kernel run with flipped/transposed repacked weights and
    pad' = 2 - pad (full-correlation identity)."""
    if _conv_v2_ok(dy.shape[4]):
        wp = _ext().tconv_repack_v2(w, True)
        return _ext().tconv_mm_v2(dy, wp, None, 2 - pad, H, W,
                                  w.shape[2], False)[0]
    wp = _ext().tconv_repack(w, True)
    return _ext().tconv_mm(dy, wp, None, 2 - pad, H, W, False)[0]


def _tconv_wgrad(dy, x, pad, with_bias):
    # The direct VALU wgrad (dconv_wgrad) measured 2.3x SLOWER than v2 at
    # the conv0 shape (serial position walk per wave) — opt-in only.
    if (x.shape[4] <= 8 and dy.shape[4] <= 64
            and os.environ.get("MAML355_DCONV_WGRAD", "0") == "1"):
        return _ext().dconv_wgrad(dy, x, pad, with_bias)
    if _wgrad_v3_ok(x.shape[4], dy.shape[4]):
        # v3: both operands staged as stored, the transpose moved into
        # the LDS read — none of v2's operand copies
        return _ext().tconv_wgrad_v3(dy, x, pad, with_bias)
    if (dy.shape[4] <= 64
            and dy.shape[1] * dy.shape[2] * dy.shape[3] >= 30000
            and os.environ.get("MAML355_WGRAD_V2", "1") != "0"):
        # v2 (global transposes -> linear async staging, any Wo).  Its
        # operand transposes are fixed cost: below ~30k reduction
        # positions the v1 gather kernel wins (measured on the omniglot
        # target passes: whole-bench +3% with v1 there)
        return _ext().tconv_wgrad_v2(dy, x, pad, with_bias)
    return _ext().tconv_wgrad(dy, x, pad, with_bias)


_TCONV = _ConvBackend(_tconv_fwd, _tconv_dgrad, _tconv_wgrad)


# ---------------------------------------------------------------------------
# backend: bf16 stride 2 (max_pooling=False backbone) — sconv.hip.  dgrad is
# four parity sub-GEMMs in one launch.  No BN-stats epilogue.
# ---------------------------------------------------------------------------
def _sconv_fwd(x, w, b, pad, want_stats):
    wp = _ext().sconv_repack(w, False)
    return _ext().sconv_fwd(x, wp, b, pad), None


def _sconv_dgrad(dy, w, pad, H, W):
    wp = _ext().sconv_repack(w, True)
    return _ext().sconv_dgrad(dy, wp, pad, H, W)


def _sconv_wgrad(dy, x, pad, with_bias):
    return _ext().sconv_wgrad(dy, x, pad, with_bias)


_SCONV = _ConvBackend(_sconv_fwd, _sconv_dgrad, _sconv_wgrad)


# ---------------------------------------------------------------------------
# backend: fp32 stride 1 — fconv.hip.  Weights are used unrounded; C and F
# are any value in 1..64 (no channel padding); wgrad is always the ordered
# private-slice reduction, so the trio is bitwise reproducible in every
# mode.  No BN-stats epilogue.
# ---------------------------------------------------------------------------
def _fconv_on() -> bool:
    """MAML355_FCONV=0 restores the pre-kernel fp32 behaviour (grouped-ATen
    conv, torch.bmm linear head) for A/B runs."""
    return os.environ.get("MAML355_FCONV", "1") != "0"


def _fconv_fwd(x, w, b, pad, want_stats):
    H, W = x.shape[2], x.shape[3]
    wp = _ext().fconv_repack(w, False)
    return _ext().fconv_mm(x, wp, b, pad, H + 2 * pad - 2, W + 2 * pad - 2), None


def _fconv_dgrad(dy, w, pad, H, W):
    """fconv_mm with flipped/transposed repacked weights and pad' = 2 - pad."""
    wp = _ext().fconv_repack(w, True)
    return _ext().fconv_mm(dy, wp, None, 2 - pad, H, W)


def _fconv_wgrad(dy, x, pad, with_bias):
    return _ext().fconv_wgrad(dy, x, pad, with_bias)


_FCONV = _ConvBackend(_fconv_fwd, _fconv_dgrad, _fconv_wgrad)


_FALLBACK_WARNED = set()


def _warn_fallback(reason: str) -> None:
    if reason not in _FALLBACK_WARNED:
        _FALLBACK_WARNED.add(reason)
        import warnings
        warnings.warn(
            f"maml355: task_conv3x3 using the grouped-ATen composition on GPU "
            f"({reason}); the MFMA kernel path does not cover this shape/config.",
            stacklevel=3)


def task_conv3x3(x, w, b=None, stride=1, padding=1, return_stats=False):
    # w is task-batched [T, F, C, 3, 3]: dim 1 = out-channels, dim 2 = in
    if (x.dtype == torch.float32 and stride == 1 and padding in (0, 1)
            and w.shape[1] <= 64 and w.shape[2] <= 64 and _fconv_on()):
        # fp32 activations: the fp32 MFMA trio, weights and bias unrounded.
        # No BN-stats epilogue: return_stats yields empty sums and the BN
        # kernels compute their own statistics, as on the stride-2 path.
        y = _ConvFwdFn.apply(_FCONV, x.contiguous(), w.float().contiguous(),
                             b.float().contiguous() if b is not None else None,
                             padding, False)[0]
        if return_stats:
            return y, torch.empty(0, device=x.device, dtype=torch.float32)
        return y
    strided_ok = stride == 2 and padding in (0, 1)
    if (not (stride == 1 or strided_ok) or x.dtype != torch.bfloat16
            or w.shape[1] > 64 or w.shape[2] > 64):
        # strides other than 1/2, fp32 compute and >64-channel shapes use
        # the grouped-ATen composition; loud, not silent
        if not (stride == 1 or strided_ok):
            _warn_fallback(f"stride {stride}, padding {padding}")
        elif x.dtype != torch.bfloat16:
            _warn_fallback(f"dtype {x.dtype}")
        else:
            _warn_fallback(f"channels > 64 (F={w.shape[1]}, C={w.shape[2]})")
        wc = w.to(x.dtype)
        bc = b.to(x.dtype) if b is not None else None
        y = ref.task_conv3x3(x, wc, bc, stride, padding)
        return (y, None) if return_stats else y
    C, F = w.shape[2], w.shape[1]
    if stride == 2:
        # max_pooling=False backbone: the stride-2 MFMA trio.  First-layer
        # C in {1,3} is zero-padded to 8 channels (vector staging), as for
        # stride 1.  No BN-stats epilogue here: return_stats yields no sums.
        if C < 8:
            x = torch.nn.functional.pad(x, (0, 8 - C))
            w = torch.nn.functional.pad(w, (0, 0, 0, 0, 0, 8 - C))
        y = _ConvFwdFn.apply(_SCONV, x.contiguous(), w.contiguous(),
                             b.contiguous() if b is not None else None,
                             padding, False)[0]
        return (y, None) if return_stats else y
    if C < 8 and not _dconv_ok(C, F):
        # small C without a direct-kernel instantiation: zero-pad to 8 so
        # the vectorized 8-channel GEMM staging applies.  F.pad is
        # differentiable, so dw/dx slicing back to C channels is automatic.
        x = torch.nn.functional.pad(x, (0, 8 - C))
        w = torch.nn.functional.pad(w, (0, 0, 0, 0, 0, 8 - C))
    y, sums = _ConvFwdFn.apply(_TCONV, x.contiguous(), w.contiguous(),
                               b.contiguous() if b is not None else None,
                               padding, return_stats)
    return (y, sums) if return_stats else y


# ---------------------------------------------------------------------------
# linear head trio — the ops are mutually bilinear (like the convs), so
# each backward composes the other two: custom kernels at every order.
# Replaces torch.bmm (hipBLASLt autotunes on first call: run #1 of a
# process differed from runs #2+ — measured 5e-3 theta drift).
# ---------------------------------------------------------------------------
class _LinFwdFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_b = b is not None
        return _ext().lin_fwd(x, w, b)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = _LinDxFn.apply(dy, w)
        want_db = ctx.has_b and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_db:
            dw_, db_ = _LinWgradFn.apply(dy, x, want_db)
            if ctx.needs_input_grad[1]:
                dw = dw_
            if want_db:
                db = db_
        return dx, dw, db


class _LinDxFn(torch.autograd.Function):
    """dx = dy @ bf16(w) — bilinear in (dy, w)."""

    @staticmethod
    def forward(ctx, dy, w):
        ctx.save_for_backward(dy, w)
        return _ext().lin_dx(dy, w)

    @staticmethod
    def backward(ctx, g):
        dy, w = ctx.saved_tensors
        g = g.contiguous()
        d_dy = d_w = None
        if ctx.needs_input_grad[0]:
            d_dy = _LinFwdFn.apply(g, w, None)
        if ctx.needs_input_grad[1]:
            d_w = _LinWgradFn.apply(dy, g, False)[0]
        return d_dy, d_w


class _LinWgradFn(torch.autograd.Function):
    """(dy, x) -> (dw = dy^T @ x, db = sum dy) — bilinear in (dy, x)."""

    @staticmethod
    def forward(ctx, dy, x, with_bias):
        ctx.save_for_backward(dy, x)
        dw, db = _ext().lin_wgrad(dy, x, with_bias)
        return dw, db

    @staticmethod
    def backward(ctx, gw, gdb):
        dy, x = ctx.saved_tensors
        d_dy = d_x = None
        if ctx.needs_input_grad[0]:
            if gw is not None:
                d_dy = _LinFwdFn.apply(x, gw.contiguous(), None)
            if gdb is not None:
                add = gdb.unsqueeze(1).to(dy.dtype)
                d_dy = add.expand_as(dy).contiguous() if d_dy is None else d_dy + add
        if ctx.needs_input_grad[1] and gw is not None:
            d_x = _LinDxFn.apply(dy, gw.contiguous())
        return d_dy, d_x, None


def task_linear(x, w, b=None):
    if x.dtype == torch.float32 and _fconv_on():
        # fp32 activations: the same kernel trio, w/b unrounded, fp32 out
        return _LinFwdFn.apply(x.contiguous(), w, b)
    if x.dtype != torch.bfloat16:
        # MAML355_FCONV=0 (or another dtype): torch composition
        return ref.task_linear(x, w.to(x.dtype), b.to(x.dtype) if b is not None else None)
    return _LinFwdFn.apply(x.contiguous(), w, b)


def fused_adam_step(params, grads, exp_avgs, exp_avg_sqs, step, lr,
                    beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, clamp=None):
    """One launch for the whole meta-update: multi-tensor Adam with the
    reference's pre-clamp fused in (few_shot_learning_system.py:330-336)."""
    keep = [i for i, g in enumerate(grads) if g is not None]
    if not keep:
        return
    ps = [params[i].data.view(-1) for i in keep]
    gs = [grads[i].contiguous().view(-1).float() for i in keep]
    ms = [exp_avgs[i].view(-1) for i in keep]
    vs = [exp_avg_sqs[i].view(-1) for i in keep]
    _ext().adam_step(ps, gs, ms, vs, int(step), float(lr), float(beta1),
                     float(beta2), float(eps), float(weight_decay),
                     float(clamp) if clamp is not None else -1.0)
