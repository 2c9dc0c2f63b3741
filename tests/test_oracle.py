"""CPU check of the float64 oracle (tests/_oracle.py) that the GPU kernel
tests compare against: it must agree with ``ops.reference`` in fp32, and the
discrete-decision exclusions it computes must stay below the share the GPU
tests allow."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _head_cases as hc
import _oracle as orc
from howtotrainyourmamlpytorch_amd import ops
from howtotrainyourmamlpytorch_amd.ops import reference as ref

SHAPES = [(2, 3, 25, 27, 48), (2, 5, 21, 21, 64)]


def _inputs(shape, seed, offset=0.0, dtype=torch.float32):
    T, NS, H, W, C = shape
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(*shape, generator=g) + offset).to(dtype)
    gamma = torch.rand(T, C, generator=g) + 0.5
    beta = torch.randn(T, C, generator=g)
    return x, gamma, beta


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_oracle_matches_reference_fp32(shape):
    T, NS, H, W, C = shape
    x, gamma, beta = _inputs(shape, seed=sum(shape))

    # BN + act, forward and first backward
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    yr, mr, vr = ref.task_bn_act(xr, gr, br)
    xo, go, bo = (orc.widen(t).requires_grad_(True) for t in (x, gamma, beta))
    yo, mo, vo, pre = orc.bn_act(xo, go, bo)
    torch.testing.assert_close(yr.double(), yo, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(mr.double(), mo, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(vr.double(), vo, rtol=1e-5, atol=1e-6)
    u = torch.randn(*shape, generator=torch.Generator().manual_seed(1))
    gr_ = torch.autograd.grad(yr, (xr, gr, br), u)
    go_ = torch.autograd.grad(yo, (xo, go, bo), u.double())
    keep = ~orc.near_zero(pre)
    torch.testing.assert_close(gr_[0].double()[keep], go_[0][keep],
                               rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(gr_[1].double(), go_[1], rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(gr_[2].double(), go_[2], rtol=1e-4, atol=1e-3)

    # apply_act=False is the pre-activation
    ypre = ref.task_bn_act(x, gamma, beta, apply_act=False)[0]
    torch.testing.assert_close(ypre.double(), pre.detach(), rtol=1e-5, atol=1e-5)

    # pool: values and routing (randn fp32 has no ties)
    xp = x.clone().requires_grad_(True)
    yp = ref.task_maxpool2x2(xp)
    xq = orc.widen(x).requires_grad_(True)
    yq, arg = orc.pool2x2(xq)
    assert (yp.double() == yq).all().item()
    gy = torch.randn_like(yp)
    (dxp,) = torch.autograd.grad(yp, xp, gy)
    (dxq,) = torch.autograd.grad(yq, xq, gy.double())
    assert (dxp.double() == dxq).all().item()
    assert (dxq[:, :, 2 * (H // 2):] == 0).all().item()

    # fused op == composition of the two
    yf, _, _, _, argf = orc.bn_act_pool(xo, go, bo)
    yc = ref.task_maxpool2x2(yr)
    torch.testing.assert_close(yc.double(), yf, rtol=1e-5, atol=1e-5)

    # conv, both strides, on a cut of the same input
    Fo = 16
    xc = x[:, :, :11, :9, :8].contiguous()
    w = torch.randn(T, Fo, 8, 3, 3, generator=torch.Generator().manual_seed(2))
    b = torch.randn(T, Fo, generator=torch.Generator().manual_seed(3))
    for stride, pad in ((1, 1), (1, 0), (2, 1), (2, 0)):
        yr_ = ref.task_conv3x3(xc, w, b, stride, pad)
        yo_ = orc.conv3x3(orc.widen(xc), orc.widen(w), orc.widen(b), stride, pad)
        torch.testing.assert_close(yr_.double(), yo_, rtol=1e-5, atol=1e-5)


def test_oracle_first_maximum_wins():
    # windows in the order (0,0), (0,1), (1,0), (1,1); ties -> lowest index
    x = torch.tensor([[1., 2., 0., 0.],
                      [2., 2., 0., 0.],
                      [5., 1., 3., 7.],
                      [1., 5., 7., 3.]], dtype=torch.float64)
    x = x.view(1, 1, 4, 4, 1).requires_grad_(True)
    y, arg = orc.pool2x2(x)
    assert y.flatten().tolist() == [2., 0., 5., 7.]
    assert arg.flatten().tolist() == [1, 0, 0, 1]
    (dx,) = torch.autograd.grad(y.sum(), x)
    want = torch.tensor([[0., 1., 1., 0.],
                         [0., 0., 0., 0.],
                         [1., 0., 0., 1.],
                         [0., 0., 0., 0.]], dtype=torch.float64)
    assert (dx.view(4, 4) == want).all().item()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("offset", [0.0, 3.0])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exclusion_shares(shape, offset, dtype):
    """The two exclusions of the GPU tests each cover less than 1e-3 of
    their cases; bf16 inputs do produce exact ties, which stay in."""
    T, NS, H, W, C = shape
    x, gamma, beta = _inputs(shape, seed=7 + sum(shape), offset=offset, dtype=dtype)
    _, _, _, pre, _ = orc.bn_act_pool(orc.widen(x), orc.widen(gamma), orc.widen(beta))
    nz = orc.share(orc.near_zero(pre))
    nt = orc.share(orc.near_tied_windows(pre))
    top = orc.windows(pre).topk(2, dim=-1).values
    exact = orc.share(top[..., 0] == top[..., 1])
    print(f"near-zero {nz:.2e}  near-tied {nt:.2e}  exact ties {exact:.2e}")
    assert nz <= orc.MAX_EXCLUDED
    assert nt <= orc.MAX_EXCLUDED
    if dtype == torch.bfloat16:
        assert exact > 0


# ---------------------------------------------------------------------------
# head, loss and update kernels: the oracle's new functions, and every bound
# of test_head_loss_update_gpu.py applied first to ops.reference in fp32 on
# the CPU, at the same cases — no bound is tighter than fp32 arithmetic allows
# ---------------------------------------------------------------------------
def test_new_oracle_functions_match_reference_in_float64():
    g = torch.Generator().manual_seed(3)
    kw = dict(rtol=1e-12, atol=0.0)
    # CE: ops.reference casts its logits to fp32, so float64 agreement is
    # with the op it wraps; the reference itself agrees at fp32 precision
    logits = torch.randn(3, 7, 20, generator=g, dtype=torch.float64) * 4
    labels = torch.randint(0, 20, (3, 7), generator=g)
    want = F.cross_entropy(logits.reshape(21, 20), labels.reshape(21),
                           reduction="none").view(3, 7).mean(dim=1)
    torch.testing.assert_close(orc.softmax_ce(logits, labels), want, **kw)
    torch.testing.assert_close(orc.softmax_ce(logits, labels.to(torch.int32)), want, **kw)
    torch.testing.assert_close(ref.softmax_cross_entropy(logits, labels).double(),
                               want, rtol=1e-5, atol=1e-6)
    x, w, b = (torch.randn(*s, generator=g, dtype=torch.float64)
               for s in ((2, 5, 9), (2, 3, 9), (2, 3)))
    torch.testing.assert_close(orc.linear(x, w, b), ref.task_linear(x, w, b), **kw)
    a, gr, lr = (torch.randn(*s, generator=g, dtype=torch.float64)
                 for s in ((3, 11), (3, 11), (11,)))
    torch.testing.assert_close(orc.lslr(a, gr, lr), ref.lslr_update(a, gr, lr), **kw)
    # Adam: the reference casts g (and, for the decay, p) to fp32, so g is
    # fp32-representable, and in the decay case g + 0.25 p is exact in fp32
    # (g in quarters, p integer); everything else it does in float64
    for clamp, decay in ((None, 0.0), (1.5, 0.0), (1.5, 0.25)):
        gd, m, v = (torch.randn(50, generator=g).double() for _ in range(3))
        gd, v = gd * 4, v.abs()
        p = torch.randn(50, generator=g).double()
        if decay:
            gd = torch.randint(-12, 13, (50,), generator=g).double() / 4
            p = torch.randint(-8, 9, (50,), generator=g).double()
        want = orc.adam_step(p, gd, m, v, 7, 0.1, 0.9, 0.999, 1e-8, decay, clamp)
        pr, mr, vr = p.clone(), m.clone(), v.clone()
        ref.fused_adam_step([pr], [gd.clone()], [mr], [vr], step=7, lr=0.1,
                            weight_decay=decay, clamp=clamp)
        for a_, r_ in zip((pr, mr, vr), want):
            torch.testing.assert_close(a_, r_, **kw)


def test_adam_oracle_clamps_before_it_decays():
    one = lambda x: torch.tensor([x], dtype=torch.float64)  # noqa: E731
    _, m, _ = orc.adam_step(one(100.0), one(5.0), one(0.0), one(0.0), 1, 0.1,
                            0.9, 0.999, 1e-8, weight_decay=0.01, clamp=1.5)
    # clamp(5) + 0.01 * 100 = 2.5, not clamp(5 + 1) = 1.5
    torch.testing.assert_close(m, one((1 - 0.9) * 2.5), rtol=1e-14, atol=0.0)


# ---- the fp32 stand-ins ----------------------------------------------------
def _linear_fp32(x, w, b):
    """fp32 reference with the kernel's roundings: w and b rounded to bf16
    (straight-through, so dw and db stay fp32), y and dx rounded to bf16."""
    st = lambda t: t + (t.detach().to(torch.bfloat16).float() - t.detach())  # noqa: E731
    return ref.task_linear(x.float(), st(w), st(b) if b is not None else None
                           ).to(torch.bfloat16)


def _ce_fp32(logits, labels):
    return ref.softmax_cross_entropy(logits, labels.long())


def _lslr_fp32(arena, grad, lr_vec):
    """The reference rounds the product and the difference; the kernel's
    forward is one fma, and its bound 2^-24 |ref| is that of one rounding.
    The value is therefore the fma (the fp32 product is exact in float64),
    the graph the reference's.  A float64 result rounded once meets that
    bound by construction: the forward half of the LSLR pre-check says
    nothing about the bound, only its backward halves do."""
    out = ref.lslr_update(arena, grad, lr_vec)
    fma = (arena.double() - lr_vec.double().unsqueeze(0) * grad.double()).float()
    return out + (fma - out).detach()


@pytest.mark.parametrize("shape", hc.LINEAR_SHAPES, ids=hc._id)
def test_fp32_reference_inside_linear_bounds(shape):
    hc.check_linear_first_order(_linear_fp32, shape, hc.CPU)
    hc.check_linear_exact(_linear_fp32, shape, hc.CPU)


@pytest.mark.parametrize("shape", hc.LINEAR_SECOND_ORDER_SHAPES, ids=hc._id)
def test_bf16_reference_inside_linear_second_order_figures(shape):
    """ops.task_linear on the CPU with bf16 activations (bf16 weights, bf16
    outputs) against the fp32 reference on widened inputs."""
    x, w, b, _ = hc.linear_inputs(shape + (True,))
    got = hc.linear_second_order(ops.task_linear, x, w, b, hc.CPU)
    want = hc.linear_second_order(ref.task_linear, x.float(), w, b, hc.CPU)
    for a, r in zip(got, want):
        torch.testing.assert_close(a, r, rtol=8e-2,
                                   atol=5e-2 * max(r.abs().max().item(), 1e-3))


@pytest.mark.parametrize("case", hc.CE_CASES, ids=hc._id)
def test_fp32_reference_inside_ce_bounds(case):
    hc.check_ce(_ce_fp32, case, hc.CPU)


@pytest.mark.parametrize("create_graph", [False, True], ids=["nograd", "create_graph"])
@pytest.mark.parametrize("shape", hc.LSLR_SHAPES, ids=hc._id)
def test_fp32_reference_inside_lslr_bounds(shape, create_graph):
    hc.check_lslr(_lslr_fp32, shape, hc.CPU, create_graph)


def test_fp32_reference_inside_lslr_second_order_bound():
    hc.check_lslr_second_order(_lslr_fp32, hc.CPU)


@pytest.mark.parametrize("case", hc.ADAM_CASES, ids=hc._id)
def test_fp32_reference_inside_adam_bounds(case):
    hc.check_adam(ref.fused_adam_step, case, hc.CPU)


@pytest.mark.parametrize("clamp,decay", [(None, 0.0), (1.5, hc.DECAY)],
                         ids=["plain", "clamp-decay"])
def test_fp32_reference_inside_fused_adam_optimizer_bounds(clamp, decay):
    hc.check_fused_adam_optimizer(hc.CPU, clamp, decay)


@pytest.mark.parametrize("step", hc.ADAM_STEPS)
def test_fp32_bias_correction_inside_its_term(step):
    """adam.hip forms ``1 - powf(float(beta), step)`` in fp32; emulated
    here with numpy float32 and held to d1, d2 of orc.adam_bias_terms."""
    d1, d2, e_bc = orc.adam_bias_terms(hc.BETA1, hc.BETA2, step)
    print(f"step {step}: d1={d1:.3e} d2={d2:.3e} e_bc={e_bc:.3e}")
    for beta, d in ((hc.BETA1, d1), (hc.BETA2, d2)):
        got = np.float32(1.0) - np.power(np.float32(beta), np.float32(step))
        assert got.dtype == np.float32
        err = abs(float(got) - (1.0 - beta ** step))
        print(f"  beta={beta:.9f}: bc={float(got):.9e} err={err:.3e} err/d={err / d:.3f}")
        assert err <= d
