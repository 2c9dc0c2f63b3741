"""BN family (bn_act.hip, bn_dbwd.hip) at the shapes the workloads reach:
cross-block reductions with ragged tails, odd H/W, the scalar (C % 8 != 0)
path, apply_act=False, bf16 backward and double-backward, offset-mean
inputs, the fused BN+act+pool op at odd sizes and the second trip of the
grid-stride loops.

fp32 runs go through autograd and are compared with ``ops.reference`` at
the tolerances of tests/test_ops_gpu.py.  bf16 runs call the kernels
directly and are compared with the exact-input float64 oracle
(tests/_oracle.py): fp32 results to rtol 1e-4 / atol 1e-2, bf16 results to
one bf16 ulp plus the absolute tolerance of the fp32 test of the same
quantity (1e-5 fwd, 1e-4 bwd, 1e-3 dbwd).  Elements whose leaky-ReLU side
or pool argmax is within 1e-4 of undecided are left out of the dx/routing
comparisons only, and may be at most 1e-3 of the cases."""

import pytest
import torch

pytestmark = pytest.mark.gpu

import _oracle as orc
from howtotrainyourmamlpytorch_amd import ops
from howtotrainyourmamlpytorch_amd.ops import hip_autograd
from howtotrainyourmamlpytorch_amd.ops import reference as ref

EPS, SLOPE = 1e-5, 0.01
A_FWD, A_BWD, A_DBWD = 1e-5, 1e-4, 1e-3


def dev():
    return torch.device("cuda", 0)


def _id(s):
    return "x".join(map(str, s))


# (T, NS, H, W, C): each the smallest reaching its mode
VEC_SHAPES = (
    # M = 2025: two 1024-row blocks (ragged second), eight 256-row blocks
    # (ragged last); rows per block 256, 85, 42, 32, 28
    [(2, 3, 25, 27, c) for c in (8, 24, 48, 64, 72)]
    + [(2, 1, 3, 3, 48), (2, 5, 3, 3, 64)]      # M = 9 < row groups
    + [(2, 5, 21, 21, 48), (2, 5, 7, 7, 64)]    # the workloads' odd stages
)
SCALAR_SHAPES = [(2, 3, 9, 7, 5), (2, 3, 9, 7, 65), (1, 2, 40, 41, 5)]
# > 1 048 576 elements: second trip of the grid-stride loops
# (bn_dbwd_apply_kernel; C = 65: the scalar norm / dx kernels)
BIG_SHAPES = [(1, 1, 130, 127, 64), (1, 1, 130, 127, 65)]
ALL_SHAPES = VEC_SHAPES + SCALAR_SHAPES + BIG_SHAPES


def _mk(shape, dtype, per_task, seed, offset=0.0, std=1.0):
    T, NS, H, W, C = shape
    g = torch.Generator().manual_seed(seed)
    x = (offset + std * torch.randn(*shape, generator=g)).to(dtype)
    gamma = torch.rand(*((T, C) if per_task else (C,)), generator=g) + 0.5
    beta = torch.randn(*((T, C) if per_task else (C,)), generator=g)
    return x, gamma, beta


def _per_task(p, T):
    """[C] or [T, C] fp32 -> float64 [T, C] leaf (per-task grads)."""
    p = orc.widen(p)
    if p.dim() == 1:
        p = p.unsqueeze(0).expand(T, -1)
    return p.clone().requires_grad_(True)


def _fold(g_t, per_task):
    return g_t if per_task else g_t.sum(0)


def _keep(pre, apply_act=True):
    """Elements kept in a dx comparison, with the share assertion."""
    if not apply_act:
        return None
    nz = orc.near_zero(pre)
    assert orc.share(nz) <= orc.MAX_EXCLUDED, orc.share(nz)
    return ~nz


# ---------------------------------------------------------------------------
# fp32 through autograd vs ops.reference
# ---------------------------------------------------------------------------
def _second_order_loss(op, x, g, b, act, M):
    """Depends on dx, dgamma and dbeta together: ggam and gbet non-zero.
    Scaled so that every upstream grad is O(1)."""
    y, _, _ = op(x, g, b, EPS, SLOPE, act)
    l1 = (y.float() ** 2).sum() / 2
    gx, gg, gb = torch.autograd.grad(l1, (x, g, b), create_graph=True)
    return ((gx.float() ** 2).sum() / 2
            + ((gg ** 2).sum() + (gb ** 2).sum()) / (2 * M ** 0.5))


def _run_fp32_autograd(shape, per_task, act, seed, offset=0.0, std=1.0):
    T, NS, H, W, C = shape
    M = NS * H * W
    x, gamma, beta = _mk(shape, torch.float32, per_task, seed, offset, std)
    u = torch.randn(*shape, generator=torch.Generator().manual_seed(seed + 1))
    pre = orc.bn_act(orc.widen(x), orc.widen(gamma), orc.widen(beta),
                     EPS, SLOPE, act)[3]
    keep = _keep(pre, act)

    def leaves(d):
        return [t.clone().to(d).requires_grad_(True) for t in (x, gamma, beta)]

    xg, gg, bg = leaves(dev())
    xr, gr, br = leaves("cpu")
    y, mean, var = ops.task_bn_act(xg, gg, bg, EPS, SLOPE, act)
    yr, mr, vr = ref.task_bn_act(xr, gr, br, EPS, SLOPE, act)
    orc.assert_close(y, yr, 1e-5, 1e-5, name="y")
    orc.assert_close(mean, mr, 1e-5, 1e-5, name="mean")
    orc.assert_close(var, vr, 1e-5, 1e-5, name="var")

    d = torch.autograd.grad(y, (xg, gg, bg), u.to(dev()))
    dr = torch.autograd.grad(yr, (xr, gr, br), u)
    orc.assert_close(d[0], dr[0], 1e-4, 1e-4, keep=keep, name="dx")
    orc.assert_close(d[1], dr[1], 1e-4, 1e-3, name="dgamma")
    orc.assert_close(d[2], dr[2], 1e-4, 1e-3, name="dbeta")

    tol = 2e-3 if per_task else 1e-3
    xg, gg, bg = leaves(dev())
    xr, gr, br = leaves("cpu")
    dd = torch.autograd.grad(
        _second_order_loss(ops.task_bn_act, xg, gg, bg, act, M), (xg, gg, bg))
    ddr = torch.autograd.grad(
        _second_order_loss(ref.task_bn_act, xr, gr, br, act, M), (xr, gr, br))
    orc.assert_close(dd[0], ddr[0], tol, tol, keep=keep, name="dd/dx")
    orc.assert_close(dd[1], ddr[1], tol, tol, name="dd/dgamma")
    orc.assert_close(dd[2], ddr[2], tol, tol, name="dd/dbeta")
    for t in ddr[1:]:
        assert t.abs().max().item() > 0


@pytest.mark.parametrize("per_task", [False, True], ids=["shared", "pertask"])
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_id)
def test_bn_act_fp32_autograd_all_orders(shape, per_task):
    _run_fp32_autograd(shape, per_task, True, seed=100 + sum(shape))


@pytest.mark.parametrize("per_task", [False, True], ids=["shared", "pertask"])
@pytest.mark.parametrize("shape", [(2, 3, 25, 27, 48), (2, 3, 9, 7, 5)], ids=_id)
def test_bn_no_act_fp32_autograd_all_orders(shape, per_task):
    """apply_act=False: the ACT=false templates of fwd, bwd and dbwd."""
    _run_fp32_autograd(shape, per_task, False, seed=200 + sum(shape))


# ---------------------------------------------------------------------------
# bf16, kernels called directly, vs the exact-input oracle
# ---------------------------------------------------------------------------
def _run_bf16_kernels(shape, per_task, act, seed, offset=0.0, std=1.0,
                      dbwd=True):
    T, NS, H, W, C = shape
    M = NS * H * W
    ext = ops.hip_ext()
    x, gamma, beta = _mk(shape, torch.bfloat16, per_task, seed, offset, std)
    g = torch.Generator().manual_seed(seed + 1)
    u = torch.randn(*shape, generator=g).to(torch.bfloat16)
    gx = torch.randn(*shape, generator=g).to(torch.bfloat16)
    ggam = torch.randn(T, C, generator=g)
    gbet = torch.randn(T, C, generator=g)

    x3, u3, gx3 = (t.to(dev()).view(T, M, C) for t in (x, u, gx))
    gd, bd, ggd, gbd = (t.to(dev()) for t in (gamma, beta, ggam, gbet))
    y, mean, var, rstd = ext.bn_act_fwd(x3, gd, bd, EPS, SLOPE, act)
    dx, dgam_t, dbet_t = ext.bn_act_bwd(u3, x3, mean, rstd, gd, bd, SLOPE, act)

    xo = orc.widen(x).requires_grad_(True)
    uo = orc.widen(u).requires_grad_(True)
    go, bo = _per_task(gamma, T), _per_task(beta, T)
    yo, mo, vo, pre = orc.bn_act(xo, go, bo, EPS, SLOPE, act)
    keep = _keep(pre, act)
    dxo, dgo, dbo = torch.autograd.grad(yo, (xo, go, bo), uo, create_graph=True)

    assert y.dtype == torch.bfloat16 and dx.dtype == torch.bfloat16
    orc.assert_bf16_close(y.view(shape), yo, A_FWD, name="y")
    orc.assert_f32_close(mean, mo, "mean")
    orc.assert_f32_close(var, vo, "var")
    orc.assert_bf16_close(dx.view(shape), dxo, A_BWD, keep=keep, name="dx")
    orc.assert_f32_close(dgam_t, dgo, "dgamma_t")
    orc.assert_f32_close(dbet_t, dbo, "dbeta_t")
    if not dbwd:
        return mean, var, mo, vo, xo

    d_u, d_x, _ = ext.bn_act_dbwd(x3, u3, gx3, mean, rstd, gd, bd, ggd, gbd,
                                  SLOPE, act)
    # d_gamma as _BNBwdFn.backward forms it from the returned sums
    gleaf = gd.clone().requires_grad_(True)
    outs = hip_autograd._BNBwdFn.apply(x3, gleaf, bd, u3, mean, rstd, SLOPE, act)
    (d_gamma,) = torch.autograd.grad(outs, gleaf, (gx3, ggd, gbd))

    L = ((dxo * orc.widen(gx)).sum() + (dgo * orc.widen(ggam)).sum()
         + (dbo * orc.widen(gbet)).sum())
    d_uo, d_xo, d_go = torch.autograd.grad(L, (uo, xo, go))
    orc.assert_bf16_close(d_u.view(shape), d_uo, A_DBWD, keep=keep, name="d_u")
    orc.assert_bf16_close(d_x.view(shape), d_xo, A_DBWD, keep=keep, name="d_x")
    orc.assert_f32_close(d_gamma, _fold(d_go, per_task), "d_gamma")
    return mean, var, mo, vo, xo


@pytest.mark.parametrize("per_task", [False, True], ids=["shared", "pertask"])
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_id)
def test_bn_kernels_bf16_match_oracle(shape, per_task):
    _run_bf16_kernels(shape, per_task, True, seed=300 + sum(shape))


@pytest.mark.parametrize("shape", [(2, 3, 25, 27, 48), (2, 3, 9, 7, 5)], ids=_id)
def test_bn_no_act_kernels_bf16_match_oracle(shape):
    _run_bf16_kernels(shape, True, False, seed=400 + sum(shape))


# ---------------------------------------------------------------------------
# offset mean: E[x^2] - mean^2 in fp32
# ---------------------------------------------------------------------------
def _var_bound_check(var, vo, xo):
    """|var - var_ref| <= 8 * 2^-24 * E[x^2]: the cancellation bound of the
    E[x^2] - mean^2 form."""
    ex2 = (xo.detach() ** 2).mean(dim=(1, 2, 3))
    err = (var.detach().cpu().double() - vo.detach()).abs()
    bound = 8 * 2.0 ** -24 * ex2
    print(f"var: max|err|={err.max().item():.3e} bound={bound.min().item():.3e} "
          f"worst err/bound={(err / bound).max().item():.3f}")
    assert (err <= bound).all().item(), (err / bound).max().item()


def test_bn_offset_mean_bf16():
    shape = (2, 3, 25, 27, 48)
    mean, var, mo, vo, xo = _run_bf16_kernels(shape, True, True, seed=500,
                                              offset=3.0, std=0.5, dbwd=False)
    _var_bound_check(var, vo, xo)


def test_bn_offset_mean_fp32():
    shape = (2, 3, 25, 27, 48)
    T, NS, H, W, C = shape
    x, gamma, beta = _mk(shape, torch.float32, True, 501, offset=3.0, std=0.5)
    u = torch.randn(*shape, generator=torch.Generator().manual_seed(502))
    xg, gg, bg = (t.clone().to(dev()).requires_grad_(True) for t in (x, gamma, beta))
    y, mean, var = ops.task_bn_act(xg, gg, bg, EPS, SLOPE, True)
    dx, dgam, dbet = torch.autograd.grad(y, (xg, gg, bg), u.to(dev()))

    xo = orc.widen(x).requires_grad_(True)
    go, bo = _per_task(gamma, T), _per_task(beta, T)
    yo, mo, vo, pre = orc.bn_act(xo, go, bo, EPS, SLOPE, True)
    dxo, dgo, dbo = torch.autograd.grad(yo, (xo, go, bo), orc.widen(u))
    _var_bound_check(var, vo, xo)
    orc.assert_close(mean, mo, 1e-5, 1e-5, name="mean")
    orc.assert_close(y, yo, 1e-5, 1e-5, name="y")
    orc.assert_close(dx, dxo, 1e-4, 1e-4, keep=_keep(pre), name="dx")
    orc.assert_close(dgam, dgo, 1e-4, 1e-3, name="dgamma")
    orc.assert_close(dbet, dbo, 1e-4, 1e-3, name="dbeta")


# ---------------------------------------------------------------------------
# fused BN + act + 2x2 pool
# ---------------------------------------------------------------------------
POOL_SHAPES = ([(2, 3, 25, 27, c) for c in (8, 24, 48, 64, 72)]
               + [(2, 1, 3, 3, 48), (2, 5, 3, 3, 64),
                  (2, 5, 21, 21, 48), (2, 5, 7, 7, 64),
                  (2, 3, 10, 12, 48)])          # one even shape


@pytest.mark.parametrize("per_task", [False, True], ids=["shared", "pertask"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=_id)
def test_bn_act_pool_matches_oracle(shape, dtype, per_task, monkeypatch):
    """Fused forward, fused plain backward (bn_act_pool_bwd), the composed
    create_graph backward and the MAML355_NO_BWDFUSE composition."""
    monkeypatch.delenv("MAML355_NO_BWDFUSE", raising=False)
    T, NS, H, W, C = shape
    Ho, Wo = H // 2, W // 2
    bf = dtype == torch.bfloat16
    # in the 3x3 shapes a single window is more than 1e-3 of the cases: the
    # seed base is one at which the oracle alone (no kernel involved)
    # excludes nothing there
    x, gamma, beta = _mk(shape, dtype, per_task, seed=620 + sum(shape))
    gy = torch.randn(T, NS, Ho, Wo, C,
                     generator=torch.Generator().manual_seed(601)).to(dtype)

    xo = orc.widen(x).requires_grad_(True)
    go, bo = _per_task(gamma, T), _per_task(beta, T)
    yo, mo, vo, pre, arg = orc.bn_act_pool(xo, go, bo, EPS, SLOPE)
    dxo, dgo, dbo = torch.autograd.grad(yo, (xo, go, bo), orc.widen(gy),
                                        create_graph=True)
    nz = orc.near_zero(pre)
    nt = orc.near_tied_windows(pre)
    assert orc.share(nz) <= orc.MAX_EXCLUDED and orc.share(nt) <= orc.MAX_EXCLUDED
    keep = ~(nz | orc.expand_windows(nt, H, W))
    dgo_f, dbo_f = _fold(dgo, per_task), _fold(dbo, per_task)

    def cmp_val(got, want, a_bf, rtol, atol, name, keep=None):
        if bf:
            assert got.dtype == torch.bfloat16
            orc.assert_bf16_close(got, want, a_bf, keep=keep, name=name)
        else:
            orc.assert_close(got, want, rtol, atol, keep=keep, name=name)

    def cmp_sum(got, want, name):
        if bf:
            orc.assert_f32_close(got, want, name)
        else:
            orc.assert_close(got, want, 1e-4, 1e-3, name=name)

    def check_grads(grads, tag):
        dx, dgam, dbet = grads
        cmp_val(dx, dxo, A_BWD, 1e-4, 1e-4, tag + " dx", keep=keep)
        cmp_sum(dgam, dgo_f, tag + " dgamma")
        cmp_sum(dbet, dbo_f, tag + " dbeta")
        # the trailing row / column take no pooled grad but still receive
        # the mean/variance terms: non-zero, and equal to the oracle's
        for odd, sl in ((H % 2, (slice(None), slice(None), H - 1)),
                        (W % 2, (slice(None), slice(None), slice(None), W - 1))):
            if odd:
                assert dxo[sl].abs().min().item() > 0
                cmp_val(dx[sl], dxo[sl], A_BWD, 1e-4, 1e-4, tag + " dx tail",
                        keep=keep[sl])

    xg, gg, bg = (t.clone().to(dev()).requires_grad_(True) for t in (x, gamma, beta))
    y, mean, var = ops.task_bn_act_pool(xg, gg, bg, EPS, SLOPE)
    assert y.shape == (T, NS, Ho, Wo, C)
    cmp_val(y, yo, A_FWD, 1e-4, 1e-4, "y")
    if bf:
        orc.assert_f32_close(mean, mo, "mean")
        orc.assert_f32_close(var, vo, "var")
    else:
        orc.assert_close(mean, mo, 1e-5, 1e-6, name="mean")
        orc.assert_close(var, vo, 1e-5, 1e-5, name="var")

    gyd = gy.to(dev())
    plain = torch.autograd.grad(y, (xg, gg, bg), gyd, retain_graph=True)
    check_grads(plain, "fused")
    graph = torch.autograd.grad(y, (xg, gg, bg), gyd, create_graph=True)
    check_grads(graph, "create_graph")

    monkeypatch.setenv("MAML355_NO_BWDFUSE", "1")
    comp = torch.autograd.grad(y, (xg, gg, bg), gyd, retain_graph=True)
    monkeypatch.delenv("MAML355_NO_BWDFUSE")
    # same math, same data: fp32 accumulation order is all that may differ
    if bf:
        orc.assert_bf16_close(plain[0], comp[0].double().cpu(), 1e-5,
                              name="fused vs composed dx")
    else:
        orc.assert_close(plain[0], comp[0].cpu(), 1e-5, 1e-5,
                         name="fused vs composed dx")
    orc.assert_close(plain[1], comp[1].cpu(), 1e-5, 1e-4, name="fused vs composed dgamma")
    orc.assert_close(plain[2], comp[2].cpu(), 1e-5, 1e-4, name="fused vs composed dbeta")

    if not bf:
        # second order through the fused op (composed Functions): fp32 only —
        # in bf16 the intermediates are rounded and the exact-input argument
        # does not hold
        (gx,) = torch.autograd.grad((y ** 2).sum() / 2, xg, create_graph=True)
        (ggx,) = torch.autograd.grad((gx ** 2).sum() / 2, xg)
        (gxo,) = torch.autograd.grad((yo ** 2).sum() / 2, xo, create_graph=True)
        (ggxo,) = torch.autograd.grad((gxo ** 2).sum() / 2, xo)
        orc.assert_close(ggx, ggxo, 1e-3, 1e-4, keep=keep, name="second order dx")


def test_bn_act_pool_fwd_second_grid_stride_trip():
    """4*513*513 = 1 052 676 pooled (position x C/8) threads: more than the
    4096 x 256 grid cap, so bn_norm_act_pool_vec_kernel strides once more.
    The pooled reference is built in fp32 from the kernel's own mean/var:
    only the normalise/pool pass is under test here."""
    T, NS, H, W, C = 1, 4, 1026, 1026, 8
    assert T * NS * (H // 2) * (W // 2) * (C // 8) > 4096 * 256
    torch.manual_seed(700)
    x = torch.randn(T, NS, H, W, C, device=dev()).to(torch.bfloat16)
    gamma = (torch.rand(C) + 0.5).to(dev())
    beta = torch.randn(C).to(dev())
    y, mean, var = ops.task_bn_act_pool(x, gamma, beta, EPS, SLOPE)
    m, v = mean.cpu().view(1, 1, 1, 1, C), var.cpu().view(1, 1, 1, 1, C)
    xf = x.cpu().float()
    pre = (xf - m) * torch.rsqrt(v + EPS) * gamma.cpu() + beta.cpu()
    a = torch.nn.functional.leaky_relu(pre, SLOPE)
    want = orc.windows(a).max(dim=-1).values
    got = y.cpu().float()
    assert got.shape == want.shape
    err = (got - want).abs()
    bound = orc.BF16_ULP * want.abs() + A_FWD
    worst = (err / bound).max().item()
    print(f"y: max|err|={err.max().item():.3e} worst err/bound={worst:.3f}")
    assert worst <= 1.0
    # the statistics themselves, loosely (they have their own tests)
    torch.testing.assert_close(mean.cpu(), xf.mean(dim=(1, 2, 3)), rtol=1e-3, atol=1e-3)
