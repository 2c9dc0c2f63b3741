"""Layer-norm family (layernorm.hip) at the shapes and modes the workloads
reach.

bf16 runs call the kernels directly on exactly widened inputs and are
compared with the float64 oracle (tests/_oracle_ln.py): bf16 results to
one bf16 ulp plus 1e-5 (fwd), 1e-4 (bwd), 1e-3 (dbwd); fp32 results (mean,
rstd, dbias_t) to rtol 1e-4 / atol 1e-2.  fp32 runs go through autograd and
are compared with ``ops.reference`` at 1e-5 (fwd), 1e-4 (bwd) and 1e-3
(second order); the second-order loss depends on dx and dbias together, so
the ``gb`` cotangent of the double-backward kernel is non-zero.  Elements
whose pre-activation is within 1e-4 of zero are left out of the dx, d_dy
and d_x comparisons only and may be at most 1e-3 of the cases (expected
for N(0,1) inputs and bias: about 6e-5).

Which test covers what (D = H*W*C; a block is 256 threads x 8 elements):

* ``(2,1,3,3,8)``      D = 72: less than one pass of a block, one image
                       per task.
* ``(3,7,3,3,8)``      many small images; dbias_t sums over 7 of them.
* ``(2,3,9,7,5)``,     D = 315 and 4095, not multiples of 8: image bases
  ``(2,3,9,7,65)``     fall on every residue, so each image has a scalar
                       head and tail around the 8-wide body (bf16), and
                       dbias runs its one-element variant.
* ``(2,5,7,7,64)``,    the workloads' odd stages.
  ``(2,5,21,21,48)``
* ``(1,2,40,41,48)``   D = 78720 >= 32768: split over 4 workgroups of
                       19680 elements, ten trips of the per-chunk loop.
* ``(1,2,26,26,49)``   D = 33124: the split threshold is D >= 32768 (two
                       chunks of at least 16384); this is the smallest
                       H*W*C of that H and W above it that is NOT a
                       multiple of 8 (so the second image's chunks start
                       misaligned), with two ragged chunks 16568 + 16556.
                       Below the threshold every other shape here runs the
                       single-workgroup kernel.
* ``(1,2100,3,3,8)``   2100 images > the 2048-block grid cap: the second
                       trip of the work-item loop (reuse of the LDS
                       reduction buffer).
* ``test_ln_no_act_*`` apply_act=False: the ACT=false templates.
* ``test_ln_offset_mean_*``  mean 3, std 0.5 at the tolerances above;
  ``test_ln_far_offset_mean_fp32_rstd``  mean 100: a bare
                       E[x^2] - mean^2 misses rstd by 1e-3 there, the
                       shifted sums must hold 1e-5.
* shared / per-task bias: the PER_TASK templates and the dbias fold."""

import pytest
import torch

pytestmark = pytest.mark.gpu

import _oracle_ln as orl
from howtotrainyourmamlpytorch_amd import ops
from howtotrainyourmamlpytorch_amd.ops import reference as ref

EPS, SLOPE = 1e-5, 0.01
A_FWD, A_BWD, A_DBWD = 1e-5, 1e-4, 1e-3


def dev():
    return torch.device("cuda", 0)


def _id(s):
    return "x".join(map(str, s))


# (T, NS, H, W, C): each the smallest reaching its mode (module docstring)
BOTH_BIAS_SHAPES = [
    (2, 1, 3, 3, 8),
    (3, 7, 3, 3, 8),
    (2, 3, 9, 7, 5),
    (2, 3, 9, 7, 65),
    (2, 5, 7, 7, 64),
    (2, 5, 21, 21, 48),
]
SPLIT_SHAPES = [(1, 2, 40, 41, 48), (1, 2, 26, 26, 49)]
MANY_IMAGES = (1, 2100, 3, 3, 8)
CASES = ([(s, pt) for s in BOTH_BIAS_SHAPES for pt in (False, True)]
         + [(s, True) for s in SPLIT_SHAPES]
         + [(SPLIT_SHAPES[0], False), (MANY_IMAGES, False)])
CASE_IDS = [_id(s) + ("-pertask" if pt else "-shared") for s, pt in CASES]
NO_ACT_SHAPES = [(2, 3, 9, 7, 5), (2, 5, 7, 7, 64)]
OFFSET_SHAPE = (2, 5, 21, 21, 48)


def _mk(shape, dtype, per_task, seed, offset=0.0, std=1.0):
    T, NS, H, W, C = shape
    g = torch.Generator().manual_seed(seed)
    x = (offset + std * torch.randn(*shape, generator=g)).to(dtype)
    bias = torch.randn(*((T, H, W, C) if per_task else (H, W, C)), generator=g)
    return x, bias


def _keep(pre, apply_act=True):
    """Elements kept in a dx comparison, with the share assertion."""
    if not apply_act:
        return None
    nz = orl.near_zero(pre)
    assert orl.share(nz) <= orl.MAX_EXCLUDED, orl.share(nz)
    return ~nz


# ---------------------------------------------------------------------------
# fp32 through autograd vs ops.reference
# ---------------------------------------------------------------------------
def _second_order_loss(op, x, b, act, NS):
    """Depends on dx and dbias together: gx and gb non-zero.  Scaled so
    that both upstream grads are O(1)."""
    y = op(x, None, b, EPS, SLOPE, act)
    l1 = (y.float() ** 2).sum() / 2
    gx, gb = torch.autograd.grad(l1, (x, b), create_graph=True)
    return (gx.float() ** 2).sum() / 2 + (gb ** 2).sum() / (2 * NS ** 0.5)


def _run_fp32_autograd(shape, per_task, act, seed, offset=0.0, std=1.0):
    T, NS, H, W, C = shape
    x, bias = _mk(shape, torch.float32, per_task, seed, offset, std)
    u = torch.randn(*shape, generator=torch.Generator().manual_seed(seed + 1))
    pre = orl.ln_act(orl.widen(x), orl.widen(bias), EPS, SLOPE, act)[3]
    keep = _keep(pre, act)

    def leaves(d):
        return [t.clone().to(d).requires_grad_(True) for t in (x, bias)]

    xg, bg = leaves(dev())
    xr, br = leaves("cpu")
    y = ops.task_layer_norm_act(xg, None, bg, EPS, SLOPE, act)
    yr = ref.task_layer_norm_act(xr, None, br, EPS, SLOPE, act)
    assert y.dtype == torch.float32 and y.shape == shape
    orl.assert_close(y, yr, 1e-5, 1e-5, name="y")

    d = torch.autograd.grad(y, (xg, bg), u.to(dev()))
    dr = torch.autograd.grad(yr, (xr, br), u)
    orl.assert_close(d[0], dr[0], 1e-4, 1e-4, keep=keep, name="dx")
    orl.assert_close(d[1], dr[1], 1e-4, 1e-4, name="dbias")

    xg, bg = leaves(dev())
    xr, br = leaves("cpu")
    dd = torch.autograd.grad(
        _second_order_loss(ops.task_layer_norm_act, xg, bg, act, NS), (xg, bg))
    ddr = torch.autograd.grad(
        _second_order_loss(ref.task_layer_norm_act, xr, br, act, NS), (xr, br))
    orl.assert_close(dd[0], ddr[0], 1e-3, 1e-3, keep=keep, name="dd/dx")
    orl.assert_close(dd[1], ddr[1], 1e-3, 1e-3, name="dd/dbias")
    assert ddr[1].abs().max().item() > 0


@pytest.mark.parametrize("shape,per_task", CASES, ids=CASE_IDS)
def test_ln_act_fp32_autograd_all_orders(shape, per_task):
    _run_fp32_autograd(shape, per_task, True, seed=100 + sum(shape))


@pytest.mark.parametrize("per_task", [False, True], ids=["shared", "pertask"])
@pytest.mark.parametrize("shape", NO_ACT_SHAPES, ids=_id)
def test_ln_no_act_fp32_autograd_all_orders(shape, per_task):
    _run_fp32_autograd(shape, per_task, False, seed=200 + sum(shape))


# ---------------------------------------------------------------------------
# bf16, kernels called directly, vs the exact-input oracle
# ---------------------------------------------------------------------------
def _run_bf16_kernels(shape, per_task, act, seed, offset=0.0, std=1.0):
    T, NS, H, W, C = shape
    D = H * W * C
    ext = ops.hip_ext()
    x, bias = _mk(shape, torch.bfloat16, per_task, seed, offset, std)
    g = torch.Generator().manual_seed(seed + 1)
    u = torch.randn(*shape, generator=g).to(torch.bfloat16)
    gx = torch.randn(*shape, generator=g).to(torch.bfloat16)
    gb = torch.randn(T, H, W, C, generator=g)

    xd, ud, gxd = (t.to(dev()) for t in (x, u, gx))
    bd = bias.to(dev()).reshape(*((T, D) if per_task else (D,)))
    gbd = gb.to(dev()).reshape(T, D)
    y, mean, rstd = ext.ln_act_fwd(xd, bd, EPS, SLOPE, act)
    dx, dbias_t = ext.ln_act_bwd(ud, xd, mean, rstd, bd, SLOPE, act)
    d_dy, d_x = ext.ln_act_dbwd(xd, ud, gxd, gbd, mean, rstd, bd, SLOPE, act)

    xo = orl.widen(x).requires_grad_(True)
    uo = orl.widen(u).requires_grad_(True)
    bo = orl.per_task_bias(bias, T)
    yo, mo, ro, pre = orl.ln_act(xo, bo, EPS, SLOPE, act)
    keep = _keep(pre, act)
    dxo, dbo = torch.autograd.grad(yo, (xo, bo), uo, create_graph=True)
    L = (dxo * orl.widen(gx)).sum() + (dbo * orl.widen(gb)).sum()
    d_uo, d_xo = torch.autograd.grad(L, (uo, xo))

    for t in (y, dx, d_dy, d_x):
        assert t.dtype == torch.bfloat16 and t.shape == shape
    assert mean.shape == rstd.shape == (T, NS)
    assert dbias_t.shape == (T, D)
    orl.assert_bf16_close(y, yo, A_FWD, name="y")
    orl.assert_f32_close(mean, mo, "mean")
    orl.assert_f32_close(rstd, ro, "rstd")
    orl.assert_bf16_close(dx, dxo, A_BWD, keep=keep, name="dx")
    orl.assert_f32_close(dbias_t, dbo.reshape(T, D), "dbias_t")
    orl.assert_bf16_close(d_dy, d_uo, A_DBWD, keep=keep, name="d_dy")
    orl.assert_bf16_close(d_x, d_xo, A_DBWD, keep=keep, name="d_x")
    return mean, rstd, mo, ro


@pytest.mark.parametrize("shape,per_task", CASES, ids=CASE_IDS)
def test_ln_kernels_bf16_match_oracle(shape, per_task):
    _run_bf16_kernels(shape, per_task, True, seed=300 + sum(shape))


@pytest.mark.parametrize("shape", NO_ACT_SHAPES, ids=_id)
def test_ln_no_act_kernels_bf16_match_oracle(shape):
    _run_bf16_kernels(shape, True, False, seed=400 + sum(shape))


def test_ln_kernels_bf16_are_bitwise_repeatable():
    """No atomics, fixed reduction order: two calls agree bit for bit, at a
    split and at an unsplit shape."""
    ext = ops.hip_ext()
    for shape in ((2, 5, 21, 21, 48), (1, 2, 26, 26, 49)):
        T, NS, H, W, C = shape
        D = H * W * C
        x, bias = _mk(shape, torch.bfloat16, True, 800)
        u = torch.randn(*shape, generator=torch.Generator().manual_seed(801))
        xd, ud = x.to(dev()), u.to(torch.bfloat16).to(dev())
        bd = bias.to(dev()).reshape(T, D)
        gbd = torch.ones(T, D, device=dev())

        def once():
            y, mean, rstd = ext.ln_act_fwd(xd, bd, EPS, SLOPE, True)
            dx, db = ext.ln_act_bwd(ud, xd, mean, rstd, bd, SLOPE, True)
            d_dy, d_x = ext.ln_act_dbwd(xd, ud, ud, gbd, mean, rstd, bd, SLOPE, True)
            return y, mean, rstd, dx, db, d_dy, d_x

        for a, b in zip(once(), once()):
            assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# offset mean: the variance must not be E[x^2] - mean^2 in fp32
# ---------------------------------------------------------------------------
def _rstd_rel_err(rstd, ro):
    rel = ((rstd.detach().cpu().double() - ro.detach()) / ro.detach()).abs().max().item()
    print(f"rstd: max rel err {rel:.3e}")
    return rel


def test_ln_offset_mean_bf16():
    mean, rstd, mo, ro = _run_bf16_kernels(OFFSET_SHAPE, True, True, seed=500,
                                           offset=3.0, std=0.5)
    _rstd_rel_err(rstd, ro)


def test_ln_offset_mean_fp32():
    _run_fp32_autograd(OFFSET_SHAPE, True, True, seed=501, offset=3.0, std=0.5)
    x, bias = _mk(OFFSET_SHAPE, torch.float32, True, 501, offset=3.0, std=0.5)
    T = OFFSET_SHAPE[0]
    y, mean, rstd = ops.hip_ext().ln_act_fwd(
        x.to(dev()), bias.to(dev()).reshape(T, -1), EPS, SLOPE, True)
    yo, mo, ro, _ = orl.ln_act(orl.widen(x), orl.widen(bias), EPS, SLOPE, True)
    _rstd_rel_err(rstd, ro)
    orl.assert_close(mean, mo, 1e-5, 1e-5, name="mean")
    orl.assert_close(rstd, ro, 1e-5, 1e-5, name="rstd")
    orl.assert_close(y, yo, 1e-5, 1e-5, name="y")


def test_ln_far_offset_mean_fp32_rstd():
    """mean 100, std 0.5 — further out than the workloads go, so that the
    two forms separate by orders of magnitude.  E[x^2] - mean^2 in fp32
    subtracts two numbers of size 1e4 to get 0.25: each carries at least
    one rounding (2^-24 * 1e4 = 6e-4), a relative variance error of 2e-3
    or more, 1e-3 on rstd.  The kernel's sums are shifted by the image's
    first element K: x - K is exact for neighbours in fp32 and
    E[(x-K)^2] <= var * (1 + z^2), z = (mean - K)/std, so nothing larger
    than a few var is subtracted and rstd keeps a few fp32 ulps (2^-23 =
    1.2e-7 each).  1e-5 lies two decades from either."""
    shape = (2, 3, 21, 21, 48)
    T = shape[0]
    x, bias = _mk(shape, torch.float32, True, 502, offset=100.0, std=0.5)
    k = x.reshape(T * shape[1], -1)
    z = ((k.mean(dim=1) - k[:, 0]) / k.std(dim=1)).abs().max().item()
    assert z < 5, z                      # the shift is a typical sample
    y, mean, rstd = ops.hip_ext().ln_act_fwd(
        x.to(dev()), bias.to(dev()).reshape(T, -1), EPS, SLOPE, True)
    _, mo, ro, _ = orl.ln_act(orl.widen(x), orl.widen(bias), EPS, SLOPE, True)
    assert _rstd_rel_err(rstd, ro) <= 1e-5
    orl.assert_close(mean, mo, 1e-6, 0.0, name="mean")


# ---------------------------------------------------------------------------
# dispatch
# ---------------------------------------------------------------------------
def test_ln_dispatch_kernels_only_for_the_backbone_form(monkeypatch):
    """weight None + elementwise bias goes to the kernels (the composition
    is not reached); a weight or a per-channel bias stays on it."""
    shape = (2, 3, 3, 3, 8)
    x, bias = _mk(shape, torch.bfloat16, False, 900)
    xd, bd = x.to(dev()), bias.to(dev())
    want = ref.task_layer_norm_act(xd, None, bd, EPS, SLOPE)
    calls = []
    real = ref.task_layer_norm_act

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(ref, "task_layer_norm_act", spy)
    y = ops.task_layer_norm_act(xd, None, bd, EPS, SLOPE)
    assert not calls
    torch.testing.assert_close(y.float(), want.float(), rtol=2 ** -7, atol=1e-5)
    ops.task_layer_norm_act(xd, torch.ones(8, device=dev()),
                            torch.zeros(8, device=dev()), EPS, SLOPE)
    ops.task_layer_norm_act(xd, None, torch.zeros(8, device=dev()), EPS, SLOPE)
    assert len(calls) == 2
