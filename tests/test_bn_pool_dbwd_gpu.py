"""Second-order backward of the BN+act+pool block on native kernels only
(``maxpool2x2_gather``, ``bn_act_dbwd_full``) and the look-ahead ordered
reduces.

The default create_graph path must give the *bits* of the path with the
ATen gather glue, the tensor formula for d_gamma and the scalar sums kernel
(``MAML355_BNPOOL_DBWD=0``) at every order, and stays within the float64
oracle's bounds that
tests/test_bn_shapes_gpu.py applies to the composed path: fp32 through
autograd (rtol 1e-3 / atol 1e-4 on activations' second-order grads, the
BN test's 1e-3 shared / 2e-3 per-task on d_gamma), bf16 with the kernels
called directly on exact inputs (one bf16 ulp + 1e-3, fp32 sums to rtol
1e-4 / atol 1e-2).  Elements whose leaky-ReLU side or pool argmax is
within 1e-4 of undecided are left out of the routing-dependent comparisons
only, and may be at most 1e-3 of the cases."""

import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _oracle as orc
from howtotrainyourmamlpytorch_amd import ops
from howtotrainyourmamlpytorch_amd.config import get_args
from howtotrainyourmamlpytorch_amd.meta.engine import MAMLFewShotClassifier

EPS, SLOPE = 1e-5, 0.01
A_DBWD = 1e-3
ENV = "MAML355_BNPOOL_DBWD"

# (T, NB, H, W, C)
SHAPES = [
    (2, 3, 7, 9, 8),      # both extents odd, one channel group
    (2, 5, 21, 21, 48),   # M = 2205: ragged 256- and 1024-row slices,
                          # 6 channel groups do not divide 256 threads
    (1, 2, 6, 4, 64),
]


def dev():
    return torch.device("cuda", 0)


def _id(s):
    return "x".join(map(str, s))


def _inputs(shape, dtype, per_task, seed):
    T, NB, H, W, C = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g).to(dtype)
    gamma = torch.rand(*((T, C) if per_task else (C,)), generator=g) + 0.5
    beta = torch.randn(*((T, C) if per_task else (C,)), generator=g)
    gy = torch.randn(T, NB, H // 2, W // 2, C, generator=g).to(dtype)
    rx = torch.randn(*shape, generator=g).to(dtype)     # functional of dx
    # of dgamma / dbeta, in the shape of gamma: a shared gamma's grad is
    # the sum over tasks, so every task sees the same weights
    rg = torch.randn(*((T, C) if per_task else (C,)), generator=g)
    rb = torch.randn(*((T, C) if per_task else (C,)), generator=g)
    return x, gamma, beta, gy, rx, rg, rb


def _fold(p_t, per_task):
    return p_t if per_task else p_t.sum(0)


def _per_task(p, T):
    """[C] or [T, C] -> [T, C] (a shared row repeated)."""
    return p if p.dim() == 2 else p.unsqueeze(0).expand(T, -1).contiguous()


def _all_orders(inp, per_task, with_pg):
    """y, the create_graph first-order grads, and the grads of a random
    linear functional of them w.r.t. x, the incoming dy and gamma."""
    x, gamma, beta, gy, rx, rg, rb = (t.to(dev()) for t in inp)
    xg, gg, bg, gyg = (t.clone().requires_grad_(True)
                       for t in (x, gamma, beta, gy))
    y, _, _ = ops.task_bn_act_pool(xg, gg, bg, EPS, SLOPE)
    dx, dgam, dbet = torch.autograd.grad(y, (xg, gg, bg), gyg,
                                         create_graph=True)
    L = (dx.float() * rx.float()).sum()
    if with_pg:
        L = L + (dgam * rg).sum() + (dbet * rb).sum()
    d_x, d_dy, d_gamma = torch.autograd.grad(L, (xg, gyg, gg))
    return [t.detach() for t in (y, dx, dgam, dbet, d_x, d_dy, d_gamma)]


NAMES = ("y", "dx", "dgamma", "dbeta", "d_x", "d_dy", "d_gamma")


def _assert_bits(a, b, what):
    for n, p, q in zip(NAMES, a, b):
        assert p.dtype == q.dtype and p.shape == q.shape, (what, n)
        assert torch.equal(p, q), \
            f"{what}: {n} differs, max|delta|=" \
            f"{(p.double() - q.double()).abs().max().item():.3e}"


def _oracle_all_orders(inp, per_task, with_pg):
    """float64, exact inputs.  Returns the oracle's second-order grads and
    the keep masks (full resolution and pooled)."""
    x, gamma, beta, gy, rx, rg, rb = inp
    T, NB, H, W, C = x.shape
    xo = orc.widen(x).requires_grad_(True)
    uo = orc.widen(gy).requires_grad_(True)
    go = orc.widen(gamma)
    bo = orc.widen(beta)
    if go.dim() == 1:
        go, bo = go.expand(T, -1), bo.expand(T, -1)
    go = go.clone().requires_grad_(True)
    bo = bo.clone().requires_grad_(True)
    yo, _, _, pre, arg = orc.bn_act_pool(xo, go, bo, EPS, SLOPE)
    dxo, dgo, dbo = torch.autograd.grad(yo, (xo, go, bo), uo,
                                        create_graph=True)
    L = (dxo * orc.widen(rx)).sum()
    if with_pg:
        L = L + ((dgo * _per_task(orc.widen(rg), T)).sum()
                 + (dbo * _per_task(orc.widen(rb), T)).sum())
    d_xo, d_uo, d_go = torch.autograd.grad(L, (xo, uo, go))
    nz = orc.near_zero(pre)
    nt = orc.near_tied_windows(pre)
    assert orc.share(nz) <= orc.MAX_EXCLUDED and orc.share(nt) <= orc.MAX_EXCLUDED
    keep = ~(nz | orc.expand_windows(nt, H, W))
    # a pooled grad depends on the leaky-ReLU side at the window's argmax
    nz_arg = torch.gather(orc.windows(nz.to(torch.uint8)), -1,
                          arg.long().unsqueeze(-1)).squeeze(-1).bool()
    assert orc.share(nz_arg) <= orc.MAX_EXCLUDED
    keep_p = ~(nt | nz_arg)
    return d_xo, d_uo, _fold(d_go, per_task), keep, keep_p


@pytest.mark.parametrize("with_pg", [True, False], ids=["paramgrads", "dxonly"])
@pytest.mark.parametrize("per_task", [False, True], ids=["shared", "pertask"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_fused_dbwd_bits_and_oracle(shape, dtype, per_task, with_pg, monkeypatch):
    T, NB, H, W, C = shape
    inp = _inputs(shape, dtype, per_task, seed=900 + sum(shape))
    monkeypatch.delenv("MAML355_NO_BWDFUSE", raising=False)
    monkeypatch.setenv(ENV, "0")
    composed = _all_orders(inp, per_task, with_pg)
    monkeypatch.delenv(ENV)
    fused = _all_orders(inp, per_task, with_pg)
    _assert_bits(fused, composed, "native vs glue")
    assert fused[4].abs().max().item() > 0 and fused[5].abs().max().item() > 0
    # the trailing row / column take no pooled grad but their d_x is not 0
    if H % 2:
        assert fused[4][:, :, H - 1].abs().min().item() > 0
    if W % 2:
        assert fused[4][:, :, :, W - 1].abs().min().item() > 0

    d_xo, d_uo, d_go, keep, keep_p = _oracle_all_orders(inp, per_task, with_pg)
    if dtype == torch.float32:
        tol = 2e-3 if per_task else 1e-3
        orc.assert_close(fused[4], d_xo, 1e-3, 1e-4, keep=keep, name="d_x")
        orc.assert_close(fused[5], d_uo, 1e-3, 1e-4, keep=keep_p, name="d_dy")
        orc.assert_close(fused[6], d_go, tol, tol, name="d_gamma")
        return
    # bf16: the kernels called directly on exactly the oracle's inputs
    ext = ops.hip_ext()
    x, gamma, beta, gy, rx, rg, rb = (t.to(dev()) for t in inp)
    M, Ho, Wo = NB * H * W, H // 2, W // 2
    _, mask, mean, _, rstd = ext.bn_act_pool_fwd(x, gamma, beta, EPS, SLOPE, None)
    mask4 = mask.view(T * NB, Ho, Wo, C)
    u = ext.maxpool2x2_bwd(gy.view(T * NB, Ho, Wo, C), mask4, H, W)
    d_u, d_x, d_gamma_t, sums = ext.bn_act_dbwd_full(
        x.view(T, M, C), u.view(T, M, C), rx.view(T, M, C), mean, rstd,
        gamma, beta, _per_task(rg, T) if with_pg else None,
        _per_task(rb, T) if with_pg else None, SLOPE, True)
    d_dyp = ext.maxpool2x2_gather(d_u.view(T * NB, H, W, C), mask4)
    assert d_x.dtype == torch.bfloat16 and d_dyp.dtype == torch.bfloat16
    assert sums.shape == (T, 5, C)
    orc.assert_bf16_close(d_x.view(shape), d_xo, A_DBWD, keep=keep, name="d_x")
    orc.assert_bf16_close(d_dyp.view(gy.shape), d_uo, A_DBWD, keep=keep_p,
                          name="d_dyp")
    orc.assert_f32_close(_fold(d_gamma_t, per_task), d_go, "d_gamma")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
def test_fused_dbwd_tied_windows(dtype, monkeypatch):
    """Inputs from {-2, ..., 2}: BN+leaky-ReLU is strictly increasing per
    channel (gamma > 0), so equal inputs stay exactly equal and over a third
    of the windows tie at their maximum; the tie decides where d_dy is
    read.  First maximum wins, as in the oracle."""
    shape = (2, 4, 7, 9, 48)
    T, NB, H, W, C = shape
    inp = list(_inputs(shape, dtype, True, seed=950))
    g = torch.Generator().manual_seed(951)
    inp[0] = torch.randint(-2, 3, shape, generator=g).to(dtype)
    win = orc.windows(orc.widen(inp[0]))
    top = win.topk(2, dim=-1).values
    assert orc.share(top[..., 0] == top[..., 1]) > 0.3
    ext = ops.hip_ext()
    mask = ext.bn_act_pool_fwd(inp[0].to(dev()), inp[1].to(dev()),
                               inp[2].to(dev()), EPS, SLOPE, None)[1]
    arg = orc.first_argmax(win)
    assert torch.equal(mask.cpu().long(), arg.long())
    assert set(arg.flatten().tolist()) == {0, 1, 2, 3}
    monkeypatch.delenv("MAML355_NO_BWDFUSE", raising=False)
    monkeypatch.setenv(ENV, "0")
    composed = _all_orders(inp, True, True)
    monkeypatch.delenv(ENV)
    fused = _all_orders(inp, True, True)
    _assert_bits(fused, composed, "ties: native vs glue")
    # d_dy is a moved value: where it came from follows the first maximum
    assert fused[5].abs().max().item() > 0


# (T, M, C): R = 4 row groups per slice (C <= 64), 2 (C = 72), 1 (C = 136);
# ragged last slice; 79 slices (more than one look-ahead batch of the reduce)
FULL_SHAPES = [(2, 2025, 8), (2, 2025, 24), (2, 2025, 48), (2, 2025, 64),
               (2, 2025, 72), (2, 300, 136), (1, 20000, 8), (2, 9, 48)]


@pytest.mark.parametrize("act", [True, False], ids=["act", "noact"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", FULL_SHAPES, ids=_id)
def test_dbwd_full_bits_equal_scalar_kernels(shape, dtype, act):
    """bn_act_dbwd_full (8-channel sums, d_gamma_t in the reduce, absent
    grads as zero) against bn_act_dbwd and the tensor formula."""
    T, M, C = shape
    ext = ops.hip_ext()
    g = torch.Generator().manual_seed(970 + sum(shape))
    x, u, gx = (torch.randn(T, M, C, generator=g).to(dtype).to(dev())
                for _ in range(3))
    gamma = (torch.rand(T, C, generator=g) + 0.5).to(dev())
    beta = torch.randn(T, C, generator=g).to(dev())
    ggam = torch.randn(T, C, generator=g).to(dev())
    gbet = torch.randn(T, C, generator=g).to(dev())
    _, mean, _, rstd = ext.bn_act_fwd(x, gamma, beta, EPS, SLOPE, act)
    zero = torch.zeros(T, C, device=dev())
    for gg, gb in ((ggam, gbet), (None, None), (ggam, None)):
        d_u0, d_x0, sums0 = ext.bn_act_dbwd(
            x, u, gx, mean, rstd, gamma, beta, zero if gg is None else gg,
            zero if gb is None else gb, SLOPE, act)
        s = sums0 / M
        d_gamma0 = rstd * M * (s[:, 4] - s[:, 0] * s[:, 2] - s[:, 1] * s[:, 3])
        d_u1, d_x1, d_gamma1, sums1 = ext.bn_act_dbwd_full(
            x, u, gx, mean, rstd, gamma, beta, gg, gb, SLOPE, act)
        assert torch.equal(sums1, sums0), "sums"
        assert torch.equal(d_u1, d_u0), "d_u"
        assert torch.equal(d_x1, d_x0), "d_x"
        assert torch.equal(d_gamma1, d_gamma0), "d_gamma_t"


# ---------------------------------------------------------------------------
# model level: 14x15 images, 8 filters, 3 stages, 2 inner steps, second
# order, max_pooling=True (15 -> 7 -> 3: odd at two stages)
# ---------------------------------------------------------------------------
IH, IW = 14, 15


def _meta_grad():
    args = get_args([
        "--batch_size", "2", "--num_classes_per_set", "3",
        "--num_samples_per_class", "2", "--num_target_samples", "2",
        "--image_height", str(IH), "--image_width", str(IW),
        "--image_channels", "1",
        "--cnn_num_filters", "8", "--num_stages", "3",
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
    xs = torch.randn(2, 3, 2, 1, IH, IW, generator=g)
    xt = torch.randn(2, 3, 2, 1, IH, IW, generator=g)
    ys = torch.arange(3).view(1, 3, 1).expand(2, 3, 2).contiguous()
    losses, _ = model.train_forward_prop((xs, xt, ys, ys.clone()), epoch=1)
    grad = torch.autograd.grad(losses["loss"], model.classifier.theta)[0]
    return losses["loss"].detach().clone(), grad.detach().clone()


def test_model_meta_gradient_bits(monkeypatch):
    """Deterministic mode (ordered reductions everywhere), as the bitwise
    comparisons of whole runs use it."""
    calls = []
    ext = ops.hip_ext()
    for name in ("maxpool2x2_gather", "bn_act_dbwd_full"):
        def counted(*a, _real=getattr(ext, name), _name=name):
            calls.append(_name)
            return _real(*a)
        monkeypatch.setattr(ext, name, counted)
    monkeypatch.setenv("MAML355_DETERMINISTIC", "1")
    monkeypatch.delenv("MAML355_NO_BWDFUSE", raising=False)
    monkeypatch.setenv(ENV, "0")
    loss0, g0 = _meta_grad()
    assert not calls
    loss0b, g0b = _meta_grad()
    assert torch.equal(g0, g0b), "the composed path itself is not reproducible"
    monkeypatch.delenv(ENV)
    loss1, g1 = _meta_grad()
    assert set(calls) == {"maxpool2x2_gather", "bn_act_dbwd_full"}, \
        "the native second-order backward did not run"
    assert torch.isfinite(g1).all().item() and g1.abs().max().item() > 0
    assert torch.equal(loss0, loss1)
    assert torch.equal(g0, g1), \
        f"max|delta|={(g0.double() - g1.double()).abs().max().item():.3e}"


# ---------------------------------------------------------------------------
# the look-ahead ordered reduces: bn_act_fwd / bn_act_bwd against the values
# the one-load-one-add reduce gave for the same inputs (recorded fixture;
# the partials are not exposed).  (1, 20000, 8): 20 slices, more than one
# look-ahead batch.
# ---------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "bn_reduce_order.json")


def reduce_inputs(T, M, C, dtype):
    """Inputs by integer arithmetic only: identical on every machine."""
    n = T * M * C
    i = np.arange(n, dtype=np.uint64)
    hx = (i * np.uint64(2654435761) + np.uint64(12345)) % np.uint64(1 << 32)
    hd = (i * np.uint64(40503) + np.uint64(977)) % np.uint64(1 << 16)
    x = (hx.astype(np.float64) / 2.0 ** 32 - 0.5) * 4.0 + 0.25
    dy = (hd.astype(np.float64) / 2.0 ** 16 - 0.5) * 2.0
    c = np.arange(C, dtype=np.float64)
    gamma = 0.5 + (c * 7 % 11) / 11.0
    beta = ((c * 5 % 13) - 6.0) / 8.0
    tt = lambda a: torch.from_numpy(a.astype(np.float32))
    return (tt(x).view(T, M, C).to(dtype), tt(dy).view(T, M, C).to(dtype),
            tt(gamma), tt(beta))


def reduce_outputs(T, M, C, dtype):
    ext = ops.hip_ext()
    x, dy, gamma, beta = (t.to(dev()) for t in reduce_inputs(T, M, C, dtype))
    _, mean, var, rstd = ext.bn_act_fwd(x, gamma, beta, EPS, SLOPE, True)
    _, dgamma_t, dbeta_t = ext.bn_act_bwd(dy, x, mean, rstd, gamma, beta,
                                          SLOPE, True)
    return {"mean": mean, "var": var, "dgamma_t": dgamma_t, "dbeta_t": dbeta_t}


REDUCE_SHAPES = [(2, 2205, 48), (1, 20000, 8)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", REDUCE_SHAPES, ids=_id)
def test_reduce_order_unchanged(shape, dtype):
    with open(GOLDEN) as f:
        golden = json.load(f)
    key = _id(shape) + ("_fp32" if dtype == torch.float32 else "_bf16")
    got = reduce_outputs(*shape, dtype)
    for name, t in got.items():
        # fp32 bit patterns, as signed 32-bit integers
        want = torch.tensor(golden[key][name], dtype=torch.int32).view(t.shape)
        assert torch.equal(t.cpu().view(torch.int32), want), (key, name)
