"""Cases, inputs and checks of the head, loss and update kernels, shared by
``test_head_loss_update_gpu.py`` (the HIP kernels) and ``test_oracle.py``
(``ops.reference`` in fp32 on the CPU, standing in for the kernels, so that
no bound is tighter than fp32 arithmetic allows).

Every check takes the implementation under test and the device it runs on,
draws its inputs from a seeded CPU generator, hands the float64 oracle
exactly the values the implementation consumes, compares every element and
returns the worst err/bound it printed.
"""

from __future__ import annotations

import numpy as np
import torch

import _oracle as orc

CPU = torch.device("cpu")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _id(case):
    """Leading sizes joined by x, the rest by -: 3x40x5-normal-fp32-uniform."""
    n = next((i for i, c in enumerate(case) if type(c) is not int), len(case))
    rest = ["bias" if c is True else "nobias" if c is False
            else f"{c:g}" if isinstance(c, float) else str(c) for c in case[n:]]
    return "-".join((["x".join(map(str, case[:n]))] if n else []) + rest)


# ---------------------------------------------------------------------------
# bf16 linear trio: (T, M, K, ways, bias)
# ---------------------------------------------------------------------------
LINEAR_SHAPES = [
    (2, 9, 64, 5, True),        # one lane pass
    (2, 1, 1, 1, True),         # M = K = ways = 1
    (3, 7, 63, 20, False),      # K below one wave; no bias
    (2, 5, 65, 64, True),       # K tail of one element; ways at the cap
    (5, 3, 200, 64, True),      # T*ways = 320: lin_db's second block
    (2, 7, 1200, 20, True),     # the mini-ImageNet head
    (3, 5500, 8, 3, True),      # 16500 rows: second wave-stride trip of lin_fwd
    (3, 5500, 64, 3, True),     # T*M*K = 1,056,000: second trip of lin_dx
    (2, 2, 8200, 64, False),    # T*ways*K = 1,049,600: second trip of lin_wgrad
]
LINEAR_SECOND_ORDER_SHAPES = [(2, 7, 72, 5), (2, 5, 200, 20)]


def linear_inputs(shape, integers=False):
    """x, dy bf16; w, b fp32 (b None without bias).  ``integers``: x, dy, b
    in {-3..3} and w in quarter units in {-0.75..0.75}; from K = 4096 on
    {-2..2} and {-0.5..0.5}, which keeps every partial sum an exact fp32
    multiple of 1/4 far below 2^24 quarter units (K = 8200: at most
    8200 * 2 * 0.5 = 8200).  A nonzero b carries 2^-10 more in fp32, which
    the kernel's rounding of the bias to bf16 has to remove: what it
    consumes, and what the oracle gets, is the integer."""
    T, M, K, ways, bias = shape
    g = _gen(1000 + T + M + K + ways)
    if integers:
        r = 2 if K >= 4096 else 3
        ri = lambda *s: torch.randint(-r, r + 1, s, generator=g).float()  # noqa: E731
        x, dy, w, b = ri(T, M, K), ri(T, M, ways), ri(T, ways, K) / 4, ri(T, ways)
        b = b + (b != 0) * 2.0 ** -10
        assert torch.equal(b.to(torch.bfloat16).float(), b.round())
    else:
        x = torch.randn(T, M, K, generator=g)
        dy = torch.randn(T, M, ways, generator=g)
        w = torch.randn(T, ways, K, generator=g)
        b = torch.randn(T, ways, generator=g)
    return (x.to(torch.bfloat16), w, b if bias else None, dy.to(torch.bfloat16))


def linear_first_order(fn, x, w, b, dy, device):
    xg = x.to(device).requires_grad_(True)
    wg = w.to(device).requires_grad_(True)
    leaves = [xg, wg]
    bg = None
    if b is not None:
        bg = b.to(device).requires_grad_(True)
        leaves.append(bg)
    y = fn(xg, wg, bg)
    grads = torch.autograd.grad(y, leaves, dy.to(device))
    return (y.detach(),) + tuple(grads)


def linear_oracle(x, w, b, dy):
    """Oracle outputs and the magnitudes sum|a||b| of the same sums."""
    def run(xo, wo, bo, dyo):
        xo, wo = xo.requires_grad_(True), wo.requires_grad_(True)
        leaves = [xo, wo] + ([bo.requires_grad_(True)] if bo is not None else [])
        yo = orc.linear(xo, wo, bo)
        return (yo.detach(),) + torch.autograd.grad(yo, leaves, dyo)
    args = (orc.widen(x), orc.round_bf16(w),
            orc.round_bf16(b) if b is not None else None, orc.widen(dy))
    ref = run(*args)
    mag = run(*(a.abs() if a is not None else None for a in args))
    return ref, mag


def check_linear_first_order(fn, shape, device):
    T, M, K, ways, bias = shape
    x, w, b, dy = linear_inputs(shape)
    got = linear_first_order(fn, x, w, b, dy, device)
    ref, mag = linear_oracle(x, w, b, dy)
    names = ("y", "dx", "dw") + (("db",) if bias else ())
    n = {"y": K + 1, "dx": ways, "dw": M, "db": M}
    return max(orc.assert_dot_bounded(g_, r_, m_, n[k], k, bf16=k in ("y", "dx"))
               for k, g_, r_, m_ in zip(names, got, ref, mag))


def check_linear_exact(fn, shape, device):
    x, w, b, dy = linear_inputs(shape, integers=True)
    got = linear_first_order(fn, x, w, b, dy, device)
    ref, _ = linear_oracle(x, w, b, dy)
    for k, g_, r_ in zip(("y", "dx", "dw", "db"), got, ref):
        want = r_.to(torch.bfloat16) if k in ("y", "dx") else r_.float()
        assert g_.dtype == want.dtype, (k, g_.dtype)
        assert torch.equal(g_.cpu(), want), \
            f"{k}: max|diff| {(orc.widen(g_) - want.double()).abs().max().item():.3e}"


def linear_second_order(fn, x, w, b, device):
    """The two scenarios of test_wconv_second_order: an inner step through
    the gw / gb grads, and create_graph through dx."""
    x_ = x.to(device)
    w_ = w.to(device).requires_grad_(True)
    b_ = b.to(device).requires_grad_(True)
    y = fn(x_, w_, b_)
    gw, gb = torch.autograd.grad((y.float() ** 2).mean(), (w_, b_), create_graph=True)
    y2 = fn(x_, w_ - 0.1 * gw, b_ - 0.1 * gb)
    out = torch.autograd.grad((y2.float() ** 2).mean(), (w_, b_))
    xi = x.to(device).requires_grad_(True)
    wi = w.to(device).requires_grad_(True)
    y = fn(xi, wi, None)
    (gx,) = torch.autograd.grad((y.float() ** 2).mean(), (xi,), create_graph=True)
    out += torch.autograd.grad((gx.float() ** 2).sum(), (xi, wi))
    return [t.detach().float().cpu() for t in out]


# ---------------------------------------------------------------------------
# softmax-CE: (T, M, ways, family, logits dtype, labels)
# ---------------------------------------------------------------------------
CE_SHAPES = [(3, 40, 5), (2, 1, 1), (2, 3, 2), (2, 7, 33), (2, 5, 64),
             (257, 3, 5),           # T > 256: ce_rowmean's second block
             (2, 8200, 5),          # 16400 rows: second trip of ce_fwd, ce_dbwd
             (2, 8200, 64)]         # 1,049,600 elements: second trip of ce_bwd
CE_FAMILIES = ["normal", "equal", "offset", "spread", "saturated"]
CE_CASES = (
    [s + ("normal", dt, "uniform") for s in CE_SHAPES for dt in ("fp32", "bf16")]
    + [s + (f, dt, "uniform") for s in ((3, 40, 5), (2, 5, 64))
       for f in CE_FAMILIES[1:] for dt in ("fp32", "bf16")]
    + [s + ("normal", dt, "last") for s in ((2, 7, 33), (2, 5, 64), (3, 40, 5))
       for dt in ("fp32", "bf16")]
    + [(3, 40, 5, "normal", dt, "int32") for dt in ("fp32", "bf16")]
    + [(2, 5, 64, "spread", "fp32", "int32")]
)


def ce_inputs(case):
    """Labels are always in [0, ways): the kernel does not check them."""
    T, M, ways, family, dt, lab = case
    g = _gen(2000 + T + M + ways + CE_FAMILIES.index(family))
    if lab == "last":
        labels = torch.full((T, M), ways - 1, dtype=torch.long)
    else:
        labels = torch.randint(0, ways, (T, M), generator=g)
    logits = torch.randn(T, M, ways, generator=g)
    if family == "equal":
        logits = torch.full((T, M, ways), 1.25)
    elif family == "offset":
        logits = logits + 1.0e4
    elif family == "spread":
        logits = logits * 30.0
    elif family == "saturated":
        top = logits.amax(dim=-1, keepdim=True) + 50.0
        logits = logits.scatter(-1, labels.unsqueeze(-1), top)
    if dt == "bf16":
        logits = logits.to(torch.bfloat16)
    if lab == "int32":
        labels = labels.to(torch.int32)
    assert 0 <= int(labels.min()) and int(labels.max()) < ways
    # the per-task upstream weight is O(M), as the meta-loss's would be for a
    # sum over rows: dlogits, its double backward and d/dgt are then O(1) at
    # every M, and the absolute part of their bounds stays small beside them
    gt = (torch.rand(T, generator=g) + 0.5) * M
    return logits, labels, gt


def check_ce(fn, case, device):
    """loss, dlogits under a per-task weight gt, and the double backward of
    ``sum dl^2`` with respect to the logits and to gt (ce_dbwd's two
    outputs).  The oracle's double backward takes the cotangent the
    implementation's own backward received, ``2 dl`` of its own dl, so the
    second comparison does not inherit the error of the first."""
    logits, labels, gt = ce_inputs(case)
    bf16 = logits.dtype == torch.bfloat16
    lg = logits.to(device).requires_grad_(True)
    gg = gt.to(device).requires_grad_(True)
    loss = fn(lg, labels.to(device))
    (dl,) = torch.autograd.grad((loss * gg).sum(), lg, create_graph=True)
    ddl, dgt = torch.autograd.grad((dl.float() ** 2).sum(), (lg, gg))
    assert loss.dtype == torch.float32 and dgt.dtype == torch.float32
    assert dl.dtype == logits.dtype and ddl.dtype == logits.dtype

    lo = orc.widen(logits).requires_grad_(True)
    go = orc.widen(gt).requires_grad_(True)
    loss_o = orc.softmax_ce(lo, labels)
    (dl_o,) = torch.autograd.grad((loss_o * go).sum(), lo, create_graph=True)
    ddl_o, dgt_o = torch.autograd.grad(dl_o, (lo, go), 2.0 * orc.widen(dl))
    return max(
        orc.assert_within(loss, loss_o, orc.ce_loss_bound(loss_o, lo), "loss"),
        orc.assert_within(dl, dl_o, orc.ce_prob_bound(dl_o, lo, bf16), "dlogits"),
        orc.assert_within(ddl, ddl_o, orc.ce_prob_bound(ddl_o, lo, bf16),
                          "d(sum dl^2)/dlogits"),
        orc.assert_within(dgt, dgt_o, orc.ce_prob_bound(dgt_o, lo), "d(sum dl^2)/dgt"))


# ---------------------------------------------------------------------------
# LSLR: (T, P)
# ---------------------------------------------------------------------------
LSLR_SHAPES = [(4, 1000), (1, 1), (3, 257), (128, 300),
               (2, 524_400),        # T*P > 1,048,576: forward second trip
               (2, 1_048_700)]      # P > 1,048,576: backward second trip


def lslr_inputs(shape):
    T, P = shape
    g = _gen(3000 + T + P % 1000)
    return (torch.randn(T, P, generator=g), torch.randn(T, P, generator=g),
            torch.rand(P, generator=g), torch.randn(T, P, generator=g))


def check_lslr(fn, shape, device, create_graph):
    """Forward (one fma: 2^-24 |ref|), then the backward with grad mode off
    (lslr_bwd_kernel) or under create_graph (the torch composition)."""
    T, P = shape
    arena, grad, lr, g = lslr_inputs(shape)
    a_, gr_, lr_ = (t.to(device).requires_grad_(True) for t in (arena, grad, lr))
    out = fn(a_, gr_, lr_)
    da, dgrad, dlr = torch.autograd.grad(out, (a_, gr_, lr_), g.to(device),
                                         create_graph=create_graph)
    ao, gro, lro, go = map(orc.widen, (arena, grad, lr, g))
    out_o = orc.lslr(ao, gro, lro)
    dgrad_o = -lro.unsqueeze(0) * go
    dlr_o = -(go * gro).sum(dim=0)
    assert torch.equal(da.detach().cpu(), g), "da is not the upstream grad bitwise"
    u = orc.EPS32
    return max(
        orc.assert_within(out, out_o, u * out_o.abs(), "out"),
        orc.assert_within(dgrad, dgrad_o, (2 if create_graph else 1) * u * dgrad_o.abs(),
                          "dgrad"),
        orc.assert_within(dlr, dlr_o, (T + 1) * u * (go * gro).abs().sum(dim=0), "dlr"))


def check_lslr_second_order(fn, device, shape=(3, 257)):
    """loss = sum dgrad^2 + sum dlr^2 of the create_graph backward,
    differentiated with respect to grad, lr and the upstream g; against the
    oracle at rtol 1e-5 + 1e-6 max|ref|."""
    arena, grad, lr, g = lslr_inputs(shape)

    def run(fn_, ts, dev):
        a_, gr_, lr_, g_ = (t.to(dev).requires_grad_(True) for t in ts)
        out = fn_(a_, gr_, lr_)
        _, dgrad, dlr = torch.autograd.grad(out, (a_, gr_, lr_), g_, create_graph=True)
        return torch.autograd.grad((dgrad ** 2).sum() + (dlr ** 2).sum(), (gr_, lr_, g_))

    got = run(fn, (arena, grad, lr, g), device)
    want = run(orc.lslr, tuple(map(orc.widen, (arena, grad, lr, g))), CPU)
    return max(orc.assert_within(a, r, 1e-5 * r.abs() + 1e-6 * r.abs().max(), name)
               for name, a, r in zip(("d/dgrad", "d/dlr", "d/dg"), got, want))


# ---------------------------------------------------------------------------
# Adam.  The kernel takes lr, betas, eps and the decay as fp32, so the tests
# pass the fp32 roundings of 0.1, (0.9, 0.999), 1e-8 and 0.01 to kernel and
# oracle alike: the oracle sees exactly what the kernel consumes.
# ---------------------------------------------------------------------------
def f32(x):
    return float(np.float32(x))


LR, BETA1, BETA2, ADAM_EPS, DECAY = f32(0.1), f32(0.9), f32(0.999), f32(1e-8), f32(0.01)
ADAM_STEPS = [1, 2, 1000, 100000]
FOUR = [(1000,), (64, 9), (7,), (3, 5, 5)]
TABLE32 = [(n,) for n in (1, 2, 3, 1, 255, 257, 1, 64) * 4]
LARGE = [(1_000_000,), (48_876,), (400,)]   # 1,048,576 + 700; a boundary 300 into trip 2
ADAM_SETS = {"four": FOUR, "table32": TABLE32, "large": LARGE}
_VARIANTS = [(None, 0.0), (1.5, 0.0), (None, DECAY), (1.5, DECAY)]
# (set, step, clamp, decay, what)
ADAM_CASES = (
    [(s, step, c, wd, "plain") for s in ("four", "table32")
     for step in ADAM_STEPS for c, wd in _VARIANTS]
    + [("large", 1, None, 0.0, "plain"), ("large", 2, 1.5, DECAY, "plain")]
    + [("four", step, None, 0.0, "zero_params") for step in ADAM_STEPS]
    + [("four", 2, 1.5, DECAY, "transposed_grad"), ("four", 2, 1.5, 0.0, "bf16_grad"),
       ("four", 1000, None, DECAY, "zero_params")]
)


def adam_inputs(set_name, what="plain"):
    """Tensor i is filled from its own range (g in 0.1 * [i, i + 0.5], p
    around -i, m and v scaled by i + 1), so an element attributed to the
    wrong table entry cannot pass; every seventh gradient of the longer
    tensors sits exactly at +-1.5 and the next one at +-4."""
    shapes = ADAM_SETS[set_name]
    g = _gen(4000 + len(shapes))
    ps, gs, ms, vs = [], [], [], []
    for i, s in enumerate(shapes):
        r = lambda: torch.rand(*s, generator=g)  # noqa: E731
        sign = 1.0 if i % 2 == 0 else -1.0
        gr = sign * 0.1 * (i + 0.5 * r())
        if gr.numel() >= 7:
            flat = gr.view(-1)
            flat[0::7] = 1.5 * sign
            flat[1::7] = -4.0 * sign
            flat[2::7] = torch.randn(flat[2::7].shape, generator=g)
        ps.append(torch.zeros(*s) if what == "zero_params" else -float(i) + r())
        ms.append(0.01 * (i + 1) * (r() - 0.3))
        vs.append(0.001 * (i + 1) * (r() + 0.01))
        if what == "bf16_grad":
            gr = gr.to(torch.bfloat16)
        elif what == "transposed_grad" and gr.dim() == 2:
            gr = gr.t().contiguous().t()        # same values, strides (1, rows)
            assert not gr.is_contiguous()
        gs.append(gr)
    return ps, gs, ms, vs


def check_adam_state(got, before, step, clamp, decay, lr=LR, beta1=BETA1,
                     beta2=BETA2, eps=ADAM_EPS):
    """``got`` = (ps, ms, vs) after the step, ``before`` = (ps, gs, ms, vs)."""
    worst = 0.0
    for i, (p, g, m, v) in enumerate(zip(*before)):
        ref, bound = orc.adam_bounds(orc.widen(p), orc.widen(g), orc.widen(m),
                                     orc.widen(v), step, lr, beta1, beta2, eps,
                                     decay, clamp)
        for k, name in enumerate(("p", "m", "v")):
            assert got[k][i].dtype == torch.float32
            worst = max(worst, orc.assert_within(got[k][i], ref[k], bound[k],
                                                 f"tensor {i} {name}"))
    return worst


def check_adam(fn, case, device):
    set_name, step, clamp, decay, what = case
    d1, d2, e_bc = orc.adam_bias_terms(BETA1, BETA2, step)
    print(f"step {step}: d1={d1:.3e} d2={d2:.3e} e_bc={e_bc:.3e}")
    before = adam_inputs(set_name, what)
    ps, gs, ms, vs = ([t.clone().to(device) for t in ts] for ts in before)
    fn(ps, gs, ms, vs, step=step, lr=LR, beta1=BETA1, beta2=BETA2, eps=ADAM_EPS,
       weight_decay=decay, clamp=clamp)
    for a, b in zip(gs, before[1]):
        assert torch.equal(a.cpu(), b), "the step wrote to a gradient"
    return check_adam_state((ps, ms, vs), before, step, clamp, decay)


def check_fused_adam_optimizer(device, clamp, decay):
    """Four FusedAdam steps from zero state, compared step by step: the
    oracle restarts from the implementation's own state before each step,
    so every step is held to the single-step bounds."""
    from howtotrainyourmamlpytorch_amd.meta.fused_adam import FusedAdam
    g = _gen(4100)
    params = [torch.nn.Parameter(torch.randn(*s, generator=g).to(device)) for s in FOUR]
    opt = FusedAdam(params, lr=LR, betas=(BETA1, BETA2), eps=ADAM_EPS,
                    weight_decay=decay, grad_clamp=clamp)
    worst = 0.0
    for step in range(1, 5):
        grads = [3.0 * torch.randn(*s, generator=g) for s in FOUR]
        for p, gr in zip(params, grads):
            p.grad = gr.to(device)
        state = [opt.state[p] for p in params]
        before = ([p.detach().cpu().clone() for p in params], grads,
                  [s["exp_avg"].cpu().clone() if s else torch.zeros_like(gr)
                   for s, gr in zip(state, grads)],
                  [s["exp_avg_sq"].cpu().clone() if s else torch.zeros_like(gr)
                   for s, gr in zip(state, grads)])
        opt.step()
        got = ([p.detach() for p in params],
               [opt.state[p]["exp_avg"] for p in params],
               [opt.state[p]["exp_avg_sq"] for p in params])
        assert all(int(opt.state[p]["step"].item()) == step for p in params)
        worst = max(worst, check_adam_state(got, before, step, clamp, decay))
    return worst
