"""Isolated kernel micro-benchmarks on flagship shapes (run on MI355X):

    python tools/bench_kernels.py
    python tools/bench_kernels.py --strided         # max_pooling=False stages
    python tools/bench_kernels.py --strided-model   # ... plus whole-model A/B
    python tools/bench_kernels.py --ln              # layer-norm kernels vs torch
    python tools/bench_kernels.py --ln-model        # ... plus whole-model A/B
    python tools/bench_kernels.py --wgrad           # wgrad v1 / v2 / v3 per shape
    python tools/bench_kernels.py --conv-input      # pad copy / first-layer fwd A/B
    python tools/bench_kernels.py --fconv           # fp32 conv trio vs grouped ATen
    python tools/bench_kernels.py --fconv-model     # fp32 modes, whole-model A/B
    python tools/bench_kernels.py --bn-pool-dbwd    # support BN+pool bwd / dbwd A/B

Prints per-kernel time, effective TFLOP/s (conv) or TB/s (memory-bound),
so optimization effort goes where the roofline says.
"""

import sys
import time

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from howtotrainyourmamlpytorch_amd import ops  # noqa: E402
from howtotrainyourmamlpytorch_amd.ops import hip_ext  # noqa: E402


def timeit(fn, reps=30, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def bench_conv(T, NB, H, W, C, F, tag):
    dev = torch.device("cuda")
    x = torch.randn(T, NB, H, W, C, device=dev).to(torch.bfloat16)
    w = torch.randn(T, F, C, 3, 3, device=dev)
    b = torch.randn(T, F, device=dev)
    ext = hip_ext()
    wp = ext.tconv_repack(w, False)
    wpd = ext.tconv_repack(w, True)
    y = ext.tconv_mm(x, wp, b, 1, H, W, False)[0]
    dy = torch.randn_like(y)

    flops = 2.0 * T * NB * H * W * F * 9 * C
    t_f = timeit(lambda: ext.tconv_mm(x, wp, b, 1, H, W, False))
    t_d = timeit(lambda: ext.tconv_mm(dy, wpd, None, 1, H, W, False))
    t_w = timeit(lambda: ext.tconv_wgrad(dy, x, 1, True))
    print(f"[conv {tag}] T{T} NB{NB} {H}x{W} C{C}->F{F}  "
          f"fwd {t_f*1e6:7.1f}us {flops/t_f/1e12:6.1f}TF | "
          f"dgrad {t_d*1e6:7.1f}us {flops/t_d/1e12:6.1f}TF | "
          f"wgrad {t_w*1e6:7.1f}us {flops/t_w/1e12:6.1f}TF")
    if C % 8 == 0:
        wp2 = ext.tconv_repack_v2(w, False)
        wpd2 = ext.tconv_repack_v2(w, True)
        t_f2 = timeit(lambda: ext.tconv_mm_v2(x, wp2, b, 1, H, W, F, False))
        t_d2 = timeit(lambda: ext.tconv_mm_v2(dy, wpd2, None, 1, H, W, C, False))
        print(f"[conv {tag}]   v2:                 "
              f"fwd {t_f2*1e6:7.1f}us {flops/t_f2/1e12:6.1f}TF | "
              f"dgrad {t_d2*1e6:7.1f}us {flops/t_d2/1e12:6.1f}TF")
    if F <= 64:
        t_w2 = timeit(lambda: ext.tconv_wgrad_v2(dy, x, 1, True))
        line = (f"[conv {tag}]   wgrad_v2:           "
                f"{t_w2*1e6:7.1f}us {flops/t_w2/1e12:6.1f}TF")
        if _v3_ok(C, F):
            line += " | " + _wgrad_v3_column(ext, dy, x, flops)
        print(line)


HBM_BPS = 6.3e12   # what the hardware sustains (profiles/README.md)


def _v3_ok(C, F):
    return F % 8 == 0 and F <= 64 and (C % 8 == 0 or C in (1, 3))


def _wgrad_v3_column(ext, dy, x, flops, t_w3=None):
    """Whole tconv_wgrad_v3 call (first-layer channel pad included) beside
    the whole v2 call: time, the call's byte floor (dY + X once at HBM
    rate) and the share of it reached, and the results compared at the
    size that is timed."""
    if t_w3 is None:
        t_w3 = timeit(lambda: ext.tconv_wgrad_v3(dy, x, 1, True))
    floor = (dy.numel() + x.numel()) * 2 / HBM_BPS
    dw2 = ext.tconv_wgrad_v2(dy, x, 1, True)[0]
    dw3 = ext.tconv_wgrad_v3(dy, x, 1, True)[0]
    return (f"wgrad_v3 {t_w3*1e6:7.1f}us {flops/t_w3/1e12:6.1f}TF "
            f"floor {floor*1e6:6.1f}us (floor/time {100*floor/t_w3:4.1f}%) "
            f"max|dw3-dw2| {(dw3 - dw2).abs().max().item():.3e} "
            f"max|dw2| {dw2.abs().max().item():.3e}")


def bench_wgrad(T, NB, H, W, C, F, tag):
    """wgrad v1 / v2 / v3 whole calls at one shape, interleaved."""
    dev = torch.device("cuda")
    ext = hip_ext()
    x = torch.randn(T, NB, H, W, C, device=dev).to(torch.bfloat16)
    dy = torch.randn(T, NB, H, W, F, device=dev).to(torch.bfloat16)
    flops = 2.0 * T * NB * H * W * F * 9 * C
    fns = [lambda: ext.tconv_wgrad(dy, x, 1, True),
           lambda: ext.tconv_wgrad_v2(dy, x, 1, True),
           lambda: ext.tconv_wgrad_v3(dy, x, 1, True)]
    # timed windows of some 20 ms of kernel work, whatever the shape
    reps = max(3, min(100, int(0.02 / timeit(fns[2], reps=2, warmup=1))))
    t1, t2, t3 = _median_rounds(fns, rounds=3, reps=reps, warmup=2)
    print(f"[wgrad {tag}] T{T} NB{NB} {H}x{W} C{C}->F{F} K={NB*H*W} | "
          f"v1 {t1*1e6:8.1f}us | v2 {t2*1e6:8.1f}us | "
          + _wgrad_v3_column(ext, dy, x, flops, t3)
          + f" | v3/v2 x{t2/t3:4.2f} v3/v1 x{t1/t3:4.2f}", flush=True)
    del x, dy
    torch.cuda.empty_cache()


def main_wgrad():
    for T in (128, 32):
        # mini-imagenet 5w1s: target pass (75 images), then support (5)
        bench_wgrad(T, 75, 84, 84, 3, 48, "mi-conv0-tgt")
        bench_wgrad(T, 75, 42, 42, 48, 48, "mi-conv1-tgt")
        bench_wgrad(T, 75, 21, 21, 48, 48, "mi-conv2-tgt")
        bench_wgrad(T, 75, 10, 10, 48, 48, "mi-conv3-tgt")
        bench_wgrad(T, 5, 84, 84, 3, 48, "mi-conv0-sup")
        bench_wgrad(T, 5, 42, 42, 48, 48, "mi-conv1-sup")
        bench_wgrad(T, 5, 21, 21, 48, 48, "mi-conv2-sup")
        bench_wgrad(T, 5, 10, 10, 48, 48, "mi-conv3-sup")
        # omniglot 20w5s: 100-image support and target passes
        bench_wgrad(T, 100, 28, 28, 1, 64, "om-conv0-tgt")
        bench_wgrad(T, 100, 14, 14, 64, 64, "om-conv1-tgt")
        bench_wgrad(T, 100, 7, 7, 64, 64, "om-conv2-tgt")
        bench_wgrad(T, 100, 3, 3, 64, 64, "om-conv3-tgt")


PEAK_F32 = 157.3e12   # fp32 vector / fp32 MFMA peak (FLOP/s)


def _with_env(name, value, fn):
    """fn under one setting of a per-call toggle (None = unset, the default)."""
    import os

    def run():
        if value is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = value
        try:
            return fn()
        finally:
            os.environ.pop(name, None)
    return run


def _reps_for(fn, window=0.02):
    return max(3, min(100, int(window / timeit(fn, reps=2, warmup=1))))


def bench_conv_input(T, NB, H, W, C, tag):
    """tconv_mm_v2 whole calls, forward and dgrad (C -> C, pad 1): zero-
    bordered copy + GEMM (MAML355_CONV_V2_NOPAD=0) against the GEMM reading
    the unpadded input, interleaved; results compared at the timed size."""
    dev = torch.device("cuda")
    ext = hip_ext()
    x = torch.randn(T, NB, H, W, C, device=dev).to(torch.bfloat16)
    w = torch.randn(T, C, C, 3, 3, device=dev).mul(0.1)
    b = torch.randn(T, C, device=dev)
    wp = ext.tconv_repack_v2(w, False)
    wpd = ext.tconv_repack_v2(w, True)
    flops = 2.0 * T * NB * H * W * C * 9 * C
    cols = []
    for name, call in (
            ("fwd", lambda: ext.tconv_mm_v2(x, wp, b, 1, H, W, C, False)[0]),
            ("dgrad", lambda: ext.tconv_mm_v2(x, wpd, None, 1, H, W, C, False)[0])):
        off = _with_env("MAML355_CONV_V2_NOPAD", "0", call)
        on = _with_env("MAML355_CONV_V2_NOPAD", None, call)
        same = torch.equal(off(), on())
        t0, t1 = _median_rounds([off, on], rounds=3, reps=_reps_for(on), warmup=2)
        cols.append(f"{name} pad+mm {t0*1e6:8.1f}us | mm {t1*1e6:8.1f}us "
                    f"{flops/t1/1e12:6.1f}TF x{t0/t1:4.2f} "
                    f"{'bitwise' if same else 'DIFFERENT'}")
    print(f"[conv-input {tag}] T{T} NB{NB} {H}x{W} C{C} | " + " | ".join(cols),
          flush=True)
    del x, w, wp, wpd
    torch.cuda.empty_cache()


def bench_dconv_fwd(T, NB, H, W, C, F, tag):
    """First-layer forward: vector-unit kernel (MAML355_DCONV_FWD_V2=0)
    against the fp32-MFMA kernel, with the store floor (Y bytes at the HBM
    rate) and the FMA floor (flops at the fp32 peak) beside them."""
    dev = torch.device("cuda")
    ext = hip_ext()
    x = torch.randn(T, NB, H, W, C, device=dev).to(torch.bfloat16)
    w = torch.randn(T, F, C, 3, 3, device=dev).mul(0.1)
    b = torch.randn(T, F, device=dev)
    call = lambda: ext.dconv_fwd(x, w, b, 1, H, W)  # noqa: E731
    off = _with_env("MAML355_DCONV_FWD_V2", "0", call)
    on = _with_env("MAML355_DCONV_FWD_V2", None, call)
    same = torch.equal(off(), on())
    t0, t1 = _median_rounds([off, on], rounds=3, reps=_reps_for(on), warmup=2)
    flops = 2.0 * T * NB * H * W * F * 9 * C
    st_floor = T * NB * H * W * F * 2 / HBM_BPS
    fma_floor = flops / PEAK_F32
    print(f"[dconv-fwd {tag}] T{T} NB{NB} {H}x{W} C{C}->F{F} | "
          f"old {t0*1e6:8.1f}us {flops/t0/1e12:5.1f}TF | "
          f"new {t1*1e6:8.1f}us {flops/t1/1e12:5.1f}TF x{t0/t1:4.2f} | "
          f"store floor {st_floor*1e6:7.1f}us FMA floor {fma_floor*1e6:7.1f}us "
          f"(new/max floor x{t1/max(st_floor, fma_floor):4.2f}) | "
          f"{'equal' if same else 'DIFFERENT'}", flush=True)
    del x, w
    torch.cuda.empty_cache()


def main_conv_input():
    for T in (128, 32):
        # mini-imagenet 5w1s conv layers 1-3: target (75 images), support (5)
        for nb, who in ((75, "tgt"), (5, "sup")):
            bench_conv_input(T, nb, 42, 42, 48, f"mi-conv1-{who}")
            bench_conv_input(T, nb, 21, 21, 48, f"mi-conv2-{who}")
            bench_conv_input(T, nb, 10, 10, 48, f"mi-conv3-{who}")
        # omniglot 20w5s: 100-image support and target passes
        bench_conv_input(T, 100, 14, 14, 64, "om-conv1")
        bench_conv_input(T, 100, 7, 7, 64, "om-conv2")
        bench_conv_input(T, 100, 3, 3, 64, "om-conv3")
        bench_dconv_fwd(T, 75, 84, 84, 3, 48, "mi-conv0-tgt")
        bench_dconv_fwd(T, 5, 84, 84, 3, 48, "mi-conv0-sup")
        bench_dconv_fwd(T, 100, 28, 28, 1, 64, "om-conv0")


def bench_bn(T, M, C, tag):
    dev = torch.device("cuda")
    x = torch.randn(T, M, C, device=dev).to(torch.bfloat16)
    gamma = torch.rand(C, device=dev) + 0.5
    beta = torch.randn(C, device=dev)
    ext = hip_ext()
    y, mean, var, rstd = ext.bn_act_fwd(x, gamma, beta, 1e-5, 0.01, True)
    dy = torch.randn_like(y)
    nbytes = T * M * C * 2
    t_f = timeit(lambda: ext.bn_act_fwd(x, gamma, beta, 1e-5, 0.01, True))
    t_b = timeit(lambda: ext.bn_act_bwd(dy, x, mean, rstd, gamma, beta, 0.01, True))
    # fwd: read x twice (sums+norm) + write y; bwd: read dy,x twice + write dx
    print(f"[bn {tag}] T{T} M{M} C{C}  fwd {t_f*1e6:6.1f}us "
          f"{3*nbytes/t_f/1e12:5.2f}TB/s | bwd {t_b*1e6:6.1f}us "
          f"{5*nbytes/t_b/1e12:5.2f}TB/s")


def bench_pool(N, H, W, C, tag):
    dev = torch.device("cuda")
    x = torch.randn(N, H, W, C, device=dev).to(torch.bfloat16)
    ext = hip_ext()
    y, mask = ext.maxpool2x2_fwd(x)
    dy = torch.randn_like(y)
    nbytes = N * H * W * C * 2
    t_f = timeit(lambda: ext.maxpool2x2_fwd(x))
    t_b = timeit(lambda: ext.maxpool2x2_bwd(dy, mask, H, W))
    print(f"[pool {tag}] N{N} {H}x{W} C{C}  fwd {t_f*1e6:6.1f}us "
          f"{1.625*nbytes/t_f/1e12:5.2f}TB/s | bwd {t_b*1e6:6.1f}us "
          f"{1.875*nbytes/t_b/1e12:5.2f}TB/s")


def _median_rounds(fns, rounds=5, reps=20, warmup=5):
    """Interleaved A/B timing: every round times each variant once, so
    clock and neighbour noise hit all of them alike; returns the median
    per-call time of each variant."""
    for fn in fns:
        timeit(fn, reps=warmup, warmup=0)
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            ts[i].append(timeit(fn, reps=reps, warmup=1))
    return [sorted(t)[len(t) // 2] for t in ts]


def bench_sconv(T, NB, H, W, C, F, tag, pad=1):
    """Stride-2 conv trio (sconv.hip, through the same entry points the
    autograd Functions use, repack and first-layer channel pad included)
    against the grouped-ATen composition ``ref.task_conv3x3(stride=2)`` in
    bf16 at the same shape — fwd, dgrad and wgrad timed separately."""
    from howtotrainyourmamlpytorch_amd.ops import reference as ref
    dev = torch.device("cuda")
    ext = hip_ext()
    x = torch.randn(T, NB, H, W, C, device=dev).to(torch.bfloat16)
    w = torch.randn(T, F, C, 3, 3, device=dev).mul(0.1)
    b = torch.randn(T, F, device=dev)
    Ho, Wo = (H + 2 * pad - 3) // 2 + 1, (W + 2 * pad - 3) // 2 + 1
    dy = torch.randn(T, NB, Ho, Wo, F, device=dev).to(torch.bfloat16)
    flops = 2.0 * T * NB * Ho * Wo * F * 9 * C
    first = C < 8   # first layer: no dgrad in the net (x is the image)

    def k_fwd():
        with torch.no_grad():
            ops.task_conv3x3(x, w, b, stride=2, padding=pad)

    xk = torch.nn.functional.pad(x, (0, 8 - C)) if first else x
    wk = torch.nn.functional.pad(w, (0, 0, 0, 0, 0, 8 - C)) if first else w

    def k_dgrad():
        ext.sconv_dgrad(dy, ext.sconv_repack(wk, True), pad, H, W)

    def k_wgrad():
        ext.sconv_wgrad(dy, xk, pad, True)

    xr = x.clone().requires_grad_(True)
    wr = w.to(torch.bfloat16).requires_grad_(True)
    br = b.to(torch.bfloat16).requires_grad_(True)
    yr = ref.task_conv3x3(xr, wr, br, 2, pad)

    def r_fwd():
        with torch.no_grad():
            ref.task_conv3x3(x, w.to(torch.bfloat16), b.to(torch.bfloat16), 2, pad)

    def r_dgrad():
        torch.autograd.grad(yr, xr, dy, retain_graph=True)

    def r_wgrad():
        torch.autograd.grad(yr, (wr, br), dy, retain_graph=True)

    kf, rf = _median_rounds([k_fwd, r_fwd])
    kw, rw = _median_rounds([k_wgrad, r_wgrad])
    line = (f"[sconv {tag}] T{T} NB{NB} {H}x{W} C{C}->F{F} | "
            f"fwd kernel {kf*1e6:7.1f}us {flops/kf/1e12:5.1f}TF "
            f"fallback {rf*1e6:8.1f}us x{rf/kf:5.1f} | ")
    if first:
        line += "dgrad n/a (image input) | "
    else:
        kd, rd = _median_rounds([k_dgrad, r_dgrad])
        line += (f"dgrad kernel {kd*1e6:7.1f}us {flops/kd/1e12:5.1f}TF "
                 f"fallback {rd*1e6:8.1f}us x{rd/kd:5.1f} | ")
    line += (f"wgrad kernel {kw*1e6:7.1f}us {flops/kw/1e12:5.1f}TF "
             f"fallback {rw*1e6:8.1f}us x{rw/kw:5.1f}")
    print(line, flush=True)


def bench_gavgpool(N, H, W, C, tag):
    dev = torch.device("cuda")
    ext = hip_ext()
    x = torch.randn(N, H, W, C, device=dev).to(torch.bfloat16)
    dy = torch.randn(N, C, device=dev).to(torch.bfloat16)
    kf, rf = _median_rounds([lambda: ext.gavgpool_fwd(x),
                             lambda: x.mean(dim=(1, 2))])
    kb, rb = _median_rounds([
        lambda: ext.gavgpool_bwd(dy, H, W),
        lambda: (dy.view(N, 1, 1, C) / (H * W)).expand(N, H, W, C).contiguous()])
    print(f"[gavgpool {tag}] N{N} {H}x{W} C{C} | fwd kernel {kf*1e6:6.1f}us "
          f"x.mean {rf*1e6:6.1f}us | bwd kernel {kb*1e6:6.1f}us "
          f"torch {rb*1e6:6.1f}us", flush=True)


def bench_ln(T, NS, H, W, C, tag, rounds=3, reps=5):
    """Layer-norm + bias + leaky-ReLU (layernorm.hip) fwd, bwd and dbwd in
    bf16 against the torch composition ``ref.task_layer_norm_act`` and what
    autograd composes from it — the routing the kernels replace.  Shared
    [H, W, C] bias (the default, meta-only form)."""
    from howtotrainyourmamlpytorch_amd.ops import reference as ref
    dev = torch.device("cuda")
    ext = hip_ext()
    D = H * W * C
    x = torch.randn(T, NS, H, W, C, device=dev).to(torch.bfloat16)
    bias = torch.randn(H, W, C, device=dev)
    dy = torch.randn(T, NS, H, W, C, device=dev).to(torch.bfloat16)
    gx = torch.randn(T, NS, H, W, C, device=dev).to(torch.bfloat16)
    gb = torch.randn(H, W, C, device=dev)
    gb_t = gb.reshape(1, D).expand(T, D).contiguous()
    b1 = bias.reshape(D)
    _, mean, rstd = ext.ln_act_fwd(x, b1, 1e-5, 0.01, True)
    nbytes = T * NS * D * 2

    def k_fwd():
        ext.ln_act_fwd(x, b1, 1e-5, 0.01, True)

    def k_bwd():
        ext.ln_act_bwd(dy, x, mean, rstd, b1, 0.01, True)

    def k_dbwd():
        ext.ln_act_dbwd(x, dy, gx, gb_t, mean, rstd, b1, 0.01, True)

    def r_fwd():
        with torch.no_grad():
            ref.task_layer_norm_act(x, None, bias, 1e-5, 0.01, True)

    head = f"[ln {tag}] T{T} NS{NS} {H}x{W}x{C} (D={D}, {T * NS} images)"
    # timed windows of some 50 ms of kernel work, whatever the shape
    reps = max(reps, min(200, int(0.05 / timeit(k_dbwd, reps=3, warmup=2))))
    kf, rf = _median_rounds([k_fwd, r_fwd], rounds, reps, 2)
    # kernel passes over the data — fwd: x twice, y; bwd: x and dy twice, dx,
    # x and dy again for dbias; dbwd: x, dy, gx twice, d_dy, d_x
    print(f"{head} | fwd kernel {kf*1e6:9.1f}us {3*nbytes/kf/1e12:5.2f}TB/s "
          f"composition {rf*1e6:10.1f}us x{rf/kf:5.1f}", flush=True)

    def composition():
        xr = x.clone().requires_grad_(True)
        br = bias.clone().requires_grad_(True)
        ur = dy.clone().requires_grad_(True)
        yr = ref.task_layer_norm_act(xr, None, br, 1e-5, 0.01, True)

        def r_bwd():
            torch.autograd.grad(yr, (xr, br), dy, retain_graph=True)

        kb, rb = _median_rounds([k_bwd, r_bwd], rounds, reps, 2)
        print(f"{head} | bwd kernel {kb*1e6:9.1f}us {7*nbytes/kb/1e12:5.2f}TB/s "
              f"composition {rb*1e6:10.1f}us x{rb/kb:5.1f}", flush=True)
        dxr, dbr = torch.autograd.grad(yr, (xr, br), ur, create_graph=True)

        def r_dbwd():
            torch.autograd.grad((dxr, dbr), (ur, xr), (gx, gb), retain_graph=True)

        kd, rd = _median_rounds([k_dbwd, r_dbwd], rounds, reps, 2)
        print(f"{head} | dbwd kernel {kd*1e6:9.1f}us {8*nbytes/kd/1e12:5.2f}TB/s "
              f"composition {rd*1e6:10.1f}us x{rd/kd:5.1f}", flush=True)

    try:
        composition()
        return
    except torch.cuda.OutOfMemoryError:
        pass
    torch.cuda.empty_cache()
    print(f"{head} | the composition's autograd graph does not fit in memory "
          f"at this size; kernels alone:", flush=True)
    kb, = _median_rounds([k_bwd], rounds, reps, 2)
    kd, = _median_rounds([k_dbwd], rounds, reps, 2)
    print(f"{head} | bwd kernel {kb*1e6:9.1f}us {7*nbytes/kb/1e12:5.2f}TB/s | "
          f"dbwd kernel {kd*1e6:9.1f}us {8*nbytes/kd/1e12:5.2f}TB/s", flush=True)


def bench_ln_model(model_name, tasks_per_gpu, steps=3, warmup=2, rounds=3):
    """Whole-model second-order MSL step of the layer-norm backbone on
    synthetic episodes (bench.py's configuration with --norm_layer
    layer_norm): the kernels against the torch composition they replace,
    interleaved in one process."""
    import argparse
    import bench
    from howtotrainyourmamlpytorch_amd.data import SyntheticEpisodeStream
    from howtotrainyourmamlpytorch_amd.meta.engine import MAMLFewShotClassifier
    from howtotrainyourmamlpytorch_amd.ops import reference as ref

    cli = argparse.Namespace(model=model_name, tasks_per_gpu=tasks_per_gpu,
                             inner_steps=5, second_order="True")
    args = bench.build_args(cli, 1)
    args.norm_layer = "layer_norm"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = MAMLFewShotClassifier(
        im_shape=(2, args.image_channels, args.image_height, args.image_width),
        device=dev, args=args)
    stream = SyntheticEpisodeStream(args)
    batches = [tuple(t.to(dev) for t in b) for b in stream.get_train_batches(4)]
    kernel_ln = ops.task_layer_norm_act

    def run(old):
        ops.task_layer_norm_act = ref.task_layer_norm_act if old else kernel_ln
        try:
            for i in range(warmup):
                model.run_train_iter(batches[i % 4], epoch=0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                model.run_train_iter(batches[i % 4], epoch=0)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps
        finally:
            ops.task_layer_norm_act = kernel_ln

    tk, to = [], []
    try:
        for _ in range(rounds):
            tk.append(run(False))
            to.append(run(True))
    except torch.cuda.OutOfMemoryError:
        print(f"[ln model {model_name}] {tasks_per_gpu} tasks/step: out of "
              f"memory (kernel runs so far: {tk})", flush=True)
        return
    mk, mo = sorted(tk)[len(tk) // 2], sorted(to)[len(to) // 2]
    print(f"[ln model {model_name}] {tasks_per_gpu} tasks/step, 2nd order "
          f"MSL | kernels {mk*1e3:8.1f} ms/step {tasks_per_gpu/mk:7.1f} tasks/s | "
          f"torch composition {mo*1e3:8.1f} ms/step "
          f"{tasks_per_gpu/mo:7.1f} tasks/s | x{mo/mk:.2f}", flush=True)


def main_ln():
    # stage-0 layer norm of the two bench workloads at bench.py's 128 tasks
    # per GPU; the support pass of the second is the few-large-images case
    # that is split over workgroups
    bench_ln(128, 20, 28, 28, 64, "om-20w5s-s0-tgt")
    bench_ln(128, 75, 84, 84, 48, "mi-5w1s-s0-tgt")
    bench_ln(128, 5, 84, 84, 48, "mi-5w1s-s0-sup")
    bench_ln(8, 5, 84, 84, 48, "mi-5w1s-s0-sup-8tasks")
    if "--ln-model" in sys.argv:
        bench_ln_model("maml++_omniglot_20w5s", 16)
        bench_ln_model("maml++_miniimagenet_5w1s", 16)


def bench_strided_model(model_name, tasks_per_gpu, steps=3, warmup=2, rounds=3):
    """Whole-model second-order MSL step of the max_pooling=False backbone
    on synthetic episodes (bench.py's configuration with that one flag
    flipped): the kernel routing against the routing it replaces (grouped-
    ATen stride-2 conv + x.mean pool), interleaved in one process."""
    import argparse
    import bench
    from howtotrainyourmamlpytorch_amd.data import SyntheticEpisodeStream
    from howtotrainyourmamlpytorch_amd.meta.engine import MAMLFewShotClassifier
    from howtotrainyourmamlpytorch_amd.ops import hip_autograd
    from howtotrainyourmamlpytorch_amd.ops import reference as ref

    cli = argparse.Namespace(model=model_name, tasks_per_gpu=tasks_per_gpu,
                             inner_steps=5, second_order="True")
    args = bench.build_args(cli, 1)
    args.max_pooling = False
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = MAMLFewShotClassifier(
        im_shape=(2, args.image_channels, args.image_height, args.image_width),
        device=dev, args=args)
    stream = SyntheticEpisodeStream(args)
    batches = [tuple(t.to(dev) for t in b) for b in stream.get_train_batches(4)]

    kernel_conv, kernel_pool = hip_autograd.task_conv3x3, ops.task_global_avgpool

    def old_conv(x, w, b=None, stride=1, padding=1, return_stats=False):
        if stride == 1:
            return kernel_conv(x, w, b, stride, padding, return_stats)
        y = ref.task_conv3x3(x, w.to(x.dtype),
                             b.to(x.dtype) if b is not None else None,
                             stride, padding)
        return (y, None) if return_stats else y

    def run(old):
        hip_autograd.task_conv3x3 = old_conv if old else kernel_conv
        ops.task_global_avgpool = ref.task_global_avgpool if old else kernel_pool
        try:
            for i in range(warmup):
                model.run_train_iter(batches[i % 4], epoch=0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                model.run_train_iter(batches[i % 4], epoch=0)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps
        finally:
            hip_autograd.task_conv3x3 = kernel_conv
            ops.task_global_avgpool = kernel_pool

    tk, to = [], []
    for _ in range(rounds):
        tk.append(run(False))
        to.append(run(True))
    mk, mo = sorted(tk)[len(tk) // 2], sorted(to)[len(to) // 2]
    print(f"[strided model {model_name}] {tasks_per_gpu} tasks/step, 2nd order "
          f"MSL | kernels {mk*1e3:8.1f} ms/step {tasks_per_gpu/mk:7.1f} tasks/s | "
          f"grouped-ATen routing {mo*1e3:8.1f} ms/step "
          f"{tasks_per_gpu/mo:7.1f} tasks/s | x{mo/mk:.2f}", flush=True)


def main_strided(with_model):
    # mini-imagenet strided stages 84->42->21->11->6, target pass
    bench_sconv(8, 75, 84, 84, 3, 48, "mi-s0-tgt")
    bench_sconv(8, 75, 42, 42, 48, 48, "mi-s1-tgt")
    bench_sconv(8, 75, 21, 21, 48, 48, "mi-s2-tgt")
    bench_sconv(8, 75, 11, 11, 48, 48, "mi-s3-tgt")
    # omniglot 20w5s strided stages 28->14->7->4->2, 100-image support
    bench_sconv(8, 100, 28, 28, 1, 64, "om-s0-sup")
    bench_sconv(8, 100, 14, 14, 64, 64, "om-s1-sup")
    bench_sconv(8, 100, 7, 7, 64, 64, "om-s2-sup")
    bench_sconv(8, 100, 4, 4, 64, 64, "om-s3-sup")
    bench_gavgpool(8 * 75, 6, 6, 48, "mi-tgt")
    bench_gavgpool(8 * 100, 2, 2, 64, "om-sup")
    if with_model:
        bench_strided_model("maml++_miniimagenet_5w1s", 128)
        bench_strided_model("maml++_omniglot_20w5s", 128)


FP32_MATRIX_PEAK = 157.3e12   # v_mfma_f32_16x16x4_f32, spec


def bench_fconv(T, NB, H, W, C, F, tag, pad=1):
    """fp32 stride-1 conv trio (fconv.hip, through the entry points the
    autograd Functions use, repack included) against the grouped-ATen
    forward ``ref.task_conv3x3`` and its autograd backward on the same fp32
    tensors.  Per call: ms, TF, the fraction of the fp32 matrix peak and the
    fraction of the byte floor (every operand and the result once over HBM)."""
    from howtotrainyourmamlpytorch_amd.ops import reference as ref
    dev = torch.device("cuda")
    ext = hip_ext()
    x = torch.randn(T, NB, H, W, C, device=dev)
    w = torch.randn(T, F, C, 3, 3, device=dev).mul(0.1)
    b = torch.randn(T, F, device=dev)
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    dy = torch.randn(T, NB, Ho, Wo, F, device=dev)
    flops = 2.0 * T * NB * Ho * Wo * F * 9 * C
    nbytes = 4.0 * (x.numel() + dy.numel() + w.numel())
    first = C < 8   # first layer: no dgrad in the net (x is the image)

    def k_fwd():
        ext.fconv_mm(x, ext.fconv_repack(w, False), b, pad, Ho, Wo)

    def k_dgrad():
        ext.fconv_mm(dy, ext.fconv_repack(w, True), None, 2 - pad, H, W)

    def k_wgrad():
        ext.fconv_wgrad(dy, x, pad, True)

    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True)
    yr = ref.task_conv3x3(xr, wr, br, 1, pad)

    def r_fwd():
        with torch.no_grad():
            ref.task_conv3x3(x, w, b, 1, pad)

    def r_dgrad():
        torch.autograd.grad(yr, xr, dy, retain_graph=True)

    def r_wgrad():
        torch.autograd.grad(yr, (wr, br), dy, retain_graph=True)

    def col(name, k, r):
        return (f"{name} kernel {k*1e3:7.3f}ms {flops/k/1e12:5.1f}TF "
                f"{100*flops/k/FP32_MATRIX_PEAK:4.1f}%peak "
                f"{100*nbytes/HBM_BPS/k:4.1f}%bytefloor | "
                f"ATen {r*1e3:8.3f}ms x{r/k:5.1f}")

    kf, rf = _median_rounds([k_fwd, r_fwd], rounds=3, reps=5, warmup=2)
    kw, rw = _median_rounds([k_wgrad, r_wgrad], rounds=3, reps=5, warmup=2)
    line = f"[fconv {tag}] T{T} NB{NB} {H}x{W} C{C}->F{F} | " + col("fwd", kf, rf)
    if first:
        line += " | dgrad n/a (image input)"
    else:
        kd, rd = _median_rounds([k_dgrad, r_dgrad], rounds=3, reps=5, warmup=2)
        line += " | " + col("dgrad", kd, rd)
    line += " | " + col("wgrad", kw, rw)
    print(line, flush=True)


def bench_fconv_model(model_name, tasks_per_gpu, mode, steps=3, warmup=2,
                      rounds=3):
    """Whole-model second-order MSL step with fp32 activations on synthetic
    episodes (bench.py's configuration plus ``mode``: "support" =
    --fp32_support_pass True, "fp32" = --compute_dtype fp32): the fp32
    kernels against MAML355_FCONV=0, alternating rounds in one process.
    Prints every round, so the spread between rounds can be read off."""
    import argparse
    import os
    import bench
    from howtotrainyourmamlpytorch_amd.data import SyntheticEpisodeStream
    from howtotrainyourmamlpytorch_amd.meta.engine import MAMLFewShotClassifier

    cli = argparse.Namespace(model=model_name, tasks_per_gpu=tasks_per_gpu,
                             inner_steps=5, second_order="True")
    args = bench.build_args(cli, 1)
    if mode == "support":
        args.fp32_support_pass = True
    else:
        args.compute_dtype = "fp32"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = MAMLFewShotClassifier(
        im_shape=(2, args.image_channels, args.image_height, args.image_width),
        device=dev, args=args)
    stream = SyntheticEpisodeStream(args)
    batches = [tuple(t.to(dev) for t in b) for b in stream.get_train_batches(4)]
    saved = os.environ.get("MAML355_FCONV")

    def run(old):
        import warnings
        os.environ["MAML355_FCONV"] = "0" if old else "1"
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")   # the A/B side warns
                for i in range(warmup):
                    model.run_train_iter(batches[i % 4], epoch=0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(steps):
                    model.run_train_iter(batches[i % 4], epoch=0)
                torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps
        finally:
            if saved is None:
                os.environ.pop("MAML355_FCONV", None)
            else:
                os.environ["MAML355_FCONV"] = saved

    tk, to = [], []
    try:
        for _ in range(rounds):
            tk.append(run(False))
            to.append(run(True))
    except torch.cuda.OutOfMemoryError:
        print(f"[fconv model {model_name} {mode}] {tasks_per_gpu} tasks/step: "
              f"out of memory (kernel runs so far: {tk})", flush=True)
        return
    mk, mo = sorted(tk)[len(tk) // 2], sorted(to)[len(to) // 2]
    rk = " ".join(f"{1/t:.3f}" for t in tk)
    ro = " ".join(f"{1/t:.3f}" for t in to)
    spread = max(max(tk) - min(tk), max(to) - min(to))
    print(f"[fconv model {model_name} {mode}] {tasks_per_gpu} tasks/step, 2nd "
          f"order MSL | kernels {1/mk:.3f} steps/s (rounds {rk}) | "
          f"MAML355_FCONV=0 {1/mo:.3f} steps/s (rounds {ro}) | x{mo/mk:.2f}; "
          f"difference {abs(mo-mk)*1e3:.1f} ms/step vs 3x round spread "
          f"{3*spread*1e3:.1f} ms/step", flush=True)


def main_fconv(with_model):
    if "--fconv" in sys.argv:
        # support-pass shapes: mini-imagenet 5w1s at 128 tasks (5 images)
        bench_fconv(128, 5, 84, 84, 3, 48, "mi-s0-sup")
        bench_fconv(128, 5, 42, 42, 48, 48, "mi-s1-sup")
        bench_fconv(128, 5, 21, 21, 48, 48, "mi-s2-sup")
        bench_fconv(128, 5, 10, 10, 48, 48, "mi-s3-sup")
        # omniglot 20w5s at 32 tasks (100 images)
        bench_fconv(32, 100, 28, 28, 1, 64, "om-s0-sup")
        bench_fconv(32, 100, 14, 14, 64, 64, "om-s1-sup")
        bench_fconv(32, 100, 7, 7, 64, 64, "om-s2-sup")
        bench_fconv(32, 100, 3, 3, 64, 64, "om-s3-sup")
    if with_model:
        # the task counts of the per-call shapes above: 128 and 32 per step
        for mode in ("support", "fp32"):
            bench_fconv_model("maml++_miniimagenet_5w1s", 128, mode)
            bench_fconv_model("maml++_omniglot_20w5s", 32, mode)


def bench_bn_pool_dbwd(T, NB, H, W, C, tag):
    """Support-side BN+act+pool block under create_graph: the whole first
    backward and the whole double-backward, native path against
    MAML355_BNPOOL_DBWD=0 (torch.gather glue, tensor formula for d_gamma,
    scalar sums kernel), interleaved.  The first backward is the same
    composition in both; it is timed as the control.
    Floor: the bytes the result needs at 6.3 TB/s — backward: x twice, the
    pooled dy and mask twice, dx once; double-backward: x and gx twice, the
    pooled dy and mask twice, d_x and the pooled d_dy once."""
    import os
    dev = torch.device("cuda")
    env = "MAML355_BNPOOL_DBWD"
    Ho, Wo = H // 2, W // 2
    x = torch.randn(T, NB, H, W, C, device=dev).to(torch.bfloat16).requires_grad_(True)
    gam = (torch.rand(T, C, device=dev) + 0.5).requires_grad_(True)
    bet = torch.randn(T, C, device=dev).requires_grad_(True)
    gy = torch.randn(T, NB, Ho, Wo, C, device=dev).to(torch.bfloat16).requires_grad_(True)
    rx = torch.randn(T, NB, H, W, C, device=dev).to(torch.bfloat16)
    rg, rb = torch.randn(T, C, device=dev), torch.randn(T, C, device=dev)
    y, _, _ = ops.task_bn_act_pool(x, gam, bet, 1e-5, 0.01)

    def first(flag):
        def run():
            os.environ[env] = flag
            return torch.autograd.grad(y, (x, gam, bet), gy, create_graph=True,
                                       retain_graph=True)
        return run

    def second(flag):
        os.environ[env] = flag
        outs = first(flag)()

        def run():
            os.environ[env] = flag
            return torch.autograd.grad(outs, (x, gy, gam), (rx, rg, rb),
                                       retain_graph=True)
        return run

    try:
        same = all(torch.equal(a, b) for a, b in
                   zip(first("1")() + second("1")(), first("0")() + second("0")()))
        b0, b1 = _median_rounds([first("0"), first("1")], rounds=3, reps=5, warmup=2)
        d0, d1 = _median_rounds([second("0"), second("1")], rounds=3, reps=5, warmup=2)
    finally:
        os.environ.pop(env, None)
    n = 2.0 * T * NB * H * W * C            # one full-resolution bf16 tensor
    p = 3.0 * T * NB * Ho * Wo * C          # pooled bf16 tensor + its mask
    fb, fd = (3 * n + 2 * p) / 6.3e12, (6 * n + 2 * p + p * 2 / 3) / 6.3e12
    print(f"[bn-pool-dbwd {tag}] T{T} NB{NB} {H}x{W} C{C} bits_equal={same} | "
          f"bwd composed {b0*1e6:7.1f}us native {b1*1e6:7.1f}us x{b0/b1:4.2f} "
          f"floor {fb*1e6:6.1f}us ratio {b1/fb:4.1f} | dbwd composed "
          f"{d0*1e6:7.1f}us native {d1*1e6:7.1f}us x{d0/d1:4.2f} "
          f"floor {fd*1e6:6.1f}us ratio {d1/fd:4.1f}", flush=True)


def main_bn_pool_dbwd():
    # the four support stages: mini-imagenet 5w1s at 128 tasks (5 images),
    # omniglot 20w5s at 32 tasks (100 images)
    for hw in (84, 42, 21, 10):
        bench_bn_pool_dbwd(128, 5, hw, hw, 48, f"mi-{hw}")
    for hw in (28, 14, 7, 3):
        bench_bn_pool_dbwd(32, 100, hw, hw, 64, f"om-{hw}")


def main():
    assert torch.cuda.is_available()
    print(torch.cuda.get_device_name(0))
    if "--bn-pool-dbwd" in sys.argv:
        main_bn_pool_dbwd()
        return
    if "--fconv" in sys.argv or "--fconv-model" in sys.argv:
        main_fconv("--fconv-model" in sys.argv)
        return
    if "--ln" in sys.argv or "--ln-model" in sys.argv:
        main_ln()
        return
    if "--wgrad" in sys.argv:
        main_wgrad()
        return
    if "--conv-input" in sys.argv:
        main_conv_input()
        return
    if "--strided" in sys.argv or "--strided-model" in sys.argv:
        # max_pooling=False backbone only: kernels vs the routing they replace
        main_strided("--strided-model" in sys.argv)
        return
    # mini-imagenet flagship: 8 tasks/GPU, target pass (75 imgs/task)
    bench_conv(8, 75, 84, 84, 3, 48, "mi-conv0-tgt")
    bench_conv(128, 75, 84, 84, 3, 48, "mi-conv0-tgt-128")
    bench_conv(8, 75, 42, 42, 48, 48, "mi-conv1-tgt")
    bench_conv(8, 75, 21, 21, 48, 48, "mi-conv2-tgt")
    bench_conv(8, 5, 42, 42, 48, 48, "mi-conv1-sup")
    # omniglot 20w5s: 100-image support
    bench_conv(8, 100, 28, 28, 64, 64, "om-conv1-sup")
    bench_bn(8, 75 * 42 * 42, 48, "mi-bn1-tgt")
    bench_bn(8, 100 * 28 * 28, 64, "om-bn1")
    bench_pool(8 * 75, 84, 84, 48, "mi-pool0-tgt")
    bench_conv0_wrapper(8, 75, 84, 84, 3, 48, "mi-conv0-tgt")
    bench_conv0_wrapper(8, 100, 28, 28, 1, 64, "om-conv0-sup")




def bench_conv0_wrapper(T, NB, H, W, C, F, tag):
    """First-layer conv through the dispatch wrapper (exercises the
    channel-pad-to-8 path): fwd and fwd+wgrad."""
    dev = torch.device("cuda")
    x = torch.randn(T, NB, H, W, C, device=dev).to(torch.bfloat16)
    w = torch.randn(T, F, C, 3, 3, device=dev, requires_grad=True)
    b = torch.randn(T, F, device=dev, requires_grad=True)
    flops = 2.0 * T * NB * H * W * F * 9 * C
    t_f = timeit(lambda: ops.task_conv3x3(x, w, b), reps=20)

    def fb():
        y = ops.task_conv3x3(x, w, b)
        torch.autograd.grad(y.float().sum(), [w, b])
    t_fb = timeit(fb, reps=20)
    print(f"[conv0w {tag}] T{T} NB{NB} {H}x{W} C{C}->F{F}  "
          f"fwd {t_f*1e6:7.1f}us {flops/t_f/1e12:6.1f}TF | "
          f"fwd+wgrad {t_fb*1e6:7.1f}us")


if __name__ == "__main__":
    main()
