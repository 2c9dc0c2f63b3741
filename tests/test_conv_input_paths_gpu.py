"""The two ways operands reach the conv kernels must give the same bits.

``tconv_mm_v2`` reads the unpadded input and sends border taps to the zero
page (default) or runs on a zero-bordered copy (MAML355_CONV_V2_NOPAD=0): a
zero is the same MFMA operand either way, so Y is compared with
``torch.equal``, forward and dgrad.  ``dconv_fwd`` runs the fp32 chain
``acc = bias; acc = fmaf(x, w, acc)`` over (ky, kx, c) on the fp32 matrix
unit (default for C in {1, 3}) or on the vector unit
(MAML355_DCONV_FWD_V2=0); the two may differ in the sign of a zero only,
which ``torch.equal`` does not see.  The values themselves are checked
against the float64 oracle by tests/test_tconv_shapes_gpu.py, which runs the
defaults; the address logic is walked on the CPU by
tests/test_tconv_mm_addr.py."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from howtotrainyourmamlpytorch_amd import ops

_ENV = ("MAML355_CONV_V2_NOPAD", "MAML355_CONV_V2_SBUF",
        "MAML355_DCONV_FWD_V2", "MAML355_DETERMINISTIC")


def dev():
    return torch.device("cuda", 0)


def _id(s):
    return "x".join(map(str, s))


def _mk(T, NB, H, W, C, F, pad, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, NB, H, W, C, generator=g).to(torch.bfloat16)
    w = torch.randn(T, F, C, 3, 3, generator=g).mul(0.1)
    b = torch.randn(T, F, generator=g)
    dy = torch.randn(T, NB, H + 2 * pad - 2, W + 2 * pad - 2, F,
                     generator=g).to(torch.bfloat16)
    assert (x != 0).all() and (w != 0).all() and (dy != 0).all()
    return x.to(dev()), w.to(dev()), b.to(dev()), dy.to(dev())


def _both(monkeypatch, name, fn):
    """fn() with toggle `name` off ("0"), then at its default."""
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(name, "0")
    off = fn()
    monkeypatch.delenv(name)
    on = fn()
    torch.cuda.synchronize()
    return off, on


# (T, NB, H, W, C, F, pad)
MM_SHAPES = [
    (2, 3, 11, 9, 48, 48, 1),     # odd, non-square
    (2, 3, 12, 11, 64, 64, 0),    # no border forward, two-deep border in dgrad
    (2, 3, 7, 7, 8, 8, 1),        # K9 = 72: K-tail and border in one step
    (1, 2, 3, 3, 16, 32, 0),      # Ho = Wo = 1
    (1, 1, 1, 1, 8, 8, 1),        # every tap but the centre is border
    (3, 7, 21, 21, 48, 48, 1),    # 3087 rows: seams inside a tile, ragged end
    (2, 3, 10, 10, 16, 48, 1),    # C != F
]


@pytest.mark.parametrize("shape", MM_SHAPES, ids=_id)
def test_mm_v2_unpadded_input_bitwise(shape, monkeypatch):
    T, NB, H, W, C, F, pad = shape
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    x, w, b, dy = _mk(*shape, seed=sum(shape))
    ext = ops.hip_ext()
    wp = ext.tconv_repack_v2(w, False)
    wpd = ext.tconv_repack_v2(w, True)
    y0, y1 = _both(monkeypatch, "MAML355_CONV_V2_NOPAD",
                   lambda: ext.tconv_mm_v2(x, wp, b, pad, Ho, Wo, F, False)[0])
    assert y1.shape == (T, NB, Ho, Wo, F)
    assert torch.equal(y0, y1), "forward"
    assert y1.float().abs().sum().item() > 0
    dx0, dx1 = _both(
        monkeypatch, "MAML355_CONV_V2_NOPAD",
        lambda: ext.tconv_mm_v2(dy, wpd, None, 2 - pad, H, W, C, False)[0])
    assert dx1.shape == (T, NB, H, W, C)
    assert torch.equal(dx0, dx1), "dgrad"


def test_mm_v2_unpadded_input_double_buffer(monkeypatch):
    """The 80 KB double-buffered variant stages through the same code."""
    shape = (2, 3, 11, 9, 48, 48, 1)
    T, NB, H, W, C, F, pad = shape
    x, w, b, _ = _mk(*shape, seed=5)
    ext = ops.hip_ext()
    wp = ext.tconv_repack_v2(w, False)
    y_ref = ext.tconv_mm_v2(x, wp, b, pad, H, W, F, False)[0]

    def run():
        monkeypatch.setenv("MAML355_CONV_V2_SBUF", "0")
        return ext.tconv_mm_v2(x, wp, b, pad, H, W, F, False)[0]

    y0, y1 = _both(monkeypatch, "MAML355_CONV_V2_NOPAD", run)
    assert torch.equal(y0, y1) and torch.equal(y1, y_ref)


def test_mm_v2_unpadded_input_with_stats(monkeypatch):
    """with_stats=True: Y and the BN sums.  The sums are float atomics, whose
    order changes from run to run, so the inputs are random non-zero
    integers, x from {+-1}, w and bias from {+-1, +-2}: every y is an integer
    with |y| <= 72*2 + 2 = 146, and over the 294 positions of a task (two
    blocks) sum |y| <= 42924 and sum y^2 <= 294 * 146^2 = 6266904 < 2^24.
    Every partial sum is an integer below 2^24, hence exact in fp32 in any
    order, and ``torch.equal`` is a fair demand on both Y and sums."""
    T, NB, H, W, C, F, pad = 2, 6, 7, 7, 8, 8, 1
    g = torch.Generator().manual_seed(11)

    def pick(vals, *size):
        v = torch.tensor(vals)
        return v[torch.randint(0, len(vals), size, generator=g)]

    x = pick([-1.0, 1.0], T, NB, H, W, C).to(torch.bfloat16).to(dev())
    w = pick([-2.0, -1.0, 1.0, 2.0], T, F, C, 3, 3).to(dev())
    b = pick([-2.0, -1.0, 1.0, 2.0], T, F).to(dev())
    ext = ops.hip_ext()
    wp = ext.tconv_repack_v2(w, False)
    (y0, s0), (y1, s1) = _both(
        monkeypatch, "MAML355_CONV_V2_NOPAD",
        lambda: ext.tconv_mm_v2(x, wp, b, pad, H, W, F, True))
    assert s1.shape == (T, 2, F)
    assert torch.equal(y0, y1)
    assert torch.equal(s0, s1)
    # and they are the sums of what the kernel wrote, before its rounding
    y64 = torch.nn.functional.conv2d(
        x[0].cpu().double().permute(0, 3, 1, 2), w[0].cpu().double(),
        b[0].cpu().double(), padding=pad).permute(0, 2, 3, 1)
    assert torch.equal(s1[0, 0].cpu().double(), y64.sum(dim=(0, 1, 2)))
    assert torch.equal(s1[0, 1].cpu().double(), (y64 * y64).sum(dim=(0, 1, 2)))


DCONV_SHAPES = [
    (2, 5, 14, 14, 1, 64, 1),
    (2, 5, 14, 14, 3, 48, 1),
    (2, 3, 7, 5, 3, 16, 1),
    (2, 3, 9, 11, 1, 32, 0),
    (1, 1, 1, 1, 3, 48, 1),
    (2, 2, 3, 3, 3, 48, 0),
    (2, 3, 7, 7, 8, 16, 1),       # C = 8 keeps the vector-unit kernel
    (1, 3, 20, 19, 3, 48, 1),     # more positions than one block's tiles
    # the matrix-unit kernel tiles the flat position index by 16: 15, 16, 17
    (1, 1, 3, 5, 3, 48, 1),
    (1, 1, 4, 4, 3, 48, 1),
    (1, 1, 1, 17, 1, 64, 1),
    # many small images: a wave's stride from tile to tile spans whole images
    (1, 200, 3, 3, 3, 16, 1),
]


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", DCONV_SHAPES, ids=_id)
def test_dconv_fwd_v2_bitwise(shape, with_bias, monkeypatch):
    T, NB, H, W, C, F, pad = shape
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    x, w, b, _ = _mk(*shape, seed=sum(shape) + 1)
    ext = ops.hip_ext()
    y0, y1 = _both(monkeypatch, "MAML355_DCONV_FWD_V2",
                   lambda: ext.dconv_fwd(x, w, b if with_bias else None, pad,
                                         Ho, Wo))
    assert y1.shape == (T, NB, Ho, Wo, F) and y1.dtype == torch.bfloat16
    assert torch.equal(y0, y1)
    assert y1.float().abs().sum().item() > 0
