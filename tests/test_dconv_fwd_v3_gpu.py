"""The LDS-staged first-layer forward (``dconv_fwd_v3_kernel``, the default
for C in {1, 3} in launches of 2^22 output positions and more, and at every
size with MAML355_DCONV_FWD_V3=1, which these tests set) against
``dconv_fwd_v2_kernel`` (MAML355_DCONV_FWD_V3=0).

Both run the same fp32 chain ``acc = bias; acc = fmaf(x, w, acc)`` over
(ky, kx, c) on the fp32 matrix unit; only the way x arrives differs (rows of
the zero-padded image staged in LDS against predicated per-lane loads), and a
zero from the LDS halo is the same MFMA operand as a predicated zero.  So the
results are compared with ``torch.equal`` AND as raw 16-bit patterns: even
the signs of zeros agree.

A chunk is R output lines: R = 4 at W = 84, C = 3 (eight staged rows of
86 x 3 elements fill the 2304-element LDS buffer), and for a small launch
about 336 positions otherwise (R = 12 at W = 28).  The launcher gives a small
shape one chunk per block, so the cases that need a block to walk several
chunks, the last one ragged, cap the blocks per task with
MAML355_DCONV_FWD_V3_BLOCKS=1.  The address logic itself is walked on the CPU
by tests/test_dconv_fwd_v3_addr.py."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from howtotrainyourmamlpytorch_amd import ops
from howtotrainyourmamlpytorch_amd.config import get_args
from howtotrainyourmamlpytorch_amd.meta.engine import MAMLFewShotClassifier

_ENV = ("MAML355_DCONV_FWD_V2", "MAML355_DCONV_FWD_V3",
        "MAML355_DCONV_FWD_V3_BLOCKS", "MAML355_DETERMINISTIC")


def dev():
    return torch.device("cuda", 0)


def _id(s):
    return "x".join(map(str, s))


def _mk(T, NB, H, W, C, F, pad, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, NB, H, W, C, generator=g).to(torch.bfloat16)
    w = torch.randn(T, F, C, 3, 3, generator=g).mul(0.1)
    b = torch.randn(T, F, generator=g)
    assert (x != 0).all() and (w != 0).all()
    return x.to(dev()), w.to(dev()), b.to(dev())


def _v2_then_v3(monkeypatch, fn, blocks=None):
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MAML355_DCONV_FWD_V3", "0")
    old = fn()
    monkeypatch.setenv("MAML355_DCONV_FWD_V3", "1")
    if blocks is not None:
        monkeypatch.setenv("MAML355_DCONV_FWD_V3_BLOCKS", str(blocks))
    new = fn()
    torch.cuda.synchronize()
    return old, new


def _same_bits(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype == torch.bfloat16
    assert torch.isfinite(a.float()).all().item()
    assert torch.equal(a, b)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), \
        "equal values, different bit patterns (sign of a zero)"


# (T, NB, H, W, C, F, pad)
SHAPES = [
    (1, 1, 1, 1, 3, 48, 1),       # one position
    (1, 1, 3, 5, 3, 48, 1),       # 15 positions: less than a tile
    (1, 1, 1, 17, 1, 64, 1),      # one row, 17 positions
    (2, 3, 7, 5, 3, 16, 1),       # W below the tile width
    (2, 3, 9, 11, 1, 32, 0),      # pad 0
    (2, 2, 3, 3, 3, 48, 0),       # one output position per image
    (1, 200, 3, 3, 3, 16, 1),     # a chunk of 91 lines spans 30 images
    (2, 5, 14, 14, 1, 64, 1),
    (2, 5, 14, 14, 3, 48, 1),
    (3, 2, 20, 84, 3, 48, 1),     # mini-imagenet's row width, 10 chunks
    (2, 2, 28, 28, 1, 64, 1),     # omniglot's row width
    (1, 1, 1, 254, 3, 16, 1),     # widest row that fits: R = 1, 3 staged rows
    (1, 2, 5, 300, 3, 16, 1),     # too wide for the LDS buffer: v2 runs
] + [(2, 3, 7, 7, C, F, 1) for F in (16, 32, 48, 64) for C in (1, 3)]

# several chunks per block (MAML355_DCONV_FWD_V3_BLOCKS=1), ragged last chunk,
# an image boundary inside a chunk; one per instantiation family
MULTI = [
    (1, 2, 7, 84, 3, 48, 1),      # R = 4: 14 lines = 4 + 4 + 4 + 2
    (2, 2, 7, 84, 3, 16, 0),      # R = 4: 10 lines = 4 + 4 + 2, pad 0
    (1, 2, 20, 28, 1, 64, 1),     # R = 12: 40 lines = 12 + 12 + 12 + 4
    (2, 7, 9, 9, 1, 32, 1),       # R = 38: 63 lines = 38 + 25
    (1, 40, 5, 5, 3, 64, 1),      # R = 68: 200 lines = 68 + 68 + 64
]


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_v3_bitwise(shape, with_bias, monkeypatch):
    T, NB, H, W, C, F, pad = shape
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    x, w, b = _mk(*shape, seed=sum(shape))
    ext = ops.hip_ext()
    old, new = _v2_then_v3(
        monkeypatch,
        lambda: ext.dconv_fwd(x, w, b if with_bias else None, pad, Ho, Wo))
    assert new.shape == (T, NB, Ho, Wo, F)
    _same_bits(old, new)


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("blocks", [1, 2])
@pytest.mark.parametrize("shape", MULTI, ids=_id)
def test_v3_many_chunks_per_block(shape, blocks, with_bias, monkeypatch):
    T, NB, H, W, C, F, pad = shape
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    x, w, b = _mk(*shape, seed=sum(shape) + 1)
    ext = ops.hip_ext()
    old, new = _v2_then_v3(
        monkeypatch,
        lambda: ext.dconv_fwd(x, w, b if with_bias else None, pad, Ho, Wo),
        blocks=blocks)
    _same_bits(old, new)


def test_v3_default_at_launch_size(monkeypatch):
    """No toggle set, 64 x 10 x 84 x 84 = 4.5M positions: the launcher's own
    choice (v3 from 2^22 positions up) against v2."""
    shape = (64, 10, 84, 84, 3, 16, 1)
    x, w, b = _mk(*shape, seed=5)
    ext = ops.hip_ext()
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    new = ext.dconv_fwd(x, w, b, 1, 84, 84)
    monkeypatch.setenv("MAML355_DCONV_FWD_V3", "0")
    old = ext.dconv_fwd(x, w, b, 1, 84, 84)
    torch.cuda.synchronize()
    _same_bits(old, new)


@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("shape", [(2, 3, 7, 84, 3, 48), (2, 3, 9, 11, 1, 64),
                                   (2, 4, 3, 3, 3, 16)], ids=_id)
def test_v3_reads_stay_inside_x(shape, pad, monkeypatch):
    """x is a slice from the middle of a NaN-filled buffer: a read before a
    task's first image or past the last task's last image shows as NaN."""
    T, NB, H, W, C, F = shape
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    x, w, b = _mk(T, NB, H, W, C, F, pad, seed=sum(shape) + pad)
    n = x.numel()
    big = torch.full((3 * n + 7,), float("nan"), dtype=torch.bfloat16,
                     device=dev())
    xin = big[n + 3:2 * n + 3]
    xin.copy_(x.reshape(-1))
    xin = xin.view(T, NB, H, W, C)
    assert xin.is_contiguous() and xin.data_ptr() != big.data_ptr()
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MAML355_DCONV_FWD_V3", "1")
    ext = ops.hip_ext()
    for blocks in (None, 1):
        if blocks is not None:
            monkeypatch.setenv("MAML355_DCONV_FWD_V3_BLOCKS", str(blocks))
        got = ext.dconv_fwd(xin, w, b, pad, Ho, Wo)
        want = ext.dconv_fwd(x, w, b, pad, Ho, Wo)
        torch.cuda.synchronize()
        _same_bits(want, got)
    assert torch.isnan(big[:n + 3].float()).all().item()
    assert torch.isnan(big[2 * n + 3:].float()).all().item()


IH, IW = 14, 15


def _two_iterations(filters):
    args = get_args([
        "--batch_size", "2", "--num_classes_per_set", "3",
        "--num_samples_per_class", "2", "--num_target_samples", "2",
        "--image_height", str(IH), "--image_width", str(IW),
        "--image_channels", "1",
        "--cnn_num_filters", str(filters), "--num_stages", "3",
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
    g = torch.Generator().manual_seed(9)
    theta = model.classifier.theta
    grad = loss = None
    for _ in range(2):
        xs = torch.randn(2, 3, 2, 1, IH, IW, generator=g)
        xt = torch.randn(2, 3, 2, 1, IH, IW, generator=g)
        ys = torch.arange(3).view(1, 3, 1).expand(2, 3, 2).contiguous()
        losses, _ = model.train_forward_prop((xs, xt, ys, ys.clone()), epoch=1)
        loss = losses["loss"]
        grad = torch.autograd.grad(loss, theta)[0]
        with torch.no_grad():
            theta.sub_(0.05 * grad)
    return loss.detach().clone(), grad.detach().clone()


def test_v3_model_bits(monkeypatch):
    """The 14x15 test model, two iterations, deterministic mode: loss and
    theta gradient with the staged kernel and with v2."""
    calls = []
    ext = ops.hip_ext()

    def counted(*a, _real=ext.dconv_fwd):
        calls.append(1)
        return _real(*a)
    monkeypatch.setattr(ext, "dconv_fwd", counted)
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MAML355_DETERMINISTIC", "1")
    monkeypatch.setenv("MAML355_DCONV_FWD_V3", "1")
    # The first model run of a process can differ from later identical runs
    # in the last bits of theta's gradient, whatever the toggles (profiles/
    # README.md, round 7): the runs compared here both come after one.
    _two_iterations(16)
    calls.clear()
    on = _two_iterations(16)
    assert calls, "the first layer did not run on dconv_fwd"
    monkeypatch.setenv("MAML355_DCONV_FWD_V3", "0")
    off = _two_iterations(16)
    for name, a, b in zip(("loss", "theta.grad"), on, off):
        assert torch.isfinite(a).all().item() and a.abs().max().item() > 0
        assert torch.equal(a, b), \
            f"{name}: max|delta|=" \
            f"{(a.double() - b.double()).abs().max().item():.3e}"
