"""CPU check of the float64 oracle (tests/_oracle.py) that the GPU kernel
tests compare against: it must agree with ``ops.reference`` in fp32, and the
discrete-decision exclusions it computes must stay below the share the GPU
tests allow."""

import pytest
import torch

import _oracle as orc
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
