"""2x2 max-pool (pool.hip) in fp32 and bf16, on the vector (C % 8 == 0) and
scalar paths, with exact ties, and past the grid cap of the vector
backward.  The op only moves values, so every comparison with the float64
oracle (first maximum wins, window order (0,0), (0,1), (1,0), (1,1)) is
exact."""

import pytest
import torch

pytestmark = pytest.mark.gpu

import _oracle as orc
from howtotrainyourmamlpytorch_amd import ops


def dev():
    return torch.device("cuda", 0)


def _check_all_orders(x, seed):
    """fwd, bwd (scatter) and double-backward (gather) — all exact."""
    T, NS, H, W, C = x.shape
    g = torch.Generator().manual_seed(seed)
    gy = torch.randn(T, NS, H // 2, W // 2, C, generator=g).to(x.dtype)
    r = torch.randn(T, NS, H, W, C, generator=g).to(x.dtype)

    xg = x.to(dev()).requires_grad_(True)
    gg = gy.to(dev()).requires_grad_(True)
    y = ops.task_maxpool2x2(xg)
    (dx,) = torch.autograd.grad(y, xg, gg, create_graph=True)
    # linear in dx, so d(dy) is r gathered at the argmax: values only move
    (ddy,) = torch.autograd.grad((dx * r.to(dev())).sum(), gg)

    xo = orc.widen(x).requires_grad_(True)
    go = orc.widen(gy).requires_grad_(True)
    yo, arg = orc.pool2x2(xo)
    (dxo,) = torch.autograd.grad(yo, xo, go, create_graph=True)
    (ddyo,) = torch.autograd.grad((dxo * orc.widen(r)).sum(), go)

    assert y.dtype == x.dtype and dx.dtype == x.dtype and ddy.dtype == x.dtype
    assert y.shape == yo.shape and dx.shape == x.shape
    assert (y.detach().cpu().double() == yo.detach()).all().item(), "y"
    assert (dx.detach().cpu().double() == dxo.detach()).all().item(), "dx"
    assert (ddy.cpu().double() == ddyo).all().item(), "d(dy)"
    return arg


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [48, 5])
def test_maxpool_all_orders_exact(C, dtype):
    g = torch.Generator().manual_seed(30 + C)
    x = torch.randn(2, 4, 7, 9, C, generator=g).to(dtype)
    _check_all_orders(x, seed=31)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [48, 5])
def test_maxpool_ties_first_maximum_wins(C, dtype):
    """Inputs from {-2, ..., 2}: over a third of the windows tie at their
    maximum, and the tie decides where the gradient goes."""
    g = torch.Generator().manual_seed(32 + C)
    x = torch.randint(-2, 3, (2, 4, 7, 9, C), generator=g).to(dtype)
    win = orc.windows(orc.widen(x))
    top = win.topk(2, dim=-1).values
    assert orc.share(top[..., 0] == top[..., 1]) > 0.3
    arg = _check_all_orders(x, seed=33)
    # every tie position occurs: the routing is not trivially index 0
    assert set(arg.flatten().tolist()) == {0, 1, 2, 3}


def test_maxpool_bwd_vec_second_grid_stride_trip():
    """N*H*W*C/8 = 1 052 676 > 4096 x 256: maxpool_bwd_vec_kernel strides
    once more.  bf16, exact."""
    T, NS, H, W, C = 1, 4, 513, 513, 8
    assert T * NS * H * W * (C // 8) > 4096 * 256
    g = torch.Generator().manual_seed(34)
    x = torch.randn(T, NS, H, W, C, generator=g).to(torch.bfloat16)
    gy = torch.randn(T, NS, H // 2, W // 2, C, generator=g).to(torch.bfloat16)
    xg = x.to(dev()).requires_grad_(True)
    y = ops.task_maxpool2x2(xg)
    (dx,) = torch.autograd.grad(y, xg, gy.to(dev()))
    xo = orc.widen(x).requires_grad_(True)
    yo, _ = orc.pool2x2(xo)
    (dxo,) = torch.autograd.grad(yo, xo, orc.widen(gy))
    assert (y.detach().cpu().double() == yo.detach()).all().item()
    assert (dx.cpu().double() == dxo).all().item()
    assert (dx[:, :, H - 1] == 0).all().item() and (dx[:, :, :, W - 1] == 0).all().item()
