"""The gradient of ``ParamArena.views()`` through ``arena_scatter`` (one
launch, ``MAML355_ARENA_SCATTER=1``) against autograd's own slice backward (``=0``)
in the same process: ``torch.equal`` at first and second order.

The kernel only moves values, so every element is the view gradient's own
bits or +0.0; autograd's sum gives the same except for the sign of a zero,
which ``torch.equal`` does not see.  Specs: numels (5, 1, 16, 7, 3), so
offsets 0, 5, 6, 22, 29 with P = 32 (one interior of whole 16-byte groups,
the rest misaligned), and a single parameter of 9 elements, whose rows
start misaligned from the second task on.  ``test_flagship_offsets`` calls
the kernel itself with an odd P, segments longer than one block's pass and
an absent entry."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from howtotrainyourmamlpytorch_amd import ops
from howtotrainyourmamlpytorch_amd.models.arena import ParamArena

ENV = "MAML355_ARENA_SCATTER"

SPECS = {
    "five": [("a", (5,)), ("b", (1,)), ("c", (4, 2, 2)), ("d", (7, 1)),
             ("e", (3,))],
    "single": [("w", (3, 3))],
}
COEF = (1.5, -2.0, 0.75, 3.0, -0.5)


def dev():
    return torch.device("cuda", 0)


def _arena(pa, T, seed=0):
    g = torch.Generator().manual_seed(seed)
    theta = torch.randn(pa.numel, generator=g).to(dev()).requires_grad_(True)
    # as the engine makes it: theta broadcast over the tasks, scaled per
    # task so the rows differ
    scale = torch.arange(1, T + 1, device=dev(), dtype=torch.float32)
    return theta, theta.unsqueeze(0) * scale.unsqueeze(1)


def _loss(views, use, noncontig):
    total = 0.0
    for i, (name, v) in enumerate(views.items()):
        if i not in use:
            continue
        if noncontig and v.dim() >= 3:
            # the view's gradient arrives as a transposed tensor
            total = total + (v.transpose(1, -1).contiguous() ** 2).sum() * COEF[i]
        else:
            total = total + (v ** 2).sum() * COEF[i]
    return total


def _grads(pa, T, use, noncontig, second_order):
    theta, arena = _arena(pa, T)
    views = pa.views(arena)
    loss = _loss(views, use, noncontig)
    g1, = torch.autograd.grad(loss, arena, create_graph=second_order)
    if not second_order:
        return [g1.detach()]
    # a fast-weight step, then a second differentiated use of the views
    arena2 = arena - 0.1 * g1
    loss2 = _loss(pa.views(arena2), use, False) + (g1 ** 2).sum()
    g2, = torch.autograd.grad(loss2, theta)
    return [g1.detach(), g2.detach()]


def _count_scatter(monkeypatch):
    calls = []
    ext = ops.hip_ext()
    real = ext.arena_scatter

    def counted(*a):
        calls.append(1)
        return real(*a)
    monkeypatch.setattr(ext, "arena_scatter", counted)
    return calls


CASES = {
    "all_views": (None, False, False),
    "some_views": ({0, 2}, False, False),
    "noncontiguous": (None, True, False),
    "second_order": (None, False, True),
    "second_order_some": ({0, 2}, False, True),
}


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("spec", list(SPECS))
@pytest.mark.parametrize("case", list(CASES))
def test_bits_equal_slice_path(monkeypatch, case, spec, T):
    pa = ParamArena(SPECS[spec])
    use, noncontig, second = CASES[case]
    n = len(pa.specs)
    use = set(range(n)) if use is None else {i for i in use if i < n}
    calls = _count_scatter(monkeypatch)
    monkeypatch.setenv(ENV, "0")
    want = _grads(pa, T, use, noncontig, second)
    assert not calls
    monkeypatch.setenv(ENV, "1")
    got = _grads(pa, T, use, noncontig, second)
    assert calls, "arena_scatter did not run"
    for a, b in zip(want, got):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert a.abs().max().item() > 0
        assert torch.equal(a, b), \
            f"max|delta|={(a.double() - b.double()).abs().max().item():.3e}"


def test_flagship_offsets():
    """Offsets that are not multiples of 4 with a P that is odd, so rows
    start at every alignment: the kernel called directly against the
    slice-assign it replaces, with an absent entry."""
    numels = (7, 3, 1030, 5, 260, 2)
    pa = ParamArena([(f"p{i}", (n,)) for i, n in enumerate(numels)])
    T = 5
    g = torch.Generator().manual_seed(3)
    grads = [torch.randn(T, n, generator=g).to(dev()) for n in numels]
    slots = [0, 1, 2, 4, 5]          # p3 absent
    out = ops.hip_ext().arena_scatter(
        [grads[i] for i in slots], slots, [s.offset for s in pa.specs],
        [s.numel for s in pa.specs], T, pa.numel)
    want = torch.zeros(T, pa.numel, device=dev())
    for i in slots:
        s = pa.specs[i]
        want[:, s.offset:s.offset + s.numel] = grads[i]
    assert torch.equal(out, want)
    # absent ranges are +0.0
    s = pa.specs[3]
    assert (out[:, s.offset:s.offset + s.numel].view(torch.int32) == 0).all()


@pytest.mark.parametrize("spec", list(SPECS))
def test_views_share_storage(monkeypatch, spec):
    monkeypatch.setenv(ENV, "1")
    pa = ParamArena(SPECS[spec])
    arena = torch.randn(3, pa.numel, device=dev(), requires_grad=True)
    views = pa.views(arena)
    for s in pa.specs:
        v = views[s.name]
        assert v.shape == (3,) + s.shape
        assert v.requires_grad
        assert v.untyped_storage().data_ptr() == arena.untyped_storage().data_ptr()
        assert v.data_ptr() == arena.data_ptr() + 4 * s.offset
        assert torch.equal(v.detach().reshape(3, -1),
                           arena.detach()[:, s.offset:s.offset + s.numel])
