"""The kernels that close every training step — the bf16 linear head
(linear.hip), softmax-CE (softmax_ce.hip), the LSLR update (lslr.hip) and
fused Adam (adam.hip) — against the exact-input float64 oracle, at the
shapes where each takes another path: tails below one wave, the caps, second
blocks and second grid-stride trips.

Cases, inputs, oracle calls and bounds live in ``_head_cases.py`` and
``_oracle.py``; ``test_oracle.py`` applies the same checks to the fp32
reference on the CPU first.  No element is excluded from any comparison.
Measured err/bound figures: KERNEL_TEST_MAP_HEAD.md.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

import _head_cases as hc
import _oracle as orc
from howtotrainyourmamlpytorch_amd import ops
from howtotrainyourmamlpytorch_amd.ops import reference as ref


def dev():
    assert ops.hip_ext() is not None, "these tests are about the HIP kernels"
    return torch.device("cuda", 0)


# ---------------------------------------------------------------------------
# bf16 linear trio
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", hc.LINEAR_SHAPES, ids=hc._id)
def test_linear_bf16_first_order_within_bound(shape):
    """y, dx: (n + 2) 2^-24 sum|a||b| + 2^-8 |ref|; dw, db: the first term,
    fp32; n the reduction length (K + 1 with the bias, ways, M, M)."""
    hc.check_linear_first_order(ops.task_linear, shape, dev())


@pytest.mark.parametrize("shape", hc.LINEAR_SHAPES, ids=hc._id)
def test_linear_bf16_exact_on_small_integers(shape):
    """x, dy, b in {-3..3}, w in quarter units in {-0.75..0.75}: every
    partial sum is an exact fp32 value, so y and dx equal the oracle rounded
    to bf16 and dw, db equal it as fp32.  From K = 4096 on (the K = 8200
    shape) the ranges shrink to {-2..2} and {-0.5..0.5}: partial sums stay
    below 8200 * 2 * 0.5 + 2 = 8202, in quarter units far below 2^24."""
    hc.check_linear_exact(ops.task_linear, shape, dev())


@pytest.mark.parametrize("shape", hc.LINEAR_SECOND_ORDER_SHAPES, ids=hc._id)
def test_linear_bf16_second_order(shape):
    """The scenarios and figures of test_wconv_second_order on the bf16
    head, against ops.reference on widened inputs."""
    x, w, b, _ = hc.linear_inputs(shape + (True,))
    got = hc.linear_second_order(ops.task_linear, x, w, b, dev())
    want = hc.linear_second_order(ref.task_linear, x.float(), w, b, hc.CPU)
    for name, a, r in zip(("inner dw", "inner db", "through-dx dx", "through-dx dw"),
                          got, want):
        atol = 5e-2 * max(r.abs().max().item(), 1e-3)
        orc._report(name, (a - r).abs().double(), (atol + 8e-2 * r.abs()).double())
        torch.testing.assert_close(a, r, rtol=8e-2, atol=atol)


# ---------------------------------------------------------------------------
# softmax-CE
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", hc.CE_CASES, ids=hc._id)
def test_ce_within_bound(case):
    """loss, dlogits, and both outputs of the double backward; fp32 and bf16
    logits, int32 labels, every label on the last lane, and the five input
    families (bounds: orc.ce_loss_bound, orc.ce_prob_bound)."""
    hc.check_ce(ops.softmax_cross_entropy, case, dev())


def test_ce_refuses_more_than_64_ways():
    logits = torch.zeros(2, 3, 65, device=dev())
    labels = torch.zeros(2, 3, dtype=torch.long, device=dev())
    with pytest.raises(RuntimeError, match="ways must be <= 64"):
        ops.softmax_cross_entropy(logits, labels)


# ---------------------------------------------------------------------------
# LSLR
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("create_graph", [False, True], ids=["kernel_bwd", "create_graph"])
@pytest.mark.parametrize("shape", hc.LSLR_SHAPES, ids=hc._id)
def test_lslr_within_bound(shape, create_graph):
    """out within 2^-24 |ref| (one fma); da bitwise the upstream grad; dgrad
    within 2^-24 |ref| from lslr_bwd_kernel (grad mode off) and twice that
    from the create_graph composition; dlr within (T + 1) 2^-24 sum|g grad|."""
    hc.check_lslr(ops.lslr_update, shape, dev(), create_graph)


def test_lslr_second_order_through_create_graph_branch():
    hc.check_lslr_second_order(ops.lslr_update, dev())


# ---------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", hc.ADAM_CASES, ids=hc._id)
def test_adam_within_bound(case):
    """p, m, v of one fused step against orc.adam_bounds, which documents
    the three bounds; prints e_bc, the fp32 bias-correction term."""
    hc.check_adam(ops.fused_adam_step, case, dev())


def test_adam_takes_32_tensors_and_refuses_33():
    mk = lambda n: [torch.ones(1, device=dev()) for _ in range(n)]  # noqa: E731
    with pytest.raises(RuntimeError, match="1..32 tensors"):
        ops.fused_adam_step(mk(33), mk(33), mk(33), mk(33), step=1, lr=hc.LR)
    ps = mk(32)
    ops.fused_adam_step(ps, mk(32), mk(32), mk(32), step=1, lr=hc.LR)
    assert all(p.item() != 1.0 for p in ps)


@pytest.mark.parametrize("clamp,decay", [(None, 0.0), (1.5, hc.DECAY)],
                         ids=["plain", "clamp-decay"])
def test_fused_adam_optimizer_step_by_step(clamp, decay):
    hc.check_fused_adam_optimizer(dev(), clamp, decay)
