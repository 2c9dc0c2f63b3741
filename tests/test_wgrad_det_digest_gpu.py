"""Deterministic wgrad results are pinned by digest.

Under MAML355_DETERMINISTIC=1 every wgrad entry point sums private K-chunk
slices in a fixed order, so its ``dw`` and ``db`` are a pure function of the
inputs and of the split-K plan (ops/hip/wgrad_plan.h).  The SHA-256 of their
bytes is compared with tests/golden/wgrad_det_digests.json, recorded once on
an MI355X from the commit *before* the plan moved into that header: a digest
that differs means a launcher now cuts other K-chunks or sums them in another
order.  The fixture is never re-recorded from the code under test.

Inputs come from a seeded CPU generator, so they are the same bytes on every
machine.  The plans themselves are checked on the CPU by
tests/test_wgrad_plan.py."""

import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from howtotrainyourmamlpytorch_amd import ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "wgrad_det_digests.json")

_ENV = ("MAML355_WGRAD_NSUB", "MAML355_DETERMINISTIC", "MAML355_WGRAD_V2",
        "MAML355_WGRAD_V3", "MAML355_DCONV_WGRAD")

# (T, NB, H, W, C, F, pad)
_TCONV_SHAPES = [
    (2, 3, 11, 9, 48, 48, 1),     # odd, non-square, ragged K
    (1, 1, 3, 3, 8, 8, 0),        # one position, one slice
    (4, 75, 21, 21, 48, 48, 1),   # 33 075 positions: v3 takes v2's chunks
    (2, 8, 64, 64, 16, 24, 1),    # 8-aligned C = 16, F = 24
]

# (entry point, stride, fp32 inputs, shape, MAML355_WGRAD_NSUB or None)
CASES = [(fn, 1, False, s, None)
         for fn in ("tconv_wgrad", "tconv_wgrad_v2", "tconv_wgrad_v3")
         for s in _TCONV_SHAPES]
CASES += [
    ("tconv_wgrad_v3", 1, False, (2, 5, 84, 84, 3, 48, 1), None),  # first layer
    ("tconv_wgrad_v3", 1, False, (4, 75, 21, 21, 48, 48, 1), 2),
    ("sconv_wgrad", 2, False, (2, 3, 11, 9, 48, 48, 1), None),
    ("dconv_wgrad", 1, False, (2, 5, 12, 12, 3, 48, 1), None),
    ("fconv_wgrad", 1, True, (2, 3, 11, 9, 48, 48, 1), None),
]


def case_id(case):
    fn, _, _, shape, nsub = case
    return fn + "-" + "x".join(map(str, shape)) + ("-nsub%d" % nsub if nsub else "")


def case_env(case):
    """The MAML355_* settings a case runs under; everything else unset."""
    env = {"MAML355_DETERMINISTIC": "1"}
    if case[4] is not None:
        env["MAML355_WGRAD_NSUB"] = str(case[4])
    return env


def _mk(case):
    _, stride, fp32, (T, NB, H, W, C, F, pad), _ = case
    g = torch.Generator().manual_seed(sum((T, NB, H, W, C, F, pad)))
    Ho = (H + 2 * pad - 3) // stride + 1
    Wo = (W + 2 * pad - 3) // stride + 1
    x = torch.randn(T, NB, H, W, C, generator=g)
    dy = torch.randn(T, NB, Ho, Wo, F, generator=g)
    if not fp32:
        x, dy = x.to(torch.bfloat16), dy.to(torch.bfloat16)
    return x, dy


def _sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def digests(case):
    """{"dw": sha256, "db": sha256} of one case; the MAML355_* environment is
    the caller's business (case_env)."""
    x, dy = _mk(case)
    T, NB, H, W, C, F, pad = case[3]
    d = torch.device("cuda", 0)
    dw, db = getattr(ops.hip_ext(), case[0])(dy.to(d), x.to(d), pad, True)
    torch.cuda.synchronize()
    assert dw.shape == (T, F, C, 3, 3) and dw.dtype == torch.float32
    assert db.shape == (T, F) and db.dtype == torch.float32
    assert dw.abs().sum().item() > 0 and db.abs().sum().item() > 0
    return {"dw": _sha(dw), "db": _sha(db)}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_wgrad_deterministic_digest(case, monkeypatch):
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in case_env(case).items():
        monkeypatch.setenv(k, v)
    with open(GOLDEN) as f:
        want = json.load(f)[case_id(case)]
    assert digests(case) == want
