"""The inputs, the reference and the bounds of the bf16 GATv2 attention tests
(tests/test_gatv2_bf16_gpu.py imports them), and the conditions that keep those bounds sharp,
checked with the reference alone (no GPU). Inputs: ``test_gatv2.case`` with l, r, g rounded to
bf16 and widened exactly (a stays fp32), at score scales 0.5 and 40 over
``test_gat_kernels.pattern()``. Reference: ``test_gatv2.gatv2_contract`` with its own ``c`` and
``beta = 0``, in fp64 (the oracle) and in fp32 (whose error sets ``b = test_gat_kernels.bound``).
"""
from __future__ import annotations

import functools

import pytest
import torch

from test_gat_bf16 import EPS
from test_gat_kernels import N, PAIRS, R, bound, pattern
from test_gatv2 import SCALES, SLOPE, case, gatv2_contract  # noqa: F401

BF16_OUT = ("out", "dl", "dr")


def inputs(C, heads, s):
    d = case(C, heads, s)
    return {n: d[n].bfloat16().float() for n in ("l", "r", "g")} | {"a": d["a"]}


def evaluate(C, heads, s, rowptr, col, dtype):
    """Every array the three kernels write; dr over all N sources (one source or two)."""
    d = inputs(C, heads, s)
    return gatv2_contract(rowptr, col, d["l"], d["r"], None, N, d["a"], d["g"], heads, SLOPE,
                          0.0, None, c=None, dtype=dtype)


@functools.lru_cache(maxsize=None)
def reference(C, heads, s, dtype):
    rowptr, col, _ = pattern()
    return evaluate(C, heads, s, rowptr, col, dtype)


def bounds(name, ref64, ref32):
    """(b, elementwise bound): fp32 outputs ``b``; bf16 outputs ``b + 2^-8 (|ref64| + b)``."""
    b = bound(ref64, ref32)
    return b, (b + EPS * (ref64.abs() + b) if name in BF16_OUT else torch.full_like(ref64, b))


@pytest.mark.parametrize("C,heads", PAIRS)
def test_input_conditions(C, heads):
    """fp64 and fp32 take the same LeakyReLU branch on every (edge, channel) — ``pre`` is one
    correctly rounded add of the same values — and sums of bf16 values do hit ``pre == 0``, where
    ``lam = slope``; every edge carries weight at scale 0.5 and scale 40 overflows an
    unsubtracted fp32 ``exp``."""
    for s in SCALES:
        r64, r32 = (reference(C, heads, s, t) for t in (torch.float64, torch.float32))
        assert torch.equal(r64["pre"] > 0, r32["pre"] > 0)
        assert int((r64["pre"] == 0).sum()) >= 1
    assert float(reference(C, heads, 0.5, torch.float64)["alpha"].min()) >= 1e-4
    assert float(reference(C, heads, 40.0, torch.float64)["e"].max()) > 89.0


@pytest.mark.parametrize("C,heads", PAIRS)
def test_one_wrong_edge_exceeds_the_bounds(C, heads):
    """With a row's last entry dropped, or gathered from the source half way round the source
    list, the bf16 ``out`` of that row moves by at least 20 times its bound (the factor
    test_dot_attn_bf16.py asserts for its ``out``; the smallest the reference gives here over the
    twelve pairs and both edits is 24.9), at every row length around a lane-group width and in
    the hub. No other row moves."""
    rowptr, col, _ = pattern()
    r64, r32 = (reference(C, heads, 0.5, t) for t in (torch.float64, torch.float32))
    deg = rowptr.diff()
    picked = [int((deg == n).nonzero()[0]) for n in (2, 9, 17, 33, 65, 130, 301)]
    last = rowptr[1:][picked] - 1
    keep = torch.ones(col.numel(), dtype=torch.bool)
    keep[last] = False
    hit = torch.zeros(R, dtype=torch.long)
    hit[picked] = 1
    moved = col.clone()
    moved[last] = (moved[last] + N // 2) % N
    dropped = rowptr - torch.cat([torch.zeros(1, dtype=torch.long), hit.cumsum(0)])
    for rp, cl in ((dropped, col[keep]), (rowptr, moved)):
        wrong = evaluate(C, heads, 0.5, rp, cl, torch.float64)
        ratio = ((wrong["out"] - r64["out"]).abs() / bounds("out", r64["out"], r32["out"])[1]
                 ).amax(1)
        assert (ratio[picked] >= 20).all(), ratio[picked]
        assert (ratio[hit == 0] == 0).all()
