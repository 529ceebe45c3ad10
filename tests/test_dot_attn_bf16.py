"""The inputs, the reference and the bounds of the bf16 dot-product attention tests
(tests/test_dot_attn_bf16_gpu.py imports them), and the one condition that keeps those bounds
sharp, checked with the reference alone (no GPU). Inputs: ``test_dot_attn.case`` with q, k, v, g
rounded to bf16 and widened exactly, at score scales 0.5 and 40 over
``test_gat_kernels.pattern()``. Reference: ``test_dot_attn.dot_attn_contract`` in fp64 (the
oracle) and in fp32 (whose error sets ``b = test_gat_kernels.bound``).
"""
from __future__ import annotations

import functools

import pytest
import torch

from test_dot_attn import case, dot_attn_contract
from test_gat_bf16 import EPS
from test_gat_kernels import N, PAIRS, R, bound, pattern

SCALES = [0.5, 40.0]
BF16_OUT = ("out", "dq", "dk", "dv")


def inputs(C, heads, s):
    d = case(C, heads, s)
    return {n: d[n].bfloat16().float() for n in ("q", "k", "v", "g")} | {"scale": d["scale"]}


def evaluate(C, heads, s, rowptr, col, dtype):
    """Every array the three kernels write; dk, dv over all N sources (one source or two)."""
    d = inputs(C, heads, s)
    return dot_attn_contract(rowptr, col, d["q"], d["k"], d["v"], None, None, N, d["g"], heads,
                             d["scale"], 0.0, None, dtype=dtype)


@functools.lru_cache(maxsize=None)
def reference(C, heads, s, dtype):
    rowptr, col, _ = pattern()
    return evaluate(C, heads, s, rowptr, col, dtype)


def bounds(name, ref64, ref32):
    """(b, elementwise bound): fp32 outputs ``b``; bf16 outputs ``b + 2^-8 (|ref64| + b)``."""
    b = bound(ref64, ref32)
    return b, (b + EPS * (ref64.abs() + b) if name in BF16_OUT else torch.full_like(ref64, b))


@pytest.mark.parametrize("C,heads", PAIRS)
def test_one_wrong_edge_exceeds_the_bounds(C, heads):
    """With a row's last entry dropped, or gathered from the source half way round the source
    list, the bf16 ``out`` of that row moves by at least 20 times its bound and the fp32 ``c``
    by at least 5 times its bound, at every row length around a lane-group width and in the
    hub. No other row moves."""
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
        ratio = {k: ((wrong[k] - r64[k]).abs() / bounds(k, r64[k], r32[k])[1]).amax(1)
                 for k in ("out", "c")}
        assert (ratio["out"][picked] >= 20).all(), ratio["out"][picked]
        assert (ratio["c"][picked] >= 5).all(), ratio["c"][picked]
        for k, t in ratio.items():
            assert (t[hit == 0] == 0).all(), k
