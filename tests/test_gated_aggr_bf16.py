"""The inputs, the reference and the bounds of the bf16 gated aggregation tests
(tests/test_gated_aggr_bf16_gpu.py imports them), and the condition that keeps those bounds
sharp, checked with the reference alone. Inputs: ``test_pna.values`` rounded to bf16 and widened
exactly, over ``test_pna.skewed_csr``. Reference: ``test_gated_aggr``'s contracts in fp64 (the
oracle) and in fp32 on the CPU (whose error sets ``b = test_gat_kernels.bound``).
"""
import functools

import pytest
import torch

from test_gat_bf16 import EPS
from test_gat_kernels import bound
from test_gated_aggr import gated_bwd_contract, gated_contract
from test_pna import skewed_csr, values

ROWS, COLS = 300, 257


def rounded(n, F, seed, shift=0.0):
    return (values("plain", n, F, seed) + shift).bfloat16().float()


@functools.lru_cache(maxsize=None)
def inputs(F, shift=0.0):
    """``(k, q, v, g)`` as fp32 tensors holding bf16 values; ``k`` shifted by ``shift``."""
    return (rounded(ROWS, F, 3 * F, shift), rounded(COLS, F, 3 * F + 1),
            rounded(COLS, F, 3 * F + 2), rounded(ROWS, F, 1000 + F))


@functools.lru_cache(maxsize=None)
def reference(F, shift, dtype):
    """out, ds over the skewed pattern and dq, dv over its transpose."""
    csr, (k, q, v, g) = skewed_csr(), inputs(F, shift)
    out, ds = gated_contract(csr.rowptr, csr.col, k, q, v, dtype=dtype)
    tc = csr.transpose()
    dq, dv = gated_bwd_contract(tc.rowptr, tc.col, k, q, v, g, dtype=dtype)
    return dict(out=out, ds=ds, dq=dq, dv=dv)


def bounds(ref64, ref32, eps=EPS):
    """(b, ``b + eps (|ref64| + b)``): ``eps`` = 2^-8 for one bf16 rounding, 0 for fp32."""
    b = bound(ref64, ref32)
    return b, b + eps * (ref64.double().abs() + b)


@pytest.mark.parametrize("F", [8, 64])
def test_one_wrong_edge_exceeds_the_bounds(F):
    """With a row's last entry dropped, or gathered from the source half way round the list,
    the bf16 ``out`` of that row moves by at least 4 times its bound, at degree 1, 2 and around
    one and two lane-group widths; no other row moves. Smallest ratio: 24.7 (F = 8), 88.9."""
    csr, (k, q, v, _) = skewed_csr(), inputs(F)
    rowptr, col = csr.rowptr, csr.col.long()
    r64, r32 = (reference(F, 0.0, t)["out"] for t in (torch.float64, torch.float32))
    bd = bounds(r64, r32)[1]
    deg = rowptr.diff()
    picked = [int((deg == n).nonzero()[0]) for n in (1, 2, 7, 8, 9, 15, 16, 17)
              if bool((deg == n).any())]
    assert len(picked) >= 6 and 1 in picked and 2 in picked
    last = rowptr[1:][picked] - 1
    keep = torch.ones(col.numel(), dtype=torch.bool).index_fill(0, last, False)
    hit = torch.zeros(ROWS, dtype=torch.long)
    hit[picked] = 1
    moved = col.clone()
    moved[last] = (moved[last] + COLS // 2) % COLS
    dropped = rowptr - torch.cat([torch.zeros(1, dtype=torch.long), hit.cumsum(0)])
    for rp, cl in ((dropped, col[keep]), (rowptr, moved)):
        wrong = gated_contract(rp, cl, k, q, v)[0]
        ratio = ((wrong - r64).abs() / bd).amax(1)
        assert (ratio[picked] >= 4).all(), ratio[picked]
        assert (ratio[hit == 0] == 0).all()
