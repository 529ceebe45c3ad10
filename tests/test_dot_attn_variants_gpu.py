"""The variants of the fused dot-product attention kernels (csrc/kernels/dot_attn_f32.h: one
template per kernel, the variants' statements under ``if constexpr``) pinned to one another
where a variant's extra operand is neutral: dropout at ``p = 0`` and edge features that are
all zero must give the plain kernels' results.

Pattern and inputs: see tests/test_dot_attn.py (37 rows over 41 local + 19 halo sources with
rows of degree 0, 1, LPR +- 1 and a 301-entry hub), score scale 0.5, int32 columns, two
sources. ``c`` is the fp64 oracle's, rounded to fp32, the same for both sides of a comparison.
These are exact comparisons (``torch.equal``; -0 and +0 compare equal):

* ``p = 0``: ``thr = 0`` keeps every edge and ``inv_keep = 1``; the extra multiply by 1.0f is
  exact in both the plain and the fused form.
* ``ee = 0``: ``k_j + 0`` and ``v_j + 0`` are ``k_j`` and ``v_j``. The edge source side sums the
  weights the destination side stored where the plain one recomputes them, in the same order.
"""
from __future__ import annotations

import pytest
import torch

import test_dot_attn_drop_gpu as drop_gpu
import test_dot_attn_edge_gpu as edge_gpu
import test_dot_attn_gpu as plain_gpu
from test_dot_attn import case, oracle
from test_dot_attn_edge import E

pytestmark = pytest.mark.gpu
SHAPES = [(64, 1), (128, 4), (256, 8)]
S = 0.5


@pytest.fixture(scope="module", autouse=True)
def _native():
    from dgraph_amd import _native

    assert _native.load(), "native library missing"


def _plain(C, heads):
    d, c64 = case(C, heads, S), oracle(C, heads, S, 0.0)[0]["c"]
    return d, c64, plain_gpu._Buffers(d, c64, torch.int32, True, 0.0).run()


def _assert_equal(tag, got, want, names):
    for name in names:
        same = torch.equal(got[name], want[name])
        ne = got[name] != want[name]
        diff = float((got[name][ne].double() - want[name][ne].double()).abs().max()) if ne.any() \
            else 0.0
        print(f"{tag} {name}: equal {same}, max |difference| {diff:.3e}")
        assert same, (tag, name, diff)


@pytest.mark.parametrize("C,heads", SHAPES)
def test_drop_at_p0_is_the_plain_kernels(C, heads):
    """``dot_attn_drop_*_f32`` with ``p = 0`` against ``dot_attn_*_f32`` with ``beta = 0``."""
    d, c64, want = _plain(C, heads)
    got = drop_gpu._Buffers(d, c64, torch.int32, True, 0.0).run()
    _assert_equal(f"drop p=0 C={C} heads={heads}", got, want,
                  ("out", "stat_m", "stat_l", "dq", "dk", "dv"))


@pytest.mark.parametrize("C,heads", SHAPES)
def test_edge_with_zero_rows_is_the_plain_kernels(C, heads):
    """``dot_attn_edge_*_f32`` with ``ee = 0`` against ``dot_attn_*_f32`` with ``beta = 0``."""
    d, c64, want = _plain(C, heads)
    got = edge_gpu._Buffers(d, torch.zeros(E, C), c64, torch.int32, True, 0.0).run()
    _assert_equal(f"edge ee=0 C={C} heads={heads}", got, want,
                  ("out", "stat_m", "stat_l", "dq", "dk", "dv"))
