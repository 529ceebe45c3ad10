"""The inputs and the reference of the bf16 relation-attention tests
(tests/test_gat_bf16_gpu.py imports both), and the one condition on the drawn inputs that
makes those tests sharp, checked with the reference alone (no GPU).

Reference: ``ops/gat.py::_reference`` under autograd on the bf16-rounded inputs widened
exactly, in fp64 (the oracle) and in fp32 (whose error sets the bound,
``test_gat_kernels.bound``).
"""
from __future__ import annotations

import functools

import pytest
import torch

from test_gat_kernels import HS, LS, N, PAIRS, R, SLOPE, bound, case, pattern

BF16_OUT = ("out", "gz", "gzh")
EPS = 2.0 ** -8  # one round-to-nearest-even at bf16's 7 stored mantissa bits


def inputs(C, heads, s):
    """bf16-rounded z / g / into (as fp32 values), fp32 sd and a_src scaled so that the source
    scores <z, a_src> reach the scale ``s``. sd is drawn at half that scale: sd_i + ss_j then
    changes sign inside most rows, and dL/dsd (identically 0 over a row whose entries all lie
    on one side of the leaky ReLU) carries every edge."""
    d = case(C, heads, s)
    rb = lambda t: t.bfloat16().float()  # noqa: E731
    a = d["a_src"].view(heads, C // heads) / 0.3 * s / (C // heads) ** 0.5
    return dict(z=rb(d["x"]), g=rb(d["g"]), into=rb(d["out0"]), sd=d["sd"] * 0.5, a=a)


def evaluate(d, rowptr, col, two, dtype):
    """out, the gradients and the forward's statistics over the pattern (rowptr, col)."""
    import dgraph_amd.ops.gat as G

    heads = d["a"].shape[0]
    ns, nh = (LS, HS) if two else (N, 0)
    pat = G.GatPattern(rowptr, col, ns, nh)
    rows = torch.repeat_interleave(torch.arange(R), rowptr.diff())
    mk = lambda t: t.to(dtype).requires_grad_()  # noqa: E731
    z, sd, a = mk(d["z"][:ns]), mk(d["sd"]), mk(d["a"])
    zh = mk(d["z"][ns:]) if two else None
    out = d["into"].to(dtype) + G._reference(z, zh, sd, a, pat)
    ins = [t for t in (z, zh, sd, a) if t is not None]
    names = [n for n, t in zip(("gz", "gzh", "gsd", "ga"), (z, zh, sd, a)) if t is not None]
    res = dict(zip(names, torch.autograd.grad(out, ins, d["g"].to(dtype))), out=out.detach())
    # the statistics the forward leaves: row maximum and 1 / sum per head
    ss = G.head_scores(d["z"].to(dtype), a.detach())
    e = torch.nn.functional.leaky_relu(sd.detach()[rows] + ss[col], SLOPE)
    m = torch.full((R, heads), -float("inf"), dtype=dtype).index_reduce(0, rows, e, "amax")
    den = torch.zeros(R, heads, dtype=dtype).index_add(0, rows, torch.exp(e - m[rows]))
    res["stat_m"] = m
    res["stat_l"] = torch.where(den > 0, 1 / den, torch.zeros_like(den))
    return res


@functools.lru_cache(maxsize=None)
def reference(C, heads, s, two, dtype):
    rowptr, col, _ = pattern()
    return evaluate(inputs(C, heads, s), rowptr, col, two, dtype)


def bounds(name, ref64, ref32):
    """(b, elementwise bound): fp32 outputs ``b``; bf16 outputs ``b + 2^-8 (|ref64| + b)``."""
    b = bound(ref64, ref32)
    return b, (b + EPS * (ref64.abs() + b) if name in BF16_OUT else torch.full_like(ref64, b))


@pytest.mark.parametrize("C,heads", PAIRS)
def test_one_wrong_edge_exceeds_the_bounds(C, heads):
    """With a row's last entry dropped, or gathered from another source (the one half way
    round the source list), the fp32 outputs of that row (stat_l and gsd, the larger of the
    two: 1 / sum of a hub moves by 1e-5, dL/dsd of a short one-sided row by nothing) move by
    at least ten times their bound, and the bf16 ``out`` by at least four times its bound on
    the rows of degree <= 65 (one edge of a hub carries about 2e-4 of the row, below 2^-8:
    the hubs are covered by the fp32 outputs). No other row moves."""
    rowptr, col, _ = pattern()
    d = inputs(C, heads, 0.5)
    r64, r32 = (reference(C, heads, 0.5, False, t) for t in (torch.float64, torch.float32))
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
        wrong = evaluate(d, rp, cl, False, torch.float64)
        ratio = {k: ((wrong[k] - r64[k]).abs() / bounds(k, r64[k], r32[k])[1]).amax(1)
                 for k in ("stat_l", "gsd", "out")}
        f32 = torch.maximum(ratio["stat_l"], ratio["gsd"])
        assert (f32[picked] >= 10).all(), f32[picked]
        short = [r for r in picked if deg[r] <= 65]
        assert (ratio["out"][short] >= 4).all(), ratio["out"][short]
        for k, t in ratio.items():
            assert (t[hit == 0] == 0).all(), k
