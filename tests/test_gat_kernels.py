"""The contract of the fused graph-attention kernels (csrc/kernels/gat_f32.hip) written out
per edge in plain PyTorch, and the test pattern the GPU tests run them on
(tests/test_gat_kernels_gpu.py imports both from here).

:func:`gat_contract` takes exactly what the three kernels take — the CSR pattern, the two
gathered sources, the source / destination scores as independent inputs, dL/dout, the
attention vector, ``beta`` and ``out`` on entry — and returns every array they write. It
shares no code with ``ops/gat.py::_reference``. Run in fp64 it is the oracle; run in fp32 it
gives the error a faithful fp32 evaluation of the same formula has, from which the GPU
tests derive their bound (:func:`bound`).

The tests of this file run without a GPU and pin the oracle down first:

* against ``torch.autograd.grad`` of a row-by-row ``torch.softmax`` forward (gradients with
  respect to ``sd``, ``ss`` and ``x``), and the ``a_src`` term against the gradient of
  ``ops.gat._reference`` with respect to ``z``;
* the pattern has the degrees and in-degrees the kernels can go wrong at, every edge
  carries at least ``2e-4`` of its row's weight at the small score scale, and the large
  score scale overflows ``exp`` in fp32 unless the row maximum is subtracted.
"""
from __future__ import annotations

import functools

import pytest
import torch
import torch.nn.functional as F

SLOPE = 0.2
R, LS, HS = 37, 41, 19  # destination rows, local sources, halo sources
N = LS + HS
# every LPR (16 / 32 / 64 lanes per row) boundary +-1, a hub of several chunks at every LPR
# next to an empty row and two short rows (rows 16..19 share a wave at 4 rows per wave)
DEGREES = [0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130, 0, 3, 301, 2, 0, 5]
PAIRS = [(C, h) for C in (64, 128, 256) for h in (1, 2, 4, 8)]
SCALES = [0.5, 30.0]
OUTPUTS = ("out", "stat_m", "stat_l", "c", "gsd", "gss", "gz")


def row_degrees(nrows: int = R) -> torch.Tensor:
    return torch.tensor([DEGREES[i % len(DEGREES)] for i in range(nrows)])


@functools.lru_cache(maxsize=None)
def pattern():
    """(rowptr [R+1], col [E] int64 over [local | halo], rows [E]). Columns: a cubic skew of
    a uniform draw, every other draw mirrored, over all but two sources of each part (those
    two keep in-degree 0); a draw lands in the halo part with probability 1/3."""
    gen = torch.Generator().manual_seed(20)
    deg = row_degrees()
    rowptr = torch.zeros(R + 1, dtype=torch.long)
    rowptr[1:] = torch.cumsum(deg, 0)
    E = int(rowptr[-1])
    u = torch.rand(E, generator=gen) ** 3
    halo = torch.rand(E, generator=gen) < 1.0 / 3.0
    col = torch.empty(E, dtype=torch.long)
    for part, first, n, dead in ((~halo, 0, LS, (5, 23)), (halo, LS, HS, (2, 11))):
        alive = torch.tensor([j for j in range(n) if j not in dead])
        k = (u[part] * alive.numel()).long().clamp_(max=alive.numel() - 1)
        k[1::2] = alive.numel() - 1 - k[1::2]
        col[part] = first + alive[k]
    rows = torch.repeat_interleave(torch.arange(R), deg)
    return rowptr, col, rows


def transpose(rowptr: torch.Tensor, col: torch.Tensor, ncols: int):
    """Source rows -> destination ids (each source's destinations in ascending order)."""
    rows = torch.repeat_interleave(torch.arange(rowptr.numel() - 1), rowptr[1:] - rowptr[:-1])
    order = torch.sort(col.long(), stable=True).indices
    t_rowptr = torch.zeros(ncols + 1, dtype=torch.long)
    t_rowptr[1:] = torch.cumsum(torch.bincount(col.long(), minlength=ncols), 0)
    return t_rowptr, rows[order]


@functools.lru_cache(maxsize=None)
def case(C: int, heads: int, s: float):
    """The kernels' inputs for one (C, heads, score scale), fp32 values on the CPU:
    x over all N sources (the tests split it at LS), independent scores, dL/dout, the
    attention vector and ``out`` on entry."""
    gen = torch.Generator().manual_seed(1000 * C + 10 * heads + int(s))
    rn = lambda *shape: torch.randn(*shape, generator=gen)  # noqa: E731
    return dict(C=C, heads=heads, x=rn(N, C), ss=rn(N, heads) * s, sd=rn(R, heads) * s,
                g=rn(R, C), a_src=rn(C) * 0.3, out0=rn(R, C))


def gat_contract(rowptr, col, x, x2, nsplit, ss, ss2, sd, g, a_src, slope, beta, out,
                 dtype=torch.float64):
    """What gat_fwd / gat_bwd_dst / gat_bwd_src compute, per edge, in ``dtype``.

    ``x`` / ``ss`` serve columns below ``nsplit`` (all of them without ``x2``), ``x2`` /
    ``ss2`` the columns from ``nsplit`` on. Returns out, stat_m, stat_l, c, gsd over the
    destination rows and gss, gz over all source rows (``[x rows | x2 rows]``), plus the
    per-edge ``alpha`` and pre-activation scores ``e``."""
    cv = lambda t: t.detach().cpu().to(dtype)  # noqa: E731
    rowptr, col = rowptr.cpu().long(), col.cpu().long()
    if x2 is not None:
        xa, sa = torch.cat([cv(x)[:nsplit], cv(x2)]), torch.cat([cv(ss)[:nsplit], cv(ss2)])
    else:
        xa, sa = cv(x), cv(ss)
    sd, g, a_src = cv(sd), cv(g), cv(a_src)
    nr, ns, C, Hh = rowptr.numel() - 1, xa.shape[0], xa.shape[1], sa.shape[1]
    D = C // Hh
    rows = torch.repeat_interleave(torch.arange(nr), rowptr[1:] - rowptr[:-1])
    E = rows.numel()
    pre = sd[rows] + sa[col]                                            # [E, Hh]
    lam = torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, slope))
    e = torch.where(pre > 0, pre, pre * slope)
    m = torch.full((nr, Hh), -float("inf"), dtype=dtype).index_reduce(
        0, rows, e, "amax", include_self=True)
    p = torch.exp(e - m[rows])
    den = torch.zeros(nr, Hh, dtype=dtype).index_add(0, rows, p)
    inv = torch.where(den > 0, 1.0 / den, torch.zeros_like(den))
    alpha = p * inv[rows]
    xe = xa[col].view(E, Hh, D)
    ge = g[rows].view(E, Hh, D)
    agg = torch.zeros(nr, C, dtype=dtype).index_add(
        0, rows, (alpha.unsqueeze(-1) * xe).reshape(E, C))
    res = {"out": agg if beta == 0 else beta * cv(out) + agg, "stat_m": m, "stat_l": inv}
    ga = (ge * xe).sum(-1)                                              # [E, Hh]
    c = torch.zeros(nr, Hh, dtype=dtype).index_add(0, rows, alpha * ga)
    A = torch.zeros(nr, Hh, dtype=dtype).index_add(0, rows, lam * alpha * ga)
    B = torch.zeros(nr, Hh, dtype=dtype).index_add(0, rows, lam * alpha)
    res["c"], res["gsd"] = c, A - c * B
    gss = torch.zeros(ns, Hh, dtype=dtype).index_add(0, col, lam * alpha * (ga - c[rows]))
    gz = torch.zeros(ns, C, dtype=dtype).index_add(
        0, col, (alpha.unsqueeze(-1) * ge).reshape(E, C))
    res["gss"] = gss
    res["gz"] = gz + (gss.unsqueeze(-1) * a_src.view(Hh, D)).reshape(ns, C)
    res["alpha"], res["e"] = alpha, e
    return res


def bound(ref64: torch.Tensor, ref32: torch.Tensor) -> float:
    """The largest |kernel - fp64| allowed: ``max(2e-5, 8 err32) scale`` with
    ``scale = max(1, max|fp64|)`` and ``err32 = max|fp32 - fp64| / scale`` of the same
    formula evaluated in fp32 on the CPU. 2e-5 is the project's figure for this op and for
    the fp32 SpMM; the factor 8 covers ``__expf`` (``2^(x log2 e)``: the rounding of its
    argument costs about |x| 2^-24 relative, up to ~17 half-ulps for the terms that reach
    fp32 at all) and the kernels' different, fixed summation order."""
    ref64 = ref64.double()
    scale = max(1.0, float(ref64.abs().max())) if ref64.numel() else 1.0
    err32 = float((ref32.double() - ref64).abs().max()) / scale if ref64.numel() else 0.0
    return max(2e-5, 8.0 * err32) * scale


@functools.lru_cache(maxsize=None)
def oracle(C: int, heads: int, s: float, beta: float):
    """(fp64 result, fp32 result) of :func:`gat_contract` on ``case(C, heads, s)``."""
    rowptr, col, _ = pattern()
    d = case(C, heads, s)
    args = (rowptr, col, d["x"], None, N, d["ss"], None, d["sd"], d["g"], d["a_src"], SLOPE,
            beta, d["out0"])
    return gat_contract(*args), gat_contract(*args, dtype=torch.float32)


def edge_softmax_contract(rowptr, s, g, dtype=torch.float64):
    """Softmax of ``s`` [E, H] over each CSR row per head, and its adjoint applied to
    ``g``: ``ds = alpha (g - sum_row alpha g)``."""
    rowptr, s, g = rowptr.cpu().long(), s.detach().cpu().to(dtype), g.detach().cpu().to(dtype)
    nr, Hh = rowptr.numel() - 1, s.shape[1]
    rows = torch.repeat_interleave(torch.arange(nr), rowptr[1:] - rowptr[:-1])
    m = torch.full((nr, Hh), -float("inf"), dtype=dtype).index_reduce(
        0, rows, s, "amax", include_self=True)
    p = torch.exp(s - m[rows])
    alpha = p / torch.zeros(nr, Hh, dtype=dtype).index_add(0, rows, p)[rows]
    dot = torch.zeros(nr, Hh, dtype=dtype).index_add(0, rows, alpha * g)
    return alpha, alpha * (g - dot[rows])


# ------------------------------------------------------------------------------- the tests
def test_pattern_conditions():
    rowptr, col, rows = pattern()
    deg = rowptr[1:] - rowptr[:-1]
    assert rowptr.numel() == R + 1 and torch.equal(deg, row_degrees())
    assert 1250 <= col.numel() <= 1350
    assert int(col.min()) >= 0 and int(col.max()) < N
    # a partial last row group at 4 and 2 rows per wave, for destinations and both sources
    for n in (R, LS, HS):
        assert n % 4 and n % 2
    # every lane-group width: deg in {LPR - 1, LPR, LPR + 1} and several chunks
    for lpr in (16, 32, 64):
        for d in (lpr - 1, lpr, lpr + 1):
            assert (deg == d).any()
        assert int(deg.max()) > 4 * lpr
    # the hub shares its wave (4 rows per wave) with an empty row and two short rows
    hub = int(deg.argmax())
    mates = deg[hub // 4 * 4: hub // 4 * 4 + 4]
    assert (mates == 0).any() and ((mates > 0) & (mates < 8)).sum() >= 2
    assert (deg == 0).sum() >= 3 and (deg == 1).any()
    indeg = torch.bincount(col, minlength=N)
    for part in (indeg[:LS], indeg[LS:]):
        assert (part == 0).any()
        assert ((part >= 1) & (part <= 15)).any()
        assert (part > 64).any()
    t_rowptr, t_col = transpose(rowptr, col, N)
    assert torch.equal(t_rowptr[1:] - t_rowptr[:-1], indeg)
    src = torch.repeat_interleave(torch.arange(N), indeg)
    assert torch.equal(torch.sort(src * R + t_col).values, torch.sort(col * R + rows).values)


@pytest.mark.parametrize("C,heads", PAIRS)
def test_score_scale_conditions(C, heads):
    # s = 0.5: every edge carries weight — one dropped, doubled or misattributed edge moves
    # an output by at least ten times the 2e-5 tolerance
    small, _ = oracle(C, heads, 0.5, 0.0)
    assert float(small["alpha"].min()) >= 2e-4
    # s = 30: exp overflows in fp32 (e^89 > FLT_MAX) unless the row maximum is subtracted
    big, big32 = oracle(C, heads, 30.0, 0.0)
    assert float(big["e"].max()) > 89.0
    assert not torch.isfinite(torch.exp(big["e"].max().float()))
    rowptr = pattern()[0]
    full = rowptr[1:] > rowptr[:-1]  # (an empty row's maximum is -inf)
    for k in OUTPUTS:
        for t in (big[k], big32[k]):
            assert torch.isfinite(t[full] if k == "stat_m" else t).all(), k


@pytest.mark.parametrize("C,heads", PAIRS)
def test_one_wrong_edge_exceeds_the_bound(C, heads):
    """What the alpha condition is for: with the last entry of a row dropped, or gathered
    from another source, that row of ``out`` moves by at least ten times the bound the GPU
    tests allow — at every row length around a lane-group width and in the hub."""
    rowptr, col, rows = pattern()
    d = case(C, heads, 0.5)
    r64, r32 = oracle(C, heads, 0.5, 0.0)
    bd = bound(r64["out"], r32["out"])
    deg = rowptr[1:] - rowptr[:-1]
    picked = [int((deg == n).nonzero()[0]) for n in (2, 9, 17, 33, 65, 130, 301)]
    last = rowptr[1:][picked] - 1
    keep = torch.ones(col.numel(), dtype=torch.bool)
    keep[last] = False
    hit = torch.zeros(R, dtype=torch.long)
    hit[picked] = 1
    moved = col.clone()
    moved[last] = (moved[last] + 7) % N
    for rp, cl in ((rowptr - torch.cat([torch.zeros(1, dtype=torch.long), hit.cumsum(0)]),
                    col[keep]), (rowptr, moved)):
        wrong = gat_contract(rp, cl, d["x"], None, N, d["ss"], None, d["sd"], d["g"],
                             d["a_src"], SLOPE, 0.0, None)
        diff = (wrong["out"] - r64["out"]).abs().amax(1)
        assert (diff[picked] >= 10 * bd).all(), (diff[picked], bd)
        assert (diff[hit == 0] <= 1e-12).all()


def _rowwise_forward(rowptr, col, x, ss, sd, heads):
    """out_i = sum_j softmax_j(leaky_relu(sd_i + ss_j)) x_j per head, row by row."""
    C = x.shape[1]
    outs = []
    for i in range(rowptr.numel() - 1):
        j = col[rowptr[i]:rowptr[i + 1]]
        a = torch.softmax(F.leaky_relu(sd[i] + ss[j], SLOPE), 0)           # [deg, heads]
        outs.append(torch.einsum("ek,ekd->kd", a, x[j].view(-1, heads, C // heads)).reshape(C))
    return torch.stack(outs)


@pytest.mark.parametrize("two_sources", [False, True])
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("C,heads", [(64, 1), (64, 8), (128, 4), (256, 2)])
def test_contract_matches_autograd(C, heads, s, two_sources):
    rowptr, col, _ = pattern()
    d = case(C, heads, s)
    x, ss, sd = (d[k].double().requires_grad_() for k in ("x", "ss", "sd"))
    g = d["g"].double()
    out = _rowwise_forward(rowptr, col, x, ss, sd, heads)
    gx, gss, gsd = torch.autograd.grad(out, (x, ss, sd), g)
    zero = torch.zeros(C)
    if two_sources:
        ref = gat_contract(rowptr, col, d["x"][:LS], d["x"][LS:], LS, d["ss"][:LS],
                           d["ss"][LS:], d["sd"], g, zero, SLOPE, 0.5, d["out0"])
    else:
        ref = gat_contract(rowptr, col, d["x"], None, N, d["ss"], None, d["sd"], g, zero,
                           SLOPE, 0.5, d["out0"])
    tol = dict(atol=1e-10, rtol=1e-10)
    torch.testing.assert_close(ref["out"], 0.5 * d["out0"].double() + out.detach(), **tol)
    torch.testing.assert_close(ref["gsd"], gsd, **tol)
    torch.testing.assert_close(ref["gss"], gss, **tol)
    torch.testing.assert_close(ref["gz"], gx, **tol)
    deg = rowptr[1:] - rowptr[:-1]
    assert (ref["stat_l"][deg == 0] == 0).all() and (ref["stat_l"][deg > 0] > 0).all()
    assert (ref["stat_l"][deg == 1] == 1).all()


@pytest.mark.parametrize("C,heads", [(64, 2), (128, 8), (256, 1)])
def test_contract_a_src_term_matches_op_reference(C, heads):
    """ss = z . a_src: gz carries gss (x) a_src — against autograd through ops/gat.py's
    own oracle with respect to z and the halo rows; also its transposed pattern."""
    import dgraph_amd.ops.gat as G

    rowptr, col, _ = pattern()
    d = case(C, heads, 0.5)
    pat = G.GatPattern(rowptr, col, LS, HS)
    z = d["x"][:LS].double().requires_grad_()
    zh = d["x"][LS:].double().requires_grad_()
    a = d["a_src"].double().view(heads, C // heads)
    sd, g = d["sd"].double(), d["g"].double()
    out = G._reference(z, zh, sd, a, pat)
    gz, gzh = torch.autograd.grad(out, (z, zh), g)
    ss = G.head_scores(torch.cat([z, zh]).detach(), a)
    ref = gat_contract(rowptr, col, z, zh, LS, ss[:LS], ss[LS:], sd, g, a.reshape(-1), SLOPE,
                       0.0, None)
    tol = dict(atol=1e-10, rtol=1e-10)
    torch.testing.assert_close(ref["out"], out.detach(), **tol)
    torch.testing.assert_close(ref["gz"], torch.cat([gz, gzh]), **tol)
    t_rowptr, t_col = transpose(rowptr, col, N)
    assert torch.equal(pat.t_rowptr, t_rowptr)
    src = torch.repeat_interleave(torch.arange(N), t_rowptr[1:] - t_rowptr[:-1])
    assert torch.equal(torch.sort(src * R + pat.t_col.long()).values,
                       torch.sort(src * R + t_col).values)


def test_edge_softmax_contract_matches_autograd():
    rowptr = torch.zeros(R + 1, dtype=torch.long)
    rowptr[1:] = torch.cumsum(row_degrees(), 0)
    gen = torch.Generator().manual_seed(5)
    s = (torch.randn(int(rowptr[-1]), 3, generator=gen, dtype=torch.float64) * 5).requires_grad_()
    g = torch.randn(s.shape, generator=gen, dtype=torch.float64)
    a = torch.cat([torch.softmax(s[rowptr[i]:rowptr[i + 1]], 0) for i in range(R)])
    (ds,) = torch.autograd.grad(a, s, g)
    alpha, dref = edge_softmax_contract(rowptr, s, g)
    torch.testing.assert_close(alpha, a.detach(), atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(dref, ds, atol=1e-12, rtol=1e-12)
