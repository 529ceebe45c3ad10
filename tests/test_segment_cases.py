"""Inputs and references of tests/test_segment_variants_gpu.py, which runs the three
wave-per-row gather families (csrc/kernels/spmm_softmax.hip, spmm_pna.hip, spmm_max.hip) at
every (VEC, LPR) instantiation their launchers can pick, and the CPU tests that pin both down
first.

* :func:`ladder_csr`: 142 rows over 257 sources. Row ``d`` has degree ``d`` for d = 0..136
  (every boundary ``4 G k - 1, 4 G k, 4 G k + 1`` of the four-in-flight loop for G = 1, 2, 4,
  8 lane groups up to 128, and ``2 G k`` of the backward's two-in-flight loop), row 137 has
  1,027 = 32 * 32 + 3 entries, rows 138..141 (degree 5, 33, 64, 65) repeat ONE source each:
  every slot ties, the winner is slot 0.
* :func:`many_rows_csr`: square, N = 32,768 + 4,099 rows of degree ``r % 4``. The kernels'
  grid is capped at 8,192 workgroups of four waves, so 4,099 waves take a second row, in the
  forward (rows) and in the backward (sources of the transpose) alike.
* ``many_*``: the contracts of test_pna.py / test_softmax_aggr.py (one row at a time there)
  written one SLOT at a time over all rows at once, for the 36,867-row case. In fp32 the
  sums run left to right like :func:`test_pna._sum_rows`, so they equal the row-at-a-time
  contracts bitwise (shown here on the first 400 rows and sources).
* :data:`VARIANTS`: the widths ``F`` of the GPU tests with the instantiation each reaches,
  and :func:`select`, the launchers' rule restated, which shows that the table is complete.
* The ops' CPU path on the ladder meets the accuracy rule of the GPU tests
  (``test_gat_kernels.bound``), so those cannot fail on their own inputs. Largest
  ``error / bound`` of the CPU path over the fp32 widths (a record): softmax out 0.125,
  lse 0.013, dx 0.125, dt 0.025; PNA mean 0.037, sdev 0.033, dx 0.125; max / min dx 0.014
  (0.125: the CPU path then errs exactly like the fp32 contract, and the bound is 8 times
  that error).
"""
from __future__ import annotations

import functools
import math

import pytest
import torch

from dgraph_amd.ops import kernels as K
from dgraph_amd.ops.csr import CSR
from test_gat_kernels import bound
from test_pna import ALL, EPS, pna_bwd_contract, pna_contract, values
from test_softmax_aggr import softmax_bwd_contract, softmax_contract

NSRC = 257
HUB = 1027
SINGLE = (5, 33, 64, 65)  # degrees of the rows that repeat one source
LADDER_ROWS = 137 + 1 + len(SINGLE)
SINGLE_ROWS = tuple(range(138, LADDER_ROWS))
SPLIT = 130  # split_columns boundary of the two-source cases

WAVES = 256 * 32 * 4  # the grid cap of the three launchers, in waves (= rows per sweep)
MANY = WAVES + 4099


# ------------------------------------------------------------------------------ patterns
def with_idx(csr: CSR, idx_dtype) -> CSR:
    """The same pattern with column ids of ``idx_dtype`` (``transpose`` and
    ``split_columns`` pick int32 themselves, which would leave the int64 kernels unrun)."""
    return CSR(csr.rowptr, csr.col.to(idx_dtype).contiguous(), csr.num_cols)


@functools.lru_cache(maxsize=None)
def _ladder(seed):
    g = torch.Generator().manual_seed(seed)
    deg = torch.tensor(list(range(137)) + [HUB] + list(SINGLE))
    rowptr = torch.zeros(LADDER_ROWS + 1, dtype=torch.long)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, NSRC, (int(rowptr[-1]),), generator=g)
    for r in SINGLE_ROWS:
        col[int(rowptr[r]):int(rowptr[r + 1])] = col[int(rowptr[r])]
    return rowptr, col


def ladder_csr(idx_dtype=torch.int64, seed=0) -> CSR:
    rowptr, col = _ladder(seed)
    return CSR(rowptr, col.to(idx_dtype), NSRC)


@functools.lru_cache(maxsize=None)
def _many(seed):
    g = torch.Generator().manual_seed(seed)
    deg = torch.arange(MANY) % 4
    rowptr = torch.zeros(MANY + 1, dtype=torch.long)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, MANY, (int(rowptr[-1]),), generator=g)
    return rowptr, col


def many_rows_csr(idx_dtype=torch.int32, seed=0) -> CSR:
    rowptr, col = _many(seed)
    return CSR(rowptr, col.to(idx_dtype), MANY)


def transposed(csr: CSR, idx_dtype=None):
    """``(t, rel)`` of :meth:`CSR.transpose_rel` with ``t``'s column ids of ``idx_dtype``
    (default: the CSR's own)."""
    t, rel = CSR(csr.rowptr, csr.col, csr.num_cols).transpose_rel()
    return with_idx(t, idx_dtype or csr.col.dtype), rel


def second_pattern(seed=1) -> CSR:
    """A second block over the many-rows case: every odd row empty, even row ``r`` with
    ``1 + (r / 2) % 2`` entries."""
    g = torch.Generator().manual_seed(1000 + seed)
    r = torch.arange(MANY)
    deg = torch.where(r % 2 == 0, 1 + (r // 2) % 2, torch.zeros_like(r))
    rowptr = torch.zeros(MANY + 1, dtype=torch.long)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, MANY, (int(rowptr[-1]),), generator=g)
    return CSR(rowptr, col.to(torch.int32), MANY)


def union(a: CSR, b: CSR) -> CSR:
    """Row ``r``: the entries of ``a``'s row, then those of ``b``'s (the same sources)."""
    rows = torch.cat([a.row_ids(), b.row_ids()])
    cols = torch.cat([a.col.long(), b.col.long()])
    u = CSR.from_coo(rows, cols, a.num_rows, a.num_cols, index_dtype=torch.int64)
    return CSR(u.rowptr, u.col, a.num_cols)


def split_slots(full: CSR, arg: torch.Tensor, boundary: int = SPLIT) -> torch.Tensor:
    """What two passes over ``full.split_columns(boundary)`` record for the unsplit winner
    slots ``arg`` [R, F]: the offset within the first block's row, or ``-2 -`` the offset
    within the second's (-1 stays). Valid where no value ties across the two blocks."""
    first = (full.col.long() < boundary).long()
    before = torch.cumsum(first, 0) - first  # first-block entries ahead of each slot
    start = full.rowptr[:-1].unsqueeze(1)
    k = (start + arg.long().clamp(min=0)).clamp(max=max(full.nnz - 1, 0))
    n1 = before[k] - before[start.clamp(max=max(full.nnz - 1, 0))]
    res = torch.where(first[k] == 1, n1, -2 - (arg.long() - n1))
    return torch.where(arg < 0, arg.long(), res).to(torch.int32)


def temperature(kind, F):
    """tests/test_softmax_aggr_gpu.py's: ones, or both signs with one exact 0."""
    if kind == "one":
        return torch.ones(F)
    t = torch.linspace(-3.0, 3.0, F)
    t[F // 3] = 0.0
    return t


# ------------------------------------------------------------- contracts, a slot at a time
def _slots(rowptr):
    """``(k, idx [R], has [R, 1])`` for every slot number k below the largest degree."""
    deg = rowptr[1:] - rowptr[:-1]
    last = max(int(rowptr[-1]) - 1, 0)
    for k in range(int(deg.max()) if deg.numel() else 0):
        yield k, (rowptr[:-1] + k).clamp(max=last), (deg > k).unsqueeze(1)


def _lsum(rowptr, term, F, dtype):
    """sum_k term(k, idx) over each row's slots in slot order, absent slots adding +0."""
    acc = torch.zeros(rowptr.numel() - 1, F, dtype=dtype)
    zero = torch.zeros((), dtype=dtype)
    for k, idx, has in _slots(rowptr):
        acc = acc + torch.where(has, term(k, idx), zero)
    return acc


def many_softmax(rowptr, col, x, t, dtype=torch.float64):
    """:func:`test_softmax_aggr.softmax_contract` over all rows at once."""
    x, t = x.to(dtype), t.to(dtype)
    R, F = rowptr.numel() - 1, x.shape[1]
    col = col.long()
    ne = (rowptr[1:] > rowptr[:-1]).unsqueeze(1)
    m = torch.full((R, F), float("-inf"), dtype=dtype)
    for _, idx, has in _slots(rowptr):
        m = torch.where(has, torch.maximum(m, x[col[idx]] * t), m)
    ms = torch.where(ne, m, torch.zeros((), dtype=dtype))
    w = lambda idx: torch.exp(x[col[idx]] * t - ms)  # noqa: E731
    l = _lsum(rowptr, lambda k, idx: w(idx), F, dtype)
    a = _lsum(rowptr, lambda k, idx: w(idx) * x[col[idx]], F, dtype)
    one = torch.ones((), dtype=dtype)
    out = torch.where(ne, a / torch.where(ne, l, one), torch.zeros((), dtype=dtype))
    lse = torch.where(ne, ms + torch.log(torch.where(ne, l, one)),
                      torch.full((), float("-inf"), dtype=dtype))
    return out, lse


def many_softmax_bwd(t_rowptr, t_col, x, t, g, out_fwd, lse, dtype=torch.float64):
    """:func:`test_softmax_aggr.softmax_bwd_contract` over all sources at once; ``dt`` adds
    the sources' rows in source order (fp32: one at a time, as the contract does)."""
    x, t, g = x.to(dtype), t.to(dtype), g.to(dtype)
    of, lse = out_fwd.to(dtype), lse.to(dtype)
    F = x.shape[1]
    r = t_col.long()
    xs = x[:t_rowptr.numel() - 1]
    wg = lambda idx: torch.exp(t * xs - lse[r[idx]]) * g[r[idx]]  # noqa: E731
    d = lambda idx: xs - of[r[idx]]  # noqa: E731
    dx = _lsum(t_rowptr, lambda k, idx: wg(idx) * (1 + t * d(idx)), F, dtype)
    rows = _lsum(t_rowptr, lambda k, idx: wg(idx) * d(idx) * d(idx), F, dtype)
    if dtype != torch.float32:
        return dx, rows.sum(0)
    dt = torch.zeros(F, dtype=dtype)
    for row in rows.unbind(0):
        dt = dt + row
    return dx, dt


def many_pna(rowptr, col, x, eps=EPS, dtype=torch.float64):
    """:func:`test_pna.pna_contract` over all rows at once."""
    x = x.to(dtype)
    R, F = rowptr.numel() - 1, x.shape[1]
    col = col.long()
    deg = (rowptr[1:] - rowptr[:-1]).unsqueeze(1)
    ne = deg > 0
    n = deg.clamp(min=1).to(dtype)
    zero = torch.zeros((), dtype=dtype)
    mean = torch.where(ne, _lsum(rowptr, lambda k, idx: x[col[idx]], F, dtype) / n, zero)
    q = _lsum(rowptr, lambda k, idx: (x[col[idx]] - mean) ** 2, F, dtype)
    std = torch.where(ne, (q.clamp(min=0) / n + eps).sqrt(),
                      torch.full((1, F), eps, dtype=dtype).sqrt())
    res = dict(mean=mean, std=std)
    for name, better in (("max", torch.gt), ("min", torch.lt)):
        best = torch.zeros(R, F, dtype=dtype)
        slot = torch.full((R, F), -1, dtype=torch.int32)
        for k, idx, has in _slots(rowptr):
            v = x[col[idx]]
            win = has & ((slot < 0) | better(v, best))  # strict: the first slot keeps a tie
            best = torch.where(win, v, best)
            slot = torch.where(win, torch.full((), k, dtype=torch.int32), slot)
        res[name], res["a" + name] = best, slot
    return res


def many_pna_bwd(t_rowptr, t_col, rel, x, inv_deg, fwd, g, dtype=torch.float64):
    """:func:`test_pna.pna_bwd_contract` (first source) over all sources at once."""
    x = x.to(dtype)
    F = x.shape[1]
    r = t_col.long()
    xs = x[:t_rowptr.numel() - 1]
    inv = inv_deg.to(dtype)
    cv = {k: v.to(dtype) for k, v in g.items()}
    fm, fs = fwd["mean"].to(dtype), fwd["std"].to(dtype)

    def term(k, idx):
        rr = r[idx]
        b = torch.zeros(xs.shape[0], F, dtype=dtype)
        if "mean" in cv:
            b = b + cv["mean"][rr]
        if "std" in cv:
            b = b + cv["std"][rr] * (xs - fm[rr]) / fs[rr]
        tt = inv[rr].unsqueeze(1) * b
        for name in ("max", "min"):
            if name in cv:
                tt = tt + cv[name][rr] * (fwd["a" + name][rr].long() == rel[idx].long()
                                          .unsqueeze(1))
        return tt

    return _lsum(t_rowptr, term, F, dtype)


# ------------------------------------------------------------------------------ the table
# F -> (VEC, LPR, column passes), derived from launch_fwd / launch_bwd of the three files
VARIANTS = {
    "fp32": {7: (1, 8, 1), 13: (1, 16, 1), 29: (1, 32, 1), 50: (1, 64, 1), 150: (1, 64, 3),
             8: (4, 8, 1), 48: (4, 16, 1), 128: (4, 32, 1), 172: (4, 64, 1), 256: (4, 64, 1),
             600: (4, 64, 3)},
    # segment max / min alone takes bf16, with kMaxVec = 16 / sizeof(bf16) = 8
    "bf16": {16: (8, 8, 1), 96: (8, 16, 1), 200: (8, 32, 1), 344: (8, 64, 1), 1024: (8, 64, 2),
             12: (4, 8, 1), 52: (4, 16, 1), 100: (4, 32, 1), 172: (4, 64, 1), 300: (4, 64, 2),
             7: (1, 8, 1), 13: (1, 16, 1), 29: (1, 32, 1), 50: (1, 64, 1), 150: (1, 64, 3)},
}
FP32_F = tuple(VARIANTS["fp32"])
BF16_F = tuple(VARIANTS["bf16"])
MANY_F = (12, 70)  # VEC 4 LPR 8, and VEC 1 LPR 64 over two passes (64, 6)


def select(F: int, elem_bytes: int):
    """``(VEC, LPR, column passes)`` of a contiguous, aligned ``[*, F]`` operand.

    This mirrors by hand the rule of launch_fwd_vec / launch_fwd in spmm_max.hip and of
    the ``v4 ? 4 : 1`` dispatch in spmm_softmax.hip and spmm_pna.hip, and must be updated
    with them: VEC is the widest of {16 / elem_bytes, 4, 1} that divides F, then LPR is the
    first of 8, 16, 32, 64 that holds ``lanes = ceil(F / VEC)``. It checks that
    :data:`VARIANTS` is complete, not what a kernel selected."""
    vec = next(v for v in (16 // elem_bytes, 4, 1) if F % v == 0)
    lanes = -(-F // vec)
    lpr = next((p for p in (8, 16, 32) if lanes <= p), 64)
    return vec, lpr, -(-F // (lpr * vec))


@pytest.mark.parametrize("kind,elem,vecs", [("fp32", 4, (4, 1)), ("bf16", 2, (8, 4, 1))])
def test_variants_reach_every_instantiation(kind, elem, vecs):
    table = VARIANTS[kind]
    for F, want in table.items():
        assert select(F, elem) == want, (kind, F)
    reached = {(v, p) for v, p, _ in table.values()}
    assert reached == {(v, p) for v in vecs for p in (8, 16, 32, 64)}
    assert len(reached) == (8 if kind == "fp32" else 12)
    for v in vecs:  # a multi-pass case per VEC, and a partial last pass at LPR 64
        assert any(vv == v and n > 1 for vv, _, n in table.values()), (kind, v)
        assert any(vv == v and p == 64 and F % (64 * v) for F, (vv, p, _) in table.items())
    assert [select(F, 4) for F in MANY_F] == [(4, 8, 1), (1, 64, 2)]
    assert select(128, 4)[:2] == (4, 32) and select(29, 4)[:2] == (1, 32)  # two-source cases


# ------------------------------------------------------------------------------ the inputs
def test_ladder_pattern():
    csr = ladder_csr()
    deg = csr.degree()
    assert csr.num_rows == 142 and csr.num_cols == NSRC and int(csr.col.max()) < NSRC
    assert deg[:137].tolist() == list(range(137)) and int(deg[137]) == 1027 == 32 * 32 + 3
    for G in (1, 2, 4, 8):
        edges = {4 * G * k + o for k in range(1, 128 // (4 * G) + 1) for o in (-1, 0, 1)}
        edges |= {2 * G * k for k in range(1, 128 // (2 * G) + 1)}
        assert edges <= set(deg.tolist()), G
    for r, d in zip(SINGLE_ROWS, SINGLE):
        c = csr.col[int(csr.rowptr[r]):int(csr.rowptr[r + 1])]
        assert c.numel() == d and bool((c == c[0]).all())
    # rows of degree >= 20 repeat sources: ties across lane groups
    rep = [r for r in range(20, 137)
           if csr.col[int(csr.rowptr[r]):int(csr.rowptr[r + 1])].unique().numel() < r]
    assert len(rep) > 60
    assert ladder_csr(torch.int32).col.dtype == torch.int32
    assert torch.equal(ladder_csr(torch.int32).col.long(), csr.col)
    a, b = csr.split_columns(SPLIT)  # the two-source cases: every kind of row
    da, db = a.degree(), b.degree()
    assert bool(((da > 0) & (db == 0)).any()) and bool(((da == 0) & (db > 0)).any())
    assert bool(((da > 0) & (db > 0)).any()) and int(da[0] + db[0]) == 0
    t, rel = transposed(ladder_csr(torch.int64))
    assert t.col.dtype == torch.int64 and t.num_rows == NSRC and int(t.col.max()) < 142
    assert torch.equal(csr.col[csr.rowptr[t.col] + rel.long()], t.row_ids())


def test_many_rows_pattern():
    csr = many_rows_csr()
    assert csr.num_rows == csr.num_cols == MANY == 36867 and csr.col.dtype == torch.int32
    assert torch.equal(csr.degree(), torch.arange(MANY) % 4) and int(csr.col.max()) < MANY
    assert WAVES == 32768 and MANY - WAVES == 4099
    t, rel = transposed(csr)
    indeg = t.degree()
    for part in (indeg[:WAVES], indeg[WAVES:]):  # both rows of a wave: 0, 1 and >= 2 entries
        assert bool((part == 0).any()) and bool((part == 1).any()) and bool((part >= 2).any())
    assert t.num_rows == MANY and int(t.col.max()) < MANY and rel.numel() == csr.nnz
    p2 = second_pattern()
    assert bool((p2.degree()[1::2] == 0).all()) and bool((p2.degree()[0::2] > 0).all())
    assert int(p2.col.max()) < MANY
    u = union(csr, p2)
    assert torch.equal(u.degree(), csr.degree() + p2.degree())
    r = 2 * 3 + 0  # row 6: 2 entries of the first block, then 2 of the second
    assert u.col[int(u.rowptr[r]):int(u.rowptr[r + 1])].tolist() == \
        csr.col[int(csr.rowptr[r]):int(csr.rowptr[r + 1])].tolist() + \
        p2.col[int(p2.rowptr[r]):int(p2.rowptr[r + 1])].tolist()


def test_split_slots_names_the_blocks():
    full = ladder_csr()
    x = values("plain", NSRC, 5, 3)
    ref = pna_contract(full.rowptr, full.col, x)
    a, b = full.split_columns(SPLIT)
    want = split_slots(full, ref["amax"])
    src = torch.where(want >= 0,
                      a.col.long()[(a.rowptr[:-1, None] + want.long().clamp(min=0)).clamp(
                          max=a.nnz - 1)],
                      SPLIT + b.col.long()[(b.rowptr[:-1, None] + (-2 - want.long()).clamp(
                          min=0)).clamp(max=b.nnz - 1)])
    gold = full.col.long()[(full.rowptr[:-1, None] + ref["amax"].long().clamp(min=0)).clamp(
        max=full.nnz - 1)]
    ne = full.degree() > 0
    assert torch.equal(src[ne], gold[ne]) and bool((want[~ne] == -1).all())
    single = want[list(SINGLE_ROWS)]
    assert bool(((single == 0) | (single == -2)).all())  # slot 0 of its block
    # and they are what the CPU path records in two passes
    out = torch.empty(142, 5)
    arg = torch.empty(142, 5, dtype=torch.int32)
    K.segment_extreme(a.rowptr, a.col, x[:SPLIT], out, arg)
    K.segment_extreme(b.rowptr, b.col, x[SPLIT:], out, arg, second=True)
    assert torch.equal(arg, want) and torch.equal(out.double(), ref["max"])


# ------------------------------------------------- the slot-at-a-time contracts are the contracts
HEAD = 400


def _head(csr: CSR, n=HEAD) -> CSR:
    return CSR(csr.rowptr[:n + 1], csr.col[:int(csr.rowptr[n])], csr.num_cols)


def _same(got, want, dtype):
    if dtype == torch.float32 or not want.is_floating_point():
        assert torch.equal(got, want)
    else:
        torch.testing.assert_close(got, want, atol=1e-12, rtol=1e-12)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_slot_contracts_equal_the_row_contracts(dtype):
    F = 6
    csr = many_rows_csr()
    x = values("plain", MANY, F, 5)
    t = temperature("channel", F)
    g = {a: values("plain", MANY, F, 20 + i) for i, a in enumerate(ALL)}
    h = _head(csr)
    so, sl = many_softmax(csr.rowptr, csr.col, x, t, dtype)
    ro, rl = softmax_contract(h.rowptr, h.col, x, t, dtype=dtype)
    _same(so[:HEAD], ro, dtype)
    _same(sl[:HEAD], rl, dtype)
    assert bool((sl[0] == float("-inf")).all()) and torch.count_nonzero(so[0]) == 0
    sp = many_pna(csr.rowptr, csr.col, x, dtype=dtype)
    rp = pna_contract(h.rowptr, h.col, x, dtype=dtype)
    for k in rp:
        _same(sp[k][:HEAD], rp[k], dtype)
    # the backward over the first 400 sources of the transpose (their entries name
    # destination rows anywhere)
    tc, rel = transposed(csr)
    th = _head(tc)
    assert int(th.degree().max()) >= 3
    inv = 1.0 / csr.degree().clamp(min=1).to(dtype)
    sdx, sdt = many_softmax_bwd(th.rowptr, th.col, x, t, g["mean"], so, sl, dtype)
    rdx, rdt = softmax_bwd_contract(th.rowptr, th.col, x, t, g["mean"], so, sl, dtype=dtype)
    _same(sdx, rdx, dtype)
    _same(sdt, rdt, dtype)
    for which in (ALL, ("std",), ("max",), ("min",)):
        gw = {a: g[a] for a in which}
        sb = many_pna_bwd(th.rowptr, th.col, rel, x, inv, sp, gw, dtype)
        rb = pna_bwd_contract(th.rowptr, th.col, rel[:th.nnz], x, inv, sp, gw, dtype=dtype)
        _same(sb, rb, dtype)


# ------------------------------------------------------------------- cached ladder references
@functools.lru_cache(maxsize=None)
def softmax_case(F, xkind="plain", tscale=None):
    """``dict(x, t, g, r64, r32, d64, d32)`` of the ladder: the forward contract in fp64 and
    fp32 and the backward contract over the whole transpose, each with its own forward.
    ``xkind="offset"``: ``100 + randn`` with the scalar ``t = tscale``."""
    csr = ladder_csr()
    x = values("plain", NSRC, F, F)
    if xkind == "offset":
        x = 100.0 + x
    t = temperature("channel", F) if tscale is None else torch.full((F,), float(tscale))
    g = values("plain", csr.num_rows, F, 1000 + F)
    tc, _ = transposed(csr)
    r64 = softmax_contract(csr.rowptr, csr.col, x, t)
    r32 = softmax_contract(csr.rowptr, csr.col, x, t, dtype=torch.float32)
    d64 = softmax_bwd_contract(tc.rowptr, tc.col, x, t, g, *r64)
    d32 = softmax_bwd_contract(tc.rowptr, tc.col, x, t, g, *r32, dtype=torch.float32)
    return dict(x=x, t=t, g=g, r64=r64, r32=r32, d64=d64, d32=d32)


@functools.lru_cache(maxsize=None)
def pna_case(F, xkind="plain"):
    """``dict(x, g, r64, r32)`` of the ladder (``g``: a gradient per aggregator)."""
    csr = ladder_csr()
    x = values(xkind, NSRC, F, F)
    g = {a: values("plain", csr.num_rows, F, 2000 + F + i) for i, a in enumerate(ALL)}
    return dict(x=x, g=g, r64=pna_contract(csr.rowptr, csr.col, x),
                r32=pna_contract(csr.rowptr, csr.col, x, dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def pna_bwd_case(F, which=ALL):
    """(fp64, fp32) backward contract of :func:`pna_case` for the aggregators ``which``."""
    c = pna_case(F)
    csr = ladder_csr()
    tc, rel = transposed(csr)
    deg = csr.degree().clamp(min=1)
    g = {a: c["g"][a] for a in which}
    return (pna_bwd_contract(tc.rowptr, tc.col, rel, c["x"], 1.0 / deg.double(), c["r64"], g),
            pna_bwd_contract(tc.rowptr, tc.col, rel, c["x"], 1.0 / deg.float(), c["r32"], g,
                             dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def extreme_case(F, dtype):
    """``dict(x, g, ref)`` of the ladder for segment max / min in ``dtype``: ``ref`` is the
    fp64 PNA contract of the (exactly widened) values; ``x`` / ``g`` are ``dtype``."""
    csr = ladder_csr()
    x = values("plain", NSRC, F, F).to(dtype)
    g = values("plain", csr.num_rows, F, 3000 + F).to(dtype)
    return dict(x=x, g=g, ref=pna_contract(csr.rowptr, csr.col, x.double()))


def extreme_bwd_case(F, dtype, minimum):
    """(fp64, fp32) backward contract of :func:`extreme_case`: ``g`` to the winning slot."""
    c = extreme_case(F, dtype)
    tc, rel = transposed(ladder_csr())
    name = "min" if minimum else "max"
    one = torch.ones(LADDER_ROWS)  # inv_deg: multiplies the absent mean / std terms only
    return tuple(pna_bwd_contract(tc.rowptr, tc.col, rel, c["x"].float(), one, c["ref"],
                                  {name: c["g"].float()}, dtype=dt)
                 for dt in (torch.float64, torch.float32))


@functools.lru_cache(maxsize=None)
def many_case(F):
    """The many-rows case: inputs, the slot-at-a-time contracts in fp64 / fp32 and their
    backward contracts over the whole transpose."""
    csr = many_rows_csr()
    x = values("plain", MANY, F, 40 + F)
    t = temperature("channel", F)
    g = {a: values("plain", MANY, F, 50 + F + i) for i, a in enumerate(ALL)}
    tc, rel = transposed(csr)
    res = dict(x=x, t=t, g=g)
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        inv = 1.0 / csr.degree().clamp(min=1).to(dt)
        s = many_softmax(csr.rowptr, csr.col, x, t, dt)
        p = many_pna(csr.rowptr, csr.col, x, dtype=dt)
        res["s" + tag], res["p" + tag] = s, p
        res["sd" + tag] = many_softmax_bwd(tc.rowptr, tc.col, x, t, g["mean"], *s, dt)
        res["pd" + tag] = many_pna_bwd(tc.rowptr, tc.col, rel, x, inv, p, g, dt)
        for name in ("max", "min"):
            res[name + "d" + tag] = many_pna_bwd(tc.rowptr, tc.col, rel, x, inv, p,
                                                 {name: g[name]}, dt)
    return res


@functools.lru_cache(maxsize=None)
def many_union_case(F):
    """The contracts over :func:`union` of the many-rows case and :func:`second_pattern`
    (both blocks read the same ``x``), and the second block's own extremes."""
    c = many_case(F)
    p2 = second_pattern()
    u = union(many_rows_csr(), p2)
    res = {}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        res["s" + tag] = many_softmax(u.rowptr, u.col, c["x"], c["t"], dt)
        res["p" + tag] = many_pna(u.rowptr, u.col, c["x"], dtype=dt)
    res["second"] = many_pna(p2.rowptr, p2.col, c["x"])
    return res


# ------------------------------------------------------------ the CPU path on these inputs
def ratio(got, ref64, ref32):
    """``max|got - fp64| / bound(fp64, fp32)``."""
    err = float((got.double() - ref64.double()).abs().max()) if got.numel() else 0.0
    return err / bound(ref64, ref32)


@pytest.mark.parametrize("F", FP32_F)
def test_cpu_path_meets_the_rule_on_the_ladder(F):
    csr = ladder_csr(torch.int32)
    tc, rel = transposed(csr)
    ne = csr.degree() > 0
    figs = {}
    c = softmax_case(F)
    out, lse = K.segment_softmax(csr.rowptr, csr.col, c["x"], c["t"])
    figs["softmax out"] = ratio(out, c["r64"][0], c["r32"][0])
    figs["softmax lse"] = ratio(lse[ne], c["r64"][1][ne], c["r32"][1][ne])
    assert torch.count_nonzero(out[~ne]) == 0 and bool((lse[~ne] == float("-inf")).all())
    dx, part = K.segment_softmax_bwd(tc.rowptr, tc.col, c["x"], c["t"], c["g"], out, lse)
    figs["softmax dx"] = ratio(dx, c["d64"][0], c["d32"][0])
    figs["softmax dt"] = ratio(part.double().sum(0), c["d64"][1], c["d32"][1])
    for r in SINGLE_ROWS:  # one source, repeated: the row itself
        src = c["x"][int(csr.col[int(csr.rowptr[r])])]
        figs["softmax single"] = max(figs.get("softmax single", 0.0),
                                     ratio(out[r], src.double(), c["r32"][0][r]))
    p = pna_case(F)
    new = lambda dt=torch.float32: torch.empty(142, F, dtype=dt)  # noqa: E731
    o = dict(mean=new(), sdev=new(), vmax=new(), amax=new(torch.int32), vmin=new(),
             amin=new(torch.int32))
    K.segment_pna(csr.rowptr, csr.col, p["x"], **o)
    figs["pna mean"] = ratio(o["mean"], p["r64"]["mean"], p["r32"]["mean"])
    figs["pna sdev"] = ratio(o["sdev"], p["r64"]["std"], p["r32"]["std"])
    for a in ("max", "min"):
        assert torch.equal(o["v" + a].double(), p["r64"][a])
        assert torch.equal(o["a" + a], p["r64"]["a" + a])
        assert bool((o["a" + a][list(SINGLE_ROWS)] == 0).all())
        eo, ea = K.segment_extreme(csr.rowptr, csr.col, p["x"], minimum=a == "min")
        assert torch.equal(eo, o["v" + a]) and torch.equal(ea, o["a" + a])
    root = torch.full((len(SINGLE_ROWS), F), math.sqrt(EPS), dtype=torch.float64)
    rows = list(SINGLE_ROWS)
    figs["pna sdev single"] = ratio(o["sdev"][rows], root, p["r32"]["std"][rows])
    d64, d32 = pna_bwd_case(F)
    gd = p["g"]
    got = K.segment_pna_bwd(tc.rowptr, tc.col, rel, p["x"], csr.inv_degree(),
                            g_mean=gd["mean"], g_std=gd["std"], mean=o["mean"], sdev=o["sdev"],
                            g_max=gd["max"], amax=o["amax"], g_min=gd["min"], amin=o["amin"])
    figs["pna dx"] = ratio(got, d64, d32)
    for minimum in (False, True):
        e = extreme_case(F, torch.float32)
        e64, e32 = extreme_bwd_case(F, torch.float32, minimum)
        arg = o["amin" if minimum else "amax"]
        figs["extreme dx"] = max(figs.get("extreme dx", 0.0), ratio(
            K.segment_extreme_bwd(tc.rowptr, tc.col, rel, e["g"], arg), e64, e32))
    for k, v in figs.items():
        print(f"cpu[F={F}] {k}: error / bound {v:.3f}")
    assert all(v <= 1.0 for v in figs.values()), figs
