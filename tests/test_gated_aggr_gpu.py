"""The fused gated aggregation kernels (csrc/kernels/spmm_gated.hip, through
``K.segment_gated`` / ``K.segment_gated_bwd_src``), ``gated_aggregate``,
``dist_gated_aggregate`` and ``CommAwareResGatedGraphConv`` on the GPU against the fp64
evaluation of their contract (tests/test_gated_aggr.py: ``gated_contract`` /
``gated_bwd_contract``, one row at a time).

Inputs: the skewed CSR (300 rows over 257 columns, Poisson(7) degrees, row 0 with 5,000
entries, row 150 empty, rows 1 / 2 of degree 1 / 2) with ``k``, ``q``, ``v`` = randn, and
``k = +-100 + randn`` (``exp(100)`` is infinite in fp32: tells the ``exp(-|z|)`` form from a
plain ``1 / (1 + exp(-z))``).

Accuracy rule: ``|kernel - fp64| <= test_gat_kernels.bound(ref64, ref32)`` with ``ref32`` the
same contract in fp32 on the CPU; nothing is taken from the kernel's own output. Every figure
is printed before it is asserted. Largest ``error / bound`` seen on an MI355X (a record, not
an input to the bound):

    forward               out 0.139 (F = 600: err 3.6e-3, bound 2.6e-2, the 5,000-entry row)
                          ds 0.143   out of the degree-1 row 0.004
    source-side backward  dq 0.018   dv 0.020   dk = g * ds 0.131
    column views          out 0.118   ds 0.117   dq 0.018   dv 0.020
    k = +-100 + randn     out 0.015   ds 0.000   dq 0.000   dv 0.004
    two sources           out 0.047   ds 0.022   the row pass 1 left empty 0.005
    split patterns        dq 0.013   dv 0.007
    op                    out 0.022   dk 0.026   dq 0.007   dv 0.009
    W = 2 op              out 0.004   dk 0.006   d[q | v] 0.005
    W = 2 layer           out 0.005   dx 0.008   every parameter gradient <= 0.008

The fp32 contract sums one entry at a time (test_pna._sum_rows), so the bounds are those of a
plain fp32 evaluation.
"""
from __future__ import annotations

import dataclasses
import functools

import pytest
import torch

from conftest import rank_device, run_ranks
from dgraph_amd.ops import kernels as K
from dgraph_amd.ops.aggregate import gated_aggregate
from test_gat_kernels import bound
from test_gated_aggr import gated_bwd_contract, gated_contract, two_pass_gated
from test_pna import skewed_csr, values
from test_softmax_aggr import SPLIT, split_csr

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.25e9  # what output buffers hold outside the blocks the kernel may write
RATIOS: dict = {}
ROWS, COLS = 300, 257
VEC1 = [1, 3, 13, 29, 67]  # VEC 1 at LPR 8 / 16 / 32 / 64, and a second column pass
VEC4 = [4, 32, 64, 128, 172, 600]  # VEC 4 at each LPR; three column passes with a tail
IDX = [torch.int32, torch.int64]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(RATIOS):
        print(f"\n[gated] largest error / bound, {k}: {RATIOS[k]:.3f}", end="")


def within(tag, name, got, ref64, ref32):
    """|got - fp64| against :func:`bound`; prints the figures, records the ratio."""
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape, f"{tag} {name}: shape {tuple(got.shape)}"
    assert bool(torch.isfinite(got).all()), f"{tag} {name}: not finite"
    err = float((got - ref64.double()).abs().max()) if got.numel() else 0.0
    bd = bound(ref64, ref32)
    print(f"{tag} {name}: err {err:.3e} bound {bd:.3e} ratio {err / bd:.3f}")
    key = f"{tag.split('[')[0]} {name}"
    RATIOS[key] = max(RATIOS.get(key, 0.0), err / bd)
    assert err <= bd, f"{tag} {name}: error {err:.3e} above the bound {bd:.3e}"


@functools.lru_cache(maxsize=None)
def fwd_refs(F, shift=0.0):
    """(k, q, v, fp64 (out, ds), fp32 (out, ds)) of the skewed case, shared by the index
    widths and by the backward tests."""
    csr = skewed_csr()
    k = values("plain", ROWS, F, 3 * F) + shift
    q = values("plain", COLS, F, 3 * F + 1)
    v = values("plain", COLS, F, 3 * F + 2)
    r64 = gated_contract(csr.rowptr, csr.col, k, q, v)
    r32 = gated_contract(csr.rowptr, csr.col, k, q, v, dtype=torch.float32)
    return k, q, v, r64, r32


@functools.lru_cache(maxsize=None)
def bwd_refs(F, shift=0.0):
    """(g, fp64 (dq, dv), fp32 (dq, dv)) over the transposed skewed pattern."""
    k, q, v, _, _ = fwd_refs(F, shift)
    tc = skewed_csr().transpose()
    g = values("plain", ROWS, F, 1000 + F)
    d64 = gated_bwd_contract(tc.rowptr, tc.col, k, q, v, g)
    d32 = gated_bwd_contract(tc.rowptr, tc.col, k, q, v, g, dtype=torch.float32)
    return g, d64, d32


def run_fwd(csr, k, q, v, want_ds):
    """The forward into sentinel-filled buffers."""
    R, F = csr.num_rows, k.shape[1]
    out = torch.full((R, F), SENT, device=k.device)
    ds = torch.full((R, F), SENT, device=k.device) if want_ds else None
    return K.segment_gated(csr.rowptr, csr.col, k, q, v, out, ds)


def check_fwd(tag, out, ds, r64, r32):
    """``out`` (and ``ds``) on every row, the empty row 150 exactly zero; no sentinel left."""
    within(tag, "out", out, r64[0], r32[0])
    assert torch.count_nonzero(out[150]) == 0 and not bool((out == SENT).any())
    if ds is not None:
        within(tag, "ds", ds, r64[1], r32[1])
        assert torch.count_nonzero(ds[150]) == 0 and not bool((ds == SENT).any())


@pytest.mark.parametrize("F", VEC1 + VEC4)
@pytest.mark.parametrize("idx", IDX)
def test_forward(F, idx):
    k, q, v, r64, r32 = fwd_refs(F)
    csr = skewed_csr(idx).to(DEV)
    kd, qd, vd = k.to(DEV), q.to(DEV), v.to(DEV)
    out, ds = run_fwd(csr, kd, qd, vd, True)
    check_fwd(f"fwd+ds[F={F}]", out, ds, r64, r32)
    o2, none = run_fwd(csr, kd, qd, vd, False)
    assert none is None
    check_fwd(f"fwd[F={F}]", o2, None, r64, r32)
    c1 = int(skewed_csr().col[skewed_csr().rowptr[1]])  # the degree-1 row: one product
    one = torch.sigmoid(k[1].double() + q[c1].double()) * v[c1].double()
    within(f"fwd[F={F}]", "out of the degree-1 row", o2[1], one, one.float())


@pytest.mark.parametrize("F", VEC1 + VEC4)
@pytest.mark.parametrize("idx", IDX)
def test_backward_src(F, idx):
    k, q, v, _, _ = fwd_refs(F)
    g, d64, d32 = bwd_refs(F)
    tc = skewed_csr(idx).transpose().to(DEV)
    dq = torch.full((COLS, F), SENT, device=DEV)
    dv = torch.full((COLS, F), SENT, device=DEV)
    K.segment_gated_bwd_src(tc.rowptr, tc.col, k.to(DEV), q.to(DEV), v.to(DEV), g.to(DEV),
                            dq, dv)
    within(f"bwd[F={F}]", "dq", dq, d64[0], d32[0])
    within(f"bwd[F={F}]", "dv", dv, d64[1], d32[1])
    assert not bool((dq == SENT).any()) and not bool((dv == SENT).any())
    unread = (skewed_csr().transpose().degree() == 0).to(DEV)
    assert torch.count_nonzero(dq[unread]) == 0 and torch.count_nonzero(dv[unread]) == 0
    # dk = g * ds, the destination side, from the forward kernel's second output
    _, _, _, r64, r32 = fwd_refs(F)
    _, ds = run_fwd(skewed_csr(idx).to(DEV), k.to(DEV), q.to(DEV), v.to(DEV), True)
    within(f"bwd[F={F}]", "dk", g.to(DEV) * ds, g.double() * r64[1], g * r32[1])


@pytest.mark.parametrize("F,pad", [(3, 1), (64, 4), (172, 8)])
def test_operands_as_column_views(F, pad):
    """``k``, ``q``, ``v`` as column views of ONE ``[N, 3F]`` buffer, ``out`` / ``ds`` as
    column blocks at offset ``pad`` of a wider sentinel-filled buffer, ``dq`` / ``dv`` as the
    halves of one ``[N, 2F]`` block of another: nothing outside the blocks is written (F =
    3: row strides 9 and 8; F = 64, 172: 16-B aligned blocks)."""
    k, q, v, r64, r32 = fwd_refs(F)
    csr = skewed_csr(torch.int32).to(DEV)
    kqv = torch.full((ROWS, 3 * F), SENT, device=DEV)
    kqv[:, :F] = k.to(DEV)
    kqv[:COLS, F:2 * F] = q.to(DEV)
    kqv[:COLS, 2 * F:] = v.to(DEV)
    kd, qd, vd = kqv[:, :F], kqv[:COLS, F:2 * F], kqv[:COLS, 2 * F:]
    wide = torch.full((ROWS, 2 * F + 2 * pad), SENT, device=DEV)
    out, ds = wide[:, pad:pad + F], wide[:, pad + F:pad + 2 * F]
    K.segment_gated(csr.rowptr, csr.col, kd, qd, vd, out, ds)
    check_fwd(f"views[F={F}]", out, ds, r64, r32)
    assert bool((wide[:, :pad] == SENT).all()) and bool((wide[:, pad + 2 * F:] == SENT).all())
    # without ds: the ds block keeps its sentinel
    wide.fill_(SENT)
    K.segment_gated(csr.rowptr, csr.col, kd, qd, vd, out)
    check_fwd(f"views[F={F}]", out, None, r64, r32)
    assert bool((wide[:, :pad] == SENT).all()) and bool((wide[:, pad + F:] == SENT).all())
    # the backward: g a column view, dq | dv the halves of one block
    g, d64, d32 = bwd_refs(F)
    tc = skewed_csr(torch.int32).transpose().to(DEV)
    gw = torch.full((ROWS, F + 2 * pad), SENT, device=DEV)
    gw[:, pad:pad + F] = g.to(DEV)
    dw = torch.full((COLS + 5, 2 * F + 2 * pad), SENT, device=DEV)
    dq, dv = dw[:, pad:pad + F], dw[:, pad + F:pad + 2 * F]
    K.segment_gated_bwd_src(tc.rowptr, tc.col, kd, qd, vd, gw[:, pad:pad + F], dq, dv)
    within(f"views[F={F}]", "dq", dq[:COLS], d64[0], d32[0])
    within(f"views[F={F}]", "dv", dv[:COLS], d64[1], d32[1])
    assert bool((dw[:, :pad] == SENT).all()) and bool((dw[:, pad + 2 * F:] == SENT).all())
    assert bool((dw[COLS:] == SENT).all())  # rows past the pattern's are not written


@pytest.mark.parametrize("shift", [100.0, -100.0])
def test_saturated_gate(shift):
    """``k = +-100 + randn``, F = 24: ``exp(100)`` overflows in fp32; out, ds and the
    source gradients are finite and within the bound (+100: the neighbour sum of ``v``)."""
    F = 24
    k, q, v, r64, r32 = fwd_refs(F, shift)
    csr = skewed_csr(torch.int32)
    out, ds = run_fwd(csr.to(DEV), k.to(DEV), q.to(DEV), v.to(DEV), True)
    check_fwd(f"saturated[{shift:+.0f}]", out, ds, r64, r32)
    g, d64, d32 = bwd_refs(F, shift)
    tc = csr.transpose().to(DEV)
    dq, dv = K.segment_gated_bwd_src(tc.rowptr, tc.col, k.to(DEV), q.to(DEV), v.to(DEV),
                                     g.to(DEV))
    within(f"saturated[{shift:+.0f}]", "dq", dq, d64[0], d32[0])
    within(f"saturated[{shift:+.0f}]", "dv", dv, d64[1], d32[1])
    if shift < 0:
        assert float(out.abs().max()) < 1e-30 and float(dv.abs().max()) < 1e-30


@functools.lru_cache(maxsize=None)
def split_refs(F=40):
    full, a, b = split_csr()
    k = values("plain", ROWS, F, 30)
    q = values("plain", COLS, F, 31)
    v = values("plain", COLS, F, 32)
    r64 = gated_contract(full.rowptr, full.col, k, q, v)
    r32 = gated_contract(full.rowptr, full.col, k, q, v, dtype=torch.float32)
    return k, q, v, r64, r32


@pytest.mark.parametrize("want_ds", [True, False])
@pytest.mark.parametrize("idx", IDX)
def test_two_sources_match_the_unsplit_csr(idx, want_ds):
    """Pass 1 over columns < 130, pass 2 (accumulate) over the rest, over all rows: the fp64
    contract on the unsplit CSR within the bound; rows without an entry in the second block
    are bitwise those of pass 1."""
    k, q, v, r64, r32 = split_refs()
    full, a, b = split_csr(idx)
    out, ds, o1, d1 = two_pass_gated(a.to(DEV), b.to(DEV), k.to(DEV), q.to(DEV), v.to(DEV),
                                     want_ds)
    check_fwd("two sources", out, ds, r64, r32)
    absent = (b.degree() == 0).to(DEV)
    assert int(absent.sum()) > 1 and bool(absent[2]) and bool(absent[150])
    assert torch.equal(out[absent], o1[absent])
    if want_ds:
        assert torch.equal(ds[absent], d1[absent])
    assert torch.count_nonzero(o1[1]) == 0  # empty in pass 1, then filled
    one = torch.sigmoid(k[1].double() + q[200].double()) * v[200].double()
    within("two sources", "out of the row pass 1 left empty", out[1], one, one.float())


def test_backward_on_the_split_patterns():
    """The source-side backward on the first block's and on the second block's transposed
    pattern: ``dq`` / ``dv`` of the sources of each block match the contract restricted to
    each edge set."""
    k, q, v, _, _ = split_refs()
    full, a, b = split_csr(torch.int32)
    g = values("plain", ROWS, 40, 77)
    for name, blk, sl in (("interior", a, slice(0, SPLIT)), ("halo", b, slice(SPLIT, COLS))):
        tc = blk.transpose()
        qs, vs = q[sl].contiguous(), v[sl].contiguous()
        assert tc.num_rows == qs.shape[0]
        d64 = gated_bwd_contract(tc.rowptr, tc.col, k, qs, vs, g)
        d32 = gated_bwd_contract(tc.rowptr, tc.col, k, qs, vs, g, dtype=torch.float32)
        td = tc.to(DEV)
        dq, dv = K.segment_gated_bwd_src(td.rowptr, td.col, k.to(DEV), qs.to(DEV), vs.to(DEV),
                                         g.to(DEV))
        within(f"split bwd[{name}]", "dq", dq, d64[0], d32[0])
        within(f"split bwd[{name}]", "dv", dv, d64[1], d32[1])


@pytest.mark.parametrize("F", [29, 172])
def test_bitwise_deterministic_and_index_width(F):
    """Two runs are bitwise equal, and int32 and int64 column ids give bitwise equal
    results, forward (with and without ds) and backward."""
    k, q, v = (values("plain", n, F, 9 + i).to(DEV)
               for i, n in enumerate((ROWS, COLS, COLS)))
    gy = values("plain", ROWS, F, 13).to(DEV)
    res = []
    for idx in (torch.int32, torch.int64, torch.int32):
        csr = skewed_csr(idx, seed=9)
        cd, tc = csr.to(DEV), csr.transpose().to(DEV)
        out, ds = K.segment_gated(cd.rowptr, cd.col, k, q, v, want_ds=True)
        o2, _ = K.segment_gated(cd.rowptr, cd.col, k, q, v)
        dq, dv = K.segment_gated_bwd_src(tc.rowptr, tc.col, k, q, v, gy)
        res.append((out, ds, o2, dq, dv))
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert torch.equal(a, b)


def test_op_against_fp64():
    """``gated_aggregate`` (F = 64) through autograd: out, dk, dq and dv."""
    F = 64
    k, q, v, _, _ = fwd_refs(F)
    csr = skewed_csr(torch.int32)
    gy = values("plain", ROWS, F, 5)
    refs = []
    for dt in (torch.float64, torch.float32):
        ins = [t.to(dt).clone().requires_grad_() for t in (k, q, v)]
        o, _ = gated_contract(csr.rowptr, csr.col, *ins, dtype=dt)
        refs.append((o.detach(),) + torch.autograd.grad((o * gy.to(dt)).sum(), ins))
    ins = [t.clone().to(DEV).requires_grad_() for t in (k, q, v)]
    out = gated_aggregate(*ins, csr.to(DEV))
    out.backward(gy.to(DEV))
    got = (out, ins[0].grad, ins[1].grad, ins[2].grad)
    for name, g, i in zip(("out", "dk", "dq", "dv"), got, range(4)):
        within("op", name, g, refs[0][i], refs[1][i])


def test_contract_checks_raise():
    csr = skewed_csr(torch.int32).to(DEV)
    F = 8
    k = values("plain", ROWS, F, 1).to(DEV)
    q = values("plain", COLS, F, 2).to(DEV)
    v = values("plain", COLS, F, 3).to(DEV)
    new = lambda R=ROWS, W=F, dt=torch.float32: torch.empty(R, W, dtype=dt, device=DEV)  # noqa: E731
    call = lambda kk, qq, vv, o, d=None, **kw: K.segment_gated(  # noqa: E731
        csr.rowptr, csr.col, kk, qq, vv, o, d, **kw)
    raw = K._native.ops().segment_gated_fwd
    err = (RuntimeError, ValueError, TypeError)
    with pytest.raises(err):  # non-fp32 input on the GPU
        call(k.double(), q.double(), v.double(), new(dt=torch.float64))
    with pytest.raises(err):
        raw(csr.rowptr, csr.col, k.half(), q.half(), v.half(), new(dt=torch.float16), None,
            False)
    with pytest.raises(err):
        raw(csr.rowptr, csr.col, k, q, v, new(), new(dt=torch.float16), False)
    with pytest.raises(err):  # a CPU operand
        raw(csr.rowptr, csr.col, k, q.cpu(), v, new(), None, False)
    with pytest.raises(err):  # widths that differ
        raw(csr.rowptr, csr.col, k, q[:, :4].contiguous(), v, new(), None, False)
    # a misaligned VEC-4 view (F % 4 == 0): row stride / base, never a silent VEC = 1 run
    with pytest.raises(err):
        call(torch.empty(ROWS, 10, device=DEV)[:, :8], q, v, new())
    with pytest.raises(err):
        call(k, torch.empty(COLS, 18, device=DEV)[:, 1:9], v, new())
    with pytest.raises(err):
        call(k, q, torch.empty(COLS, 18, device=DEV)[:, 9:17], new())
    with pytest.raises(err):
        call(k, q, v, torch.empty(ROWS, 10, device=DEV)[:, 1:9])
    with pytest.raises(err):
        call(k, q, v, new(), torch.empty(ROWS, 12, device=DEV)[:, 2:10])
    with pytest.raises(err):  # a column stride
        call(k.t().contiguous().t(), q, v, new())
    with pytest.raises(err):  # fewer k / out rows than the CSR
        call(k[:100], q, v, new())
    with pytest.raises(err):
        call(k, q, v, new()[:100])
    with pytest.raises(err):
        raw(csr.rowptr, csr.col, k, q, v, new(), new()[:100], False)
    with pytest.raises(err):  # q and v of different row counts
        call(k, q, v[:200], new())
    with pytest.raises(err):  # accumulate without an earlier result
        K.segment_gated(csr.rowptr, csr.col, k, q, v, accumulate=True)
    with pytest.raises(err):  # an int16 pattern
        raw(csr.rowptr, csr.col.short(), k, q, v, new(), None, False)
    tc = skewed_csr(torch.int32).transpose().to(DEV)
    g = new()
    bwd = lambda kk, qq, vv, gg, a, b: K._native.ops().segment_gated_bwd_src(  # noqa: E731
        tc.rowptr, tc.col, kk, qq, vv, gg, a, b)
    with pytest.raises(err):  # k with fewer rows than g
        bwd(k[:100], q, v, g, new(COLS), new(COLS))
    with pytest.raises(err):  # dq with fewer rows than the transposed pattern
        bwd(k, q, v, g, new(100), new(COLS))
    with pytest.raises(err):  # a misaligned half of a gradient buffer
        bwd(k, q, v, g, torch.empty(COLS, 18, device=DEV)[:, 1:9], new(COLS))
    with pytest.raises(err):
        bwd(k, q, v, g, new(COLS), new(COLS, dt=torch.float64))
    # empty launches return without launching
    none_rp = torch.zeros(1, dtype=torch.long, device=DEV)
    none_col = torch.zeros(0, dtype=torch.int32, device=DEV)
    o, d = K.segment_gated(none_rp, none_col, k[:0], q, v, want_ds=True)
    assert o.shape == (0, F) and d.shape == (0, F)
    assert K.segment_gated(none_rp, none_col, k[:0, :0], q[:, :0], v[:, :0])[0].shape == (0, 0)
    # rows and no entries: zeros on a first pass (q / v without rows), untouched on a second
    rp0 = torch.zeros(ROWS + 1, dtype=torch.long, device=DEV)
    o = torch.full((ROWS, F), SENT, device=DEV)
    d = torch.full((ROWS, F), SENT, device=DEV)
    K.segment_gated(rp0, none_col, k, q[:0], v[:0], o, d)
    assert torch.count_nonzero(o) == 0 and torch.count_nonzero(d) == 0
    o.fill_(SENT)
    K.segment_gated(rp0, none_col, k, q, v, o, accumulate=True)
    assert bool((o == SENT).all())
    # a backward without entries zeroes dq / dv
    rpt = torch.zeros(COLS + 1, dtype=torch.long, device=DEV)
    dq, dv = K.segment_gated_bwd_src(rpt, none_col, k[:0], q, v, g[:0],
                                     torch.full((COLS, F), SENT, device=DEV),
                                     torch.full((COLS, F), SENT, device=DEV))
    assert torch.count_nonzero(dq) == 0 and torch.count_nonzero(dv) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ op and layer, W = 2
def _tiny_shape():
    from dgraph_amd.data.synthetic import SHAPES

    return dataclasses.replace(SHAPES["ogbn-arxiv"], name="tiny-64", num_nodes=64,
                               num_directed_edges=400)


def _cpu_single_rank(fn, shape, dev):
    """``fn(dtype, graph, slice, device)`` on the whole graph on the CPU in fp64 and in fp32.
    The graph is generated on ``dev`` like the ranks' parts (the synthetic generator draws
    from the device's random stream: a CPU-built graph is another graph) and moved over."""
    from dgraph_amd.data.synthetic import build_partition
    from dgraph_amd.parallel.dist_graph import DistGraph

    p = build_partition(shape, 0, 1, dev)
    g1 = DistGraph(p["csr"].to("cpu"), p["L"], 0)
    return [fn(dt, g1, slice(0, shape.num_nodes), "cpu") for dt in (torch.float64, torch.float32)]


def _rank_graph(shape, rank, world, dev):
    from dgraph_amd.data.synthetic import build_partition
    from dgraph_amd.parallel.dist_graph import DistGraph

    p = build_partition(shape, rank, world, dev)
    g = DistGraph(p["csr"], p["L"], p["H"], p["send_local_idx"], p["send_splits"],
                  p["recv_splits"])
    return g, slice(p["offsets"][rank], p["offsets"][rank + 1])


def _w2_op_body(rank, world):
    import test_gated_aggr as D

    shape = _tiny_shape()

    def run(dt, graph, sl, dev):
        return D.run_dist_op(dt, graph, sl, dev, shape)

    dev = rank_device()
    r64, r32 = _cpu_single_rank(run, shape, dev)
    graph, sl = _rank_graph(shape, rank, world, dev)
    got = run(torch.float32, graph, sl, dev)
    for name, g, a, b in zip(("out", "dk", "dqv"), got, r64, r32):
        within("W=2 op", name, g, a[sl], b[sl])


def _w2_layer_body(rank, world):
    import torch.distributed as dist

    import test_gated_aggr as D

    shape = _tiny_shape()
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(shape.num_nodes, D.LF, generator=gen)
    gy = torch.randn(shape.num_nodes, D.LOUT, generator=gen)

    def run(dt, graph, sl, dev):
        layer = D.make_layer().to(device=dev, dtype=dt)
        xl = x[sl].to(device=dev, dtype=dt).requires_grad_()
        out = layer(xl, graph)
        (out * gy[sl].to(device=dev, dtype=dt)).sum().backward()
        return out.detach(), xl.grad, {n: q.grad for n, q in layer.named_parameters()}

    dev = rank_device()
    r64, r32 = _cpu_single_rank(run, shape, dev)
    graph, sl = _rank_graph(shape, rank, world, dev)
    out, dx, grads = run(torch.float32, graph, sl, dev)
    within("W=2 layer", "out", out, r64[0][sl], r32[0][sl])
    within("W=2 layer", "dx", dx, r64[1][sl], r32[1][sl])
    assert sorted(grads) == sorted(r64[2]) and len(grads) == 8
    for n, gq in grads.items():
        dist.all_reduce(gq)
        within("W=2 layer", f"grad {n}", gq, r64[2][n], r32[2][n])


def _w2_body(rank, world):
    from dgraph_amd.comm.rccl_exec import RCCLExecutor

    _w2_op_body(rank, world)
    _w2_layer_body(rank, world)
    torch.cuda.synchronize()
    RCCLExecutor.close_all()


def test_op_and_layer_two_ranks_rccl():
    """At W = 2 over real RCCL (both ranks on GPU 0, a 64-vertex graph, one process group for
    both): dist_gated_aggregate forward, dk and d[q | v] against the CPU fp64 result, then
    CommAwareResGatedGraphConv against the same layer on the CPU in fp64: output, dx and
    every parameter gradient after the all-reduce."""
    run_ranks(_w2_body, 2, backend="rccl-one-gpu")
