"""Gated neighbourhood aggregation and the ResGatedGraphConv layer on the CPU: the op against
an fp64 contract written here row by row (it shares no code with ops/reference.py) and against
a dense masked-sum expression, its saturated limits (``k`` shifted by +-100: the plain
neighbour sum of ``v`` / zero), the accumulate mode against one pass over the unsplit CSR, the
distributed op and ``CommAwareResGatedGraphConv`` at W = 2, 3 against W = 1 / a dense
evaluation."""
import copy
import functools

import pytest
import torch

from dgraph_amd.data.synthetic import SHAPES, build_partition
from dgraph_amd.ops import kernels as K
from dgraph_amd.ops.aggregate import gated_aggregate
from dgraph_amd.ops.csr import CSR
from dgraph_amd.parallel.dist_graph import DistGraph, dist_gated_aggregate
from test_pna import _sum_rows, small_csr, values
from test_softmax_aggr import SPLIT, split_csr


# ------------------------------------------------------------------ the contract, by rows
def gated_contract(rowptr, col, k, q, v, dtype=torch.float64):
    """``(out, ds)`` of every CSR row, one row at a time, in ``dtype``: with ``s = sigmoid(k[r]
    + q[c])`` over the row's entries ``c``, ``out = sum s v[c]`` and ``ds = sum s (1 - s)
    v[c]``; zeros for an empty row. The sums are :func:`test_pna._sum_rows` (fp32: one entry
    at a time). Differentiable in ``k``, ``q`` and ``v`` in fp64."""
    k, q, v = k.to(dtype), q.to(dtype), v.to(dtype)
    F = k.shape[1]
    rp = rowptr.tolist()
    outs, dss = [], []
    for r in range(len(rp) - 1):
        s, e = rp[r], rp[r + 1]
        if e == s:
            outs.append(torch.zeros(F, dtype=dtype))
            dss.append(torch.zeros(F, dtype=dtype))
            continue
        c = col[s:e].long()
        sg = torch.sigmoid(k[r] + q[c])
        outs.append(_sum_rows(sg * v[c]))
        dss.append(_sum_rows(sg * (1 - sg) * v[c]))
    if not outs:
        return torch.zeros(0, F, dtype=dtype), torch.zeros(0, F, dtype=dtype)
    return torch.stack(outs), torch.stack(dss)


def gated_bwd_contract(t_rowptr, t_col, k, q, v, g, dtype=torch.float64):
    """The source-side backward formula of the kernel, one source row at a time, in
    ``dtype``: per entry ``r`` of source row ``c``, ``s = sigmoid(k[r] + q[c])``; ``dv[c] =
    sum s g[r]`` and ``dq[c] = v[c] sum s (1 - s) g[r]``. Returns ``(dq, dv)``."""
    k, q, v, g = k.to(dtype), q.to(dtype), v.to(dtype), g.to(dtype)
    C, F = t_rowptr.numel() - 1, q.shape[1]
    rp = t_rowptr.tolist()
    dq = torch.zeros(C, F, dtype=dtype)
    dv = torch.zeros(C, F, dtype=dtype)
    for c in range(C):
        s, e = rp[c], rp[c + 1]
        if e == s:
            continue
        r = t_col[s:e].long()
        sg = torch.sigmoid(k[r] + q[c])
        dv[c] = _sum_rows(sg * g[r])
        dq[c] = v[c] * _sum_rows(sg * (1 - sg) * g[r])
    return dq, dv


def dense_gated(csr, k, q, v):
    """``out[i] = sum_j M[i, j] sigmoid(k[i] + q[j]) v[j]`` with ``M`` the dense entry-count
    matrix of ``csr`` (parallel entries count as often as they occur)."""
    M = torch.zeros(csr.num_rows, csr.num_cols, dtype=k.dtype)
    M.index_put_((csr.row_ids().long(), csr.col.long()),
                 torch.ones(csr.nnz, dtype=k.dtype), accumulate=True)
    gate = torch.sigmoid(k.unsqueeze(1) + q.unsqueeze(0))  # [R, C, F]
    return (M.unsqueeze(2) * gate * v.unsqueeze(0)).sum(1)


@functools.lru_cache(maxsize=None)
def _small_case():
    csr = small_csr()
    k = values("plain", 40, 5, 6).double()
    q = values("plain", 30, 5, 7).double()
    v = values("plain", 30, 5, 9).double()
    gy = values("plain", 40, 5, 8).double()
    return csr, k, q, v, gy


def test_op_matches_contract_and_dense_fp64():
    csr, k, q, v, gy = _small_case()
    kr, qr, vr = (t.clone().requires_grad_() for t in (k, q, v))
    ref, _ = gated_contract(csr.rowptr, csr.col, kr, qr, vr)
    gref = torch.autograd.grad((ref * gy).sum(), (kr, qr, vr))
    ki, qi, vi = (t.clone().requires_grad_() for t in (k, q, v))
    out = gated_aggregate(ki, qi, vi, csr)
    assert out.shape == (40, 5) and out.dtype == torch.float64
    torch.testing.assert_close(out.detach(), ref.detach(), atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(out.detach(), dense_gated(csr, k, q, v), atol=1e-12, rtol=1e-12)
    assert torch.count_nonzero(out[3]) == 0  # the empty row
    c4 = int(csr.col[csr.rowptr[4]])  # degree 1: its one source
    torch.testing.assert_close(out[4].detach(), torch.sigmoid(k[4] + q[c4]) * v[c4],
                               atol=1e-14, rtol=1e-14)
    out.backward(gy)
    for name, got, want in zip("kqv", (ki.grad, qi.grad, vi.grad), gref):
        torch.testing.assert_close(got, want, atol=1e-12, rtol=1e-12, msg=lambda m: name + m)
    # the lazy export
    from dgraph_amd import ops
    assert ops.gated_aggregate is gated_aggregate


def test_backward_formula_is_the_gradient():
    """The explicit backward contract (what the kernels evaluate: ``dk = g * ds``, the
    source-side sums) equals autograd of the forward contract in fp64, and the low-level
    wrappers return ``ds`` and the two source gradients."""
    csr, k, q, v, gy = _small_case()
    kr, qr, vr = (t.clone().requires_grad_() for t in (k, q, v))
    ref, ds = gated_contract(csr.rowptr, csr.col, kr, qr, vr)
    gk, gq, gv = torch.autograd.grad((ref * gy).sum(), (kr, qr, vr))
    tp = csr.transpose()
    dq, dv = gated_bwd_contract(tp.rowptr, tp.col, k, q, v, gy)
    torch.testing.assert_close(gy * ds.detach(), gk, atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(dq, gq, atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(dv, gv, atol=1e-12, rtol=1e-12)
    out, d2 = K.segment_gated(csr.rowptr, csr.col, k, q, v, want_ds=True)
    torch.testing.assert_close(out, ref.detach(), atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(d2, ds.detach(), atol=1e-12, rtol=1e-12)
    o3, none = K.segment_gated(csr.rowptr, csr.col, k, q, v)
    assert none is None and torch.equal(o3, out)
    kdq, kdv = K.segment_gated_bwd_src(tp.rowptr, tp.col, k, q, v, gy)
    torch.testing.assert_close(kdq, gq, atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(kdv, gv, atol=1e-12, rtol=1e-12)
    # dq / dv as the halves of one buffer; a source nobody reads gets zeros
    both = torch.full((30, 10), 7.0, dtype=torch.float64)
    K.segment_gated_bwd_src(tp.rowptr, tp.col, k, q, v, gy, both[:, :5], both[:, 5:])
    assert torch.equal(both[:, :5], kdq) and torch.equal(both[:, 5:], kdv)
    unread = tp.degree() == 0
    if bool(unread.any()):
        assert torch.count_nonzero(both[unread]) == 0


def test_gradcheck_fp64():
    g = torch.Generator().manual_seed(0)
    csr = CSR.from_coo(torch.randint(0, 6, (20,), generator=g),
                       torch.randint(0, 9, (20,), generator=g), 6, 9)
    k = torch.randn(6, 3, dtype=torch.float64, generator=g).requires_grad_()
    q = torch.randn(9, 3, dtype=torch.float64, generator=g).requires_grad_()
    v = torch.randn(9, 3, dtype=torch.float64, generator=g).requires_grad_()
    assert torch.autograd.gradcheck(lambda a, b, c: gated_aggregate(a, b, c, csr), (k, q, v))


@pytest.mark.parametrize("shift", [100.0, -100.0])
def test_saturated_gate(shift):
    """``k`` shifted by +100: every gate is 1 to fp64 accuracy (``1 - sigmoid(90) < 1e-39``)
    and ``out`` is the plain neighbour sum of ``v``; by -100: every gate is below ``e^-90``
    and ``out`` is zero. Every gradient is finite (no ``inf * 0`` in either tail)."""
    csr, k, q, v, gy = _small_case()
    assert float((k.abs().max() + q.abs().max())) < 10.0
    ki, qi, vi = ((k + shift).requires_grad_(), q.clone().requires_grad_(),
                  v.clone().requires_grad_())
    out = gated_aggregate(ki, qi, vi, csr)
    want = K.spmm(csr.rowptr, csr.col, v) if shift > 0 else torch.zeros_like(out)
    torch.testing.assert_close(out.detach(), want, atol=1e-13, rtol=1e-13)
    out.backward(gy)
    for t in (ki, qi, vi):
        assert bool(torch.isfinite(t.grad).all())
    # the gate's derivative vanishes in both tails; dv is the (un)gated transposed sum
    assert float(ki.grad.abs().max()) < 1e-30 and float(qi.grad.abs().max()) < 1e-30
    tp = csr.transpose()
    wv = K.spmm(tp.rowptr, tp.col, gy) if shift > 0 else torch.zeros_like(v)
    torch.testing.assert_close(vi.grad, wv, atol=1e-13, rtol=1e-13)
    # fp32 on the reference path: finite as well
    o32, d32 = K.segment_gated(csr.rowptr, csr.col, (k + shift).float(), q.float(), v.float(),
                               want_ds=True)
    assert bool(torch.isfinite(o32).all()) and bool(torch.isfinite(d32).all())


# ------------------------------------------------------------------ two sources
def two_pass_gated(a, b, k, q, v, want_ds=True):
    """Pass 1 over the first block, then pass 2 over the second with ``accumulate=True``
    over all rows. Returns ``(out, ds, out of pass 1, ds of pass 1)``."""
    R, F = a.num_rows, k.shape[1]
    out = torch.empty(R, F, dtype=k.dtype, device=k.device)
    ds = torch.empty(R, F, dtype=k.dtype, device=k.device) if want_ds else None
    K.segment_gated(a.rowptr, a.col, k, q[:SPLIT], v[:SPLIT], out, ds)
    o1, d1 = out.clone(), (ds.clone() if want_ds else None)
    K.segment_gated(b.rowptr, b.col, k, q[SPLIT:], v[SPLIT:], out, ds, accumulate=True)
    return out, ds, o1, d1


@pytest.mark.parametrize("want_ds", [True, False])
def test_accumulate_mode_matches_unsplit(want_ds):
    full, a, b = split_csr()
    k = values("plain", 300, 6, 20).double()
    q = values("plain", 257, 6, 21).double()
    v = values("plain", 257, 6, 22).double()
    out, ds, o1, d1 = two_pass_gated(a, b, k, q, v, want_ds)
    ref, rds = gated_contract(full.rowptr, full.col, k, q, v)
    torch.testing.assert_close(out, ref, atol=1e-11, rtol=1e-12)
    absent = b.degree() == 0
    assert bool(absent[2]) and torch.equal(out[absent], o1[absent])
    if want_ds:
        torch.testing.assert_close(ds, rds, atol=1e-11, rtol=1e-12)
        assert torch.equal(ds[absent], d1[absent])
    else:
        assert ds is None
    # row 1: empty after pass 1, its one entry comes from the second block
    assert torch.count_nonzero(o1[1]) == 0
    torch.testing.assert_close(out[1], torch.sigmoid(k[1] + q[200]) * v[200], atol=1e-14,
                               rtol=1e-14)
    assert torch.count_nonzero(out[150]) == 0


def test_empty_patterns_strided_input_and_misuse():
    csr, k, q, v, gy = _small_case()
    # [k | q | v] as column views of one buffer (row stride 15), padded to 40 rows
    big = torch.zeros(40, 15, dtype=torch.float64)
    big[:, :5] = k
    big[:30, 5:10] = q
    big[:30, 10:] = v
    bigr = big.clone().requires_grad_()
    out = gated_aggregate(bigr[:, :5], bigr[:30, 5:10], bigr[:30, 10:], csr)
    torch.testing.assert_close(out.detach(), gated_aggregate(k, q, v, csr), atol=0, rtol=0)
    out.backward(gy)
    kr, qr, vr = (t.clone().requires_grad_() for t in (k, q, v))
    gated_aggregate(kr, qr, vr, csr).backward(gy)
    torch.testing.assert_close(bigr.grad[:, :5], kr.grad, atol=0, rtol=0)
    torch.testing.assert_close(bigr.grad[:30, 5:10], qr.grad, atol=0, rtol=0)
    torch.testing.assert_close(bigr.grad[:30, 10:], vr.grad, atol=0, rtol=0)
    assert torch.count_nonzero(bigr.grad[30:, 5:]) == 0
    # rows and no entries: zeros; q / v may have no rows
    empty = CSR(torch.zeros(8, dtype=torch.long), torch.zeros(0, dtype=torch.int32), 30)
    o, d = K.segment_gated(empty.rowptr, empty.col, k[:7].float(), q.float(), v.float(),
                           want_ds=True)
    assert o.shape == (7, 5) and torch.count_nonzero(o) == 0 and torch.count_nonzero(d) == 0
    o, _ = K.segment_gated(empty.rowptr, empty.col, k[:7], q[:0], v[:0])
    assert torch.count_nonzero(o) == 0
    # an accumulate pass without entries leaves everything as it is
    keep = torch.full((7, 5), 3.5, dtype=torch.float64)
    K.segment_gated(empty.rowptr, empty.col, k[:7], q, v, keep, accumulate=True)
    assert bool((keep == 3.5).all())
    # zero rows
    none = CSR(torch.zeros(1, dtype=torch.long), torch.zeros(0, dtype=torch.int32), 30)
    assert gated_aggregate(k[:0], q, v, none).shape == (0, 5)
    k0 = torch.zeros(3, 6, requires_grad=True)
    q0 = torch.zeros(0, 6, requires_grad=True)
    v0 = torch.zeros(0, 6, requires_grad=True)
    o = gated_aggregate(k0, q0, v0, CSR(torch.zeros(4, dtype=torch.long),
                                        torch.zeros(0, dtype=torch.int32), 0))
    o.sum().backward()
    assert o.shape == (3, 6) and q0.grad.shape == (0, 6) and v0.grad.shape == (0, 6)
    assert torch.count_nonzero(k0.grad) == 0
    # a backward without entries zeroes dq / dv
    dq, dv = K.segment_gated_bwd_src(torch.zeros(31, dtype=torch.long),
                                     torch.zeros(0, dtype=torch.int32), k[:0], q, v, gy[:0],
                                     torch.full((30, 5), 2.0, dtype=torch.float64),
                                     torch.full((30, 5), 2.0, dtype=torch.float64))
    assert torch.count_nonzero(dq) == 0 and torch.count_nonzero(dv) == 0
    # misuse
    with pytest.raises(ValueError):
        K.segment_gated(csr.rowptr, csr.col, k, q, v, accumulate=True)
    with pytest.raises(ValueError):
        K.segment_gated(csr.rowptr, csr.col, k, q, v[:, :4])
    with pytest.raises(ValueError):
        K.segment_gated(csr.rowptr, csr.col, k, q.float(), v)
    with pytest.raises(ValueError):
        gated_aggregate(k[:39], q, v, csr)
    with pytest.raises(ValueError):
        gated_aggregate(k, q[:29], v[:29], csr)


# ------------------------------------------------------------------ distributed
SHAPE = SHAPES["ogbn-arxiv"].scaled(0.01)
DF = 16


def _global_inputs(dtype, device="cpu", shape=SHAPE, F=DF):
    """``(k, qv, gy)`` of the whole graph: ``qv`` is ``[N, 2F]`` = ``[q | v]``."""
    g = torch.Generator().manual_seed(5)
    k = torch.randn(shape.num_nodes, F, generator=g)
    qv = torch.randn(shape.num_nodes, 2 * F, generator=g)
    gy = torch.randn(shape.num_nodes, F, generator=g)
    return tuple(t.to(dtype).to(device) for t in (k, qv, gy))


def run_dist_op(dtype, graph, sl, device, shape=SHAPE, F=DF):
    """``dist_gated_aggregate`` on the rows ``sl`` of the global inputs: ``(out, dk, dqv)``."""
    k, qv, gy = _global_inputs(dtype, device, shape, F)
    kl, ql = k[sl].clone().requires_grad_(), qv[sl].clone().requires_grad_()
    out = dist_gated_aggregate(kl, ql, graph)
    out.backward(gy[sl])
    return out.detach(), kl.grad, ql.grad


def dist_gated_body(rank, world, device="cpu", dtype=torch.float64):
    """W ranks against W = 1 on the same device and dtype: forward, ``dk`` and ``dqv`` at
    1e-9, and the W = 1 result against the row-by-row contract."""
    p1 = build_partition(SHAPE, 0, 1, device)
    g1 = DistGraph(p1["csr"], p1["L"], 0, symmetric=True)
    ref = run_dist_op(dtype, g1, slice(0, SHAPE.num_nodes), device)
    p = build_partition(SHAPE, rank, world, device)
    g = DistGraph(p["csr"], p["L"], p["H"], p["send_local_idx"], p["send_splits"],
                  p["recv_splits"])
    sl = slice(p["offsets"][rank], p["offsets"][rank + 1])
    e0 = g.edges_aggregated
    got = run_dist_op(dtype, g, sl, device)
    assert g.edges_aggregated - e0 == 2 * g.nnz
    for name, a, b in zip(("out", "dk", "dqv"), got, ref):
        torch.testing.assert_close(a, b[sl], atol=1e-9, rtol=1e-9, msg=lambda m: name + m)
    # halo rows handed in (no exchange): the same result, bit for bit
    k, qv, _ = _global_inputs(dtype, device)
    o1, saved = g.aggregate_gated(k[sl], qv[sl])
    o2, s2 = g.aggregate_gated(k[sl], qv[sl], halo_rows=saved["halo"])
    assert saved["halo"].shape == (g.H, 2 * DF) and s2["halo"] is saved["halo"]
    assert torch.equal(o1, got[0]) and torch.equal(o2, o1) and torch.equal(s2["ds"], saved["ds"])
    if rank == 0:
        c = p1["csr"]
        want, _ = gated_contract(c.rowptr, c.col, k, qv[:, :DF], qv[:, DF:])
        torch.testing.assert_close(ref[0], want, atol=1e-10, rtol=1e-10)


@pytest.mark.parametrize("world", [2, 3])
def test_dist_gated_matches_single_rank(ranks, world):
    ranks(dist_gated_body, world)


def _chunked_exchange_body(rank, world):
    """F = 160 with the exchanges cut into column chunks (0-128 and a 32-column tail): a
    chunk carries the same channel range of q and of v, and the results are those of the
    unchunked exchanges."""
    shape, F = SHAPES["ogbn-arxiv"].scaled(0.003), 160
    p = build_partition(shape, rank, world, "cpu")
    sl = slice(p["offsets"][rank], p["offsets"][rank + 1])
    res = []
    for cb in (0, 1):
        g = DistGraph(p["csr"], p["L"], p["H"], p["send_local_idx"], p["send_splits"],
                      p["recv_splits"], chunk_bytes=cb)
        chunks = g._col_chunks(g.a2a, F, 16)
        assert chunks == ([(0, F)] if cb == 0 else [(0, 128), (128, F)])
        res.append(run_dist_op(torch.float64, g, sl, "cpu", shape, F))
        k, qv, _ = _global_inputs(torch.float64, "cpu", shape, F)
        _, saved = g.aggregate_gated(k[sl], qv[sl])
        res[-1] += (saved["halo"],)
    for name, a, b in zip(("out", "dk", "dqv", "halo"), *res):
        torch.testing.assert_close(a, b, atol=1e-12, rtol=1e-12, msg=lambda m: name + m)


def test_chunked_exchange_matches_unchunked(ranks):
    ranks(_chunked_exchange_body, 2)


def test_dist_single_rank_without_symmetry_flag():
    """W = 1 with the transposed pattern built (no ``symmetric=True``) equals the op."""
    p1 = build_partition(SHAPE, 0, 1, "cpu")
    g1 = DistGraph(p1["csr"], p1["L"], 0)
    out, dk, dqv = run_dist_op(torch.float64, g1, slice(0, SHAPE.num_nodes), "cpu")
    k, qv, gy = _global_inputs(torch.float64)
    ki, qi, vi = (t.clone().requires_grad_() for t in (k, qv[:, :DF], qv[:, DF:]))
    ref = gated_aggregate(ki, qi, vi, p1["csr"])
    ref.backward(gy)
    torch.testing.assert_close(out, ref.detach(), atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(dk, ki.grad, atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(dqv, torch.cat([qi.grad, vi.grad], 1), atol=1e-12, rtol=1e-12)


def _sends_without_halo_body(rank, world):
    """Rank 0 owns vertices 0-2 and reads only those; rank 1 owns 3-4 and reads vertices 0
    and 2 of rank 0: rank 0 has sends and H == 0, and must still post both exchanges."""
    grow = torch.tensor([0, 0, 1, 2, 3, 3, 3, 4, 4])
    gcol = torch.tensor([1, 2, 0, 0, 0, 4, 2, 2, 3])
    gcsr = CSR.from_coo(grow, gcol, 5, 5)
    k = torch.tensor([[0.5, -1.0], [2.0, 0.25], [-3.0, 4.0], [1.5, -2.5], [0.75, 3.5]]).double()
    qv = torch.arange(20.0, dtype=torch.float64).reshape(5, 4).sin()
    gy = torch.arange(1.0, 11.0, dtype=torch.float64).reshape(5, 2)
    kg, qg, vg = (t.clone().requires_grad_() for t in (k, qv[:, :2], qv[:, 2:]))
    ref = gated_aggregate(kg, qg, vg, gcsr)
    ref.backward(gy)
    if rank == 0:
        csr = CSR.from_coo(torch.tensor([0, 0, 1, 2]), torch.tensor([1, 2, 0, 0]), 3, 3)
        g = DistGraph(csr, 3, 0, torch.tensor([0, 2], dtype=torch.int32), [0, 2], [0, 0])
        assert g.halo is not None and g.H == 0
        sl = slice(0, 3)
    else:
        csr = CSR.from_coo(torch.tensor([0, 0, 0, 1, 1]), torch.tensor([2, 1, 3, 3, 0]), 2, 4)
        g = DistGraph(csr, 2, 2, torch.zeros(0, dtype=torch.int32), [0, 0], [2, 0])
        sl = slice(3, 5)
    kl, ql = k[sl].clone().requires_grad_(), qv[sl].clone().requires_grad_()
    out = dist_gated_aggregate(kl, ql, g)
    out.backward(gy[sl])
    torch.testing.assert_close(out.detach(), ref.detach()[sl], atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(kl.grad, kg.grad[sl], atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(ql.grad, torch.cat([qg.grad, vg.grad], 1)[sl], atol=1e-12,
                               rtol=1e-12)


def test_rank_with_sends_and_no_halo_rows(ranks):
    ranks(_sends_without_halo_body, 2)


# ------------------------------------------------------------------ the layer
LSHAPE = SHAPES["ogbn-arxiv"].scaled(0.003)  # small enough for a dense [N, N, C] evaluation
LF, LOUT = 6, 5


def make_layer(seed=0, **kw):
    from dgraph_amd.models import CommAwareResGatedGraphConv

    torch.manual_seed(seed)
    layer = CommAwareResGatedGraphConv(LF, LOUT, **kw)
    if layer.bias is not None:
        with torch.no_grad():
            layer.bias.copy_(torch.linspace(-0.5, 0.5, LOUT))
    return layer.double()


def _dense_layer_reference(layer, x, gy, csr):
    """The module docstring's formula in fp64, dense: the output, ``dx`` and the parameter
    gradients by name."""
    ref = copy.deepcopy(layer).double()
    ref.zero_grad()
    xr = x.clone().requires_grad_()
    out = dense_gated(csr, ref.lin_key(xr), ref.lin_query(xr), ref.lin_value(xr))
    if ref.lin_skip is not None:
        out = out + ref.lin_skip(xr)
    if ref.bias is not None:
        out = out + ref.bias
    (out * gy).sum().backward()
    return out.detach(), xr.grad, {n: q.grad for n, q in ref.named_parameters()}


def layer_body(rank, world, device="cpu", dtype=torch.float64, check=None, shape=LSHAPE,
               **kw):
    import torch.distributed as dist

    if check is None:
        def check(name, got, want):
            torch.testing.assert_close(got, want, atol=1e-9, rtol=1e-9, msg=lambda m: name + m)
    p1 = build_partition(shape, 0, 1, "cpu")
    g = torch.Generator().manual_seed(12)
    x = torch.randn(shape.num_nodes, LF, generator=g).double()
    gy = torch.randn(shape.num_nodes, LOUT, generator=g).double()
    layer = make_layer(**kw)
    ro, rdx, rgrads = _dense_layer_reference(layer, x, gy, p1["csr"])
    p = build_partition(shape, rank, world, device)
    graph = DistGraph(p["csr"], p["L"], p["H"], p["send_local_idx"], p["send_splits"],
                      p["recv_splits"]) if world > 1 else DistGraph(p["csr"], p["L"], 0)
    lo, hi = p["offsets"][rank], p["offsets"][rank + 1]
    layer = layer.to(device=device, dtype=dtype)
    xl = x[lo:hi].to(device=device, dtype=dtype).requires_grad_()
    out = layer(xl, graph)
    (out * gy[lo:hi].to(device=device, dtype=dtype)).sum().backward()
    check("out", out.detach().cpu().double(), ro[lo:hi])
    check("dx", xl.grad.cpu().double(), rdx[lo:hi])
    names = [n for n, _ in layer.named_parameters()]
    assert sorted(names) == sorted(rgrads)
    for name, q in layer.named_parameters():
        grad = q.grad
        if world > 1:
            dist.all_reduce(grad)
        check(name, grad.cpu().double(), rgrads[name])


def test_layer_matches_dense_single_rank():
    layer_body(0, 1)


@pytest.mark.parametrize("world", [2, 3])
def test_layer_matches_dense_ranks(ranks, world):
    ranks(layer_body, world)


def test_layer_state_dict_and_options():
    from dgraph_amd.models.resgated import CommAwareResGatedGraphConv

    # PyG's ResGatedGraphConv(LF, LOUT) state_dict: key names and shapes
    g = torch.Generator().manual_seed(1)
    pyg = {"bias": (LOUT,), "lin_key.weight": (LOUT, LF), "lin_key.bias": (LOUT,),
           "lin_query.weight": (LOUT, LF), "lin_query.bias": (LOUT,),
           "lin_value.weight": (LOUT, LF), "lin_value.bias": (LOUT,),
           "lin_skip.weight": (LOUT, LF)}
    sd = {n: torch.randn(*s, generator=g) for n, s in pyg.items()}
    layer = CommAwareResGatedGraphConv(LF, LOUT)
    assert {n: tuple(t.shape) for n, t in layer.state_dict().items()} == pyg
    layer.load_state_dict(sd, strict=True)
    assert torch.equal(layer.lin_skip.weight, sd["lin_skip.weight"])
    layer.reset_parameters()
    assert torch.count_nonzero(layer.bias) == 0
    # root_weight=False / bias=False against the dense formula
    layer_body(0, 1, root_weight=False)
    layer_body(0, 1, bias=False)
    bare = CommAwareResGatedGraphConv(LF, LOUT, root_weight=False, bias=False)
    assert bare.lin_skip is None and bare.bias is None
    assert sorted(bare.state_dict()) == sorted(n for n in pyg
                                               if n != "bias" and "skip" not in n)
    p = build_partition(LSHAPE, 0, 1, "cpu")
    graph = DistGraph(p["csr"], p["L"], 0)
    assert bare(torch.randn(LSHAPE.num_nodes, LF), graph).shape == (LSHAPE.num_nodes, LOUT)
