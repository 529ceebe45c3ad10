"""DropEdge fused into the CSR aggregation: the keep decision (``ops/philox.py``:
``edge_keep_mask``; ``csrc/kernels/philox.h``: ``edge_keep`` through ``edge_keep_host``), the op
(``ops/kernels.py``: ``spmm_drop`` / ``kept_degree``; ``ops/aggregate.py``: ``aggregate(...,
drop=)``), ``DistGraph.aggregate_drop`` across partitions and ``SAGEConv(drop_edge=)``, all
without a GPU.

:func:`drop_contract` is the oracle, also of tests/test_drop_edge_gpu.py: the contract written
as a dense masked matrix product in a chosen dtype. It shares no code with the CPU path of
``ops/kernels.py`` (which sums the kept entries with ``index_add_``); the keep decision it
takes from ``edge_keep_mask``, which this file pins against known answers and the host
function first.
"""
from __future__ import annotations

import math

import pytest
import torch

from test_gat_kernels import N, R, pattern

SEED = 83  # test_dot_attn_drop.SEED
BIG = 5000000000  # an id base above 2^32
KNOWN = {(3, 7): [3955669019, 31218901, 2982898460, 3555284915],
         (5000000003, 5000000007): [43276113, 2204863202, 779752352, 2588960405]}


# ------------------------------------------------------------------ the oracle
def keep_of(rowptr, col, seed, p, undirected=False, transposed=False, row_map=None,
            row_ids=None, col_ids=None, row_base=0, col_base=0):
    """``(out_rows [R], entry_rows [E], keep [E])``: output row per CSR row and per entry, and
    each entry's keep decision, from the contract's id rules."""
    from dgraph_amd.ops.philox import edge_keep_mask

    rowptr, col = rowptr.cpu().long(), col.cpu().long()
    nr = rowptr.numel() - 1
    out_rows = torch.arange(nr) if row_map is None else row_map.cpu().long()
    rows = torch.repeat_interleave(out_rows, rowptr[1:] - rowptr[:-1])
    rid = rows + row_base if row_ids is None else row_ids.cpu()[rows]
    cid = col + col_base if col_ids is None else col_ids.cpu()[col]
    dst, src = (cid, rid) if transposed else (rid, cid)
    return out_rows, rows, edge_keep_mask(int(seed), dst, src, p, undirected)


def drop_contract(rowptr, col, x, seed, p, *, undirected=False, transposed=False,
                  col_scale=None, row_scale=None, beta=0.0, out=None, row_map=None,
                  row_ids=None, col_ids=None, row_base=0, col_base=0, dtype=torch.float64):
    """``(out, kept)`` of the contract in ``dtype``: ``A_keep`` as a dense ``[rows, sources]``
    matrix of kept multiplicities, ``out[o] = row_scale[o] (A_keep (col_scale x))[o] + beta
    out[o]`` on the output rows of the pattern (other rows of ``out`` unchanged), ``kept`` the
    row sums of ``A_keep`` (int64, over all rows of ``out``)."""
    cv = lambda t: None if t is None else t.detach().cpu().to(dtype)  # noqa: E731
    x, cs, rs = cv(x), cv(col_scale), cv(row_scale)
    out_rows, rows, keep = keep_of(rowptr, col, seed, p, undirected, transposed, row_map,
                                   row_ids, col_ids, row_base, col_base)
    n_out = (rowptr.numel() - 1) if out is None else out.shape[0]
    A = torch.zeros(n_out, x.shape[0], dtype=torch.int64)
    A.index_put_((rows[keep], col.cpu().long()[keep]), torch.ones((), dtype=torch.int64),
                 accumulate=True)
    agg = A.to(dtype) @ (x if cs is None else x * cs[:, None])
    if rs is not None:
        agg = agg * rs[:, None]
    res = torch.zeros(n_out, x.shape[1], dtype=dtype) if out is None else cv(out).clone()
    res[out_rows] = agg[out_rows] + (beta * res[out_rows] if beta != 0.0 else 0.0)
    return res, A.sum(1)


def mean_scale(kept, dtype=torch.float64):
    return 1.0 / kept.clamp(min=1).to(dtype)


# ------------------------------------------------------------------ the keep decision
def test_known_answers():
    from dgraph_amd.ops.philox import M32, edge_keep_mask, philox4x32_10

    for (a, b), words in KNOWN.items():
        ctr = torch.tensor([a & M32, a >> 32, b & M32, b >> 32])
        assert philox4x32_10(ctr, torch.tensor([SEED, 0])).tolist() == words
        for p in (0.1, 0.5, 0.999):
            want = words[0] >= math.floor(p * 2 ** 32)
            got = edge_keep_mask(SEED, torch.tensor([a]), torch.tensor([b]), p)
            assert bool(got) == want


@pytest.mark.parametrize("undirected", [False, True], ids=["directed", "undirected"])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5, 0.999])
@pytest.mark.parametrize("base", [0, BIG], ids=["low", "above 2^32"])
def test_host_equals_torch(base, p, undirected):
    from dgraph_amd import _native
    from dgraph_amd.ops.philox import edge_keep_mask

    assert _native.load(), "native library missing"
    gen = torch.Generator().manual_seed(7)
    a = base + torch.randint(0, 3000, (4096,), generator=gen)
    b = base + torch.randint(0, 3000, (4096,), generator=gen)
    for seed in (0, SEED, 2 ** 62 - 1):
        host = _native.ops().edge_keep_host(seed, a, b, p, undirected)
        assert host.dtype == torch.bool and host.device.type == "cpu"
        assert torch.equal(host, edge_keep_mask(seed, a, b, p, undirected))
        assert torch.equal(host, edge_keep_mask(torch.tensor([seed]), a, b, p, undirected))
    if p == 0.0:
        assert host.all()


def test_undirected_is_symmetric_and_directed_is_not():
    from dgraph_amd.ops.philox import edge_keep_mask

    gen = torch.Generator().manual_seed(8)
    a = torch.randint(0, 2 ** 40, (4096,), generator=gen)
    b = torch.randint(0, 2 ** 40, (4096,), generator=gen)
    assert torch.equal(edge_keep_mask(SEED, a, b, 0.5, True), edge_keep_mask(SEED, b, a, 0.5, True))
    assert not torch.equal(edge_keep_mask(SEED, a, b, 0.5), edge_keep_mask(SEED, b, a, 0.5))
    lo, hi = torch.minimum(a, b), torch.maximum(a, b)
    assert torch.equal(edge_keep_mask(SEED, a, b, 0.5, True), edge_keep_mask(SEED, lo, hi, 0.5))


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_keep_rate(p):
    from dgraph_amd.ops.philox import edge_keep_mask

    n = 2 ** 16
    i = torch.arange(n)
    keep = edge_keep_mask(SEED, i // 256, i % 256 + 1000, p)  # distinct pairs
    sigma = math.sqrt(p * (1 - p) / n)
    assert abs(keep.double().mean().item() - (1 - p)) < 4 * sigma


def test_bad_probability_raises():
    from dgraph_amd import _native
    from dgraph_amd.ops.aggregate import EdgeDrop
    from dgraph_amd.ops.philox import edge_keep_mask

    i = torch.arange(4)
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError):
            edge_keep_mask(5, i, i, bad)
        with pytest.raises(ValueError):
            EdgeDrop(bad, torch.tensor([1]))
        with pytest.raises(RuntimeError):
            _native.ops().edge_keep_host(5, i, i, bad, False)
    with pytest.raises(ValueError):
        EdgeDrop(0.5, torch.tensor([1, 2]))


# ------------------------------------------------------------------ the op
F = 6


def _case(dtype=torch.float64):
    from dgraph_amd.ops.csr import CSR

    rowptr, col, _ = pattern()
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(N, F, generator=gen).to(dtype)
    g = torch.randn(R, F, generator=gen).to(dtype)
    return CSR(rowptr, col, N), x, g


def _drop(p=0.5, undirected=False, seed=SEED):
    from dgraph_amd.ops.aggregate import EdgeDrop

    return EdgeDrop(p, torch.tensor([seed]), undirected)


@pytest.mark.parametrize("undirected", [False, True], ids=["directed", "undirected"])
@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_aggregate_matches_dense(reduce, undirected):
    from dgraph_amd.ops.aggregate import aggregate

    csr, x, _ = _case()
    ref, kept = drop_contract(csr.rowptr, csr.col, x, SEED, 0.5, undirected=undirected)
    assert 0 < int(kept.sum()) < csr.nnz
    if reduce == "mean":
        ref = ref * mean_scale(kept)[:, None]
        lost = (kept == 0) & (csr.degree() > 0)
        assert lost.any(), "no non-empty row loses every entry: pick another seed"
        assert torch.equal(ref[lost], torch.zeros_like(ref[lost]))
    out = aggregate(x, csr, reduce=reduce, drop=_drop(0.5, undirected))
    torch.testing.assert_close(out, ref, atol=1e-12, rtol=1e-12)
    if reduce == "mean":
        assert torch.equal(out[lost], torch.zeros_like(out[lost]))


def test_kernel_wrappers_row_map_beta_strides_and_ids():
    from dgraph_amd.ops import kernels as K

    csr, x, _ = _case()
    hc = csr.compact_rows()
    assert hc.row_map is not None and hc.num_rows < csr.num_rows
    wide = torch.full((N, 2 * F + 1), float("nan"), dtype=torch.float64)
    wide[:, 1:F + 1] = x
    xs = wide[:, 1:F + 1]  # strided rows, off the base
    gen = torch.Generator().manual_seed(12)
    out0 = torch.randn(R, F, generator=gen).double()
    rs, cs = torch.rand(R, generator=gen).double() + 0.5, torch.rand(N, generator=gen).double()
    row_ids = torch.randperm(R, generator=gen) + BIG
    col_ids = torch.randperm(N, generator=gen) + BIG
    for kw in (dict(), dict(row_base=BIG, col_base=7), dict(row_ids=row_ids, col_ids=col_ids),
               dict(undirected=True, row_ids=row_ids, col_ids=col_ids)):
        ref, kept = drop_contract(hc.rowptr, hc.col, x, SEED, 0.5, row_map=hc.row_map, beta=1.0,
                                  out=out0, row_scale=rs, col_scale=cs, **kw)
        out = K.spmm_drop(hc.rowptr, hc.col, xs, out0.clone(), seed=SEED, p=0.5,
                          row_map=hc.row_map, beta=1.0, row_scale=rs, col_scale=cs, **kw)
        torch.testing.assert_close(out, ref, atol=1e-12, rtol=1e-12)
        empty = csr.degree() == 0
        assert torch.equal(out[empty], out0[empty])  # rows outside the compacted pattern
        got = K.kept_degree(hc.rowptr, hc.col, torch.full((R,), 5, dtype=torch.int32),
                            seed=SEED, p=0.5, accumulate=True, row_map=hc.row_map,
                            num_cols=N, **kw)
        assert got.dtype == torch.int32 and torch.equal(got.long(), kept + 5)
        plain = K.kept_degree(csr.rowptr, csr.col, seed=SEED, p=0.5, num_cols=N, **kw)
        assert torch.equal(plain.long(), kept)
    with pytest.raises(ValueError):
        K.spmm_drop(hc.rowptr, hc.col, x, seed=SEED, p=0.5, row_map=hc.row_map)
    with pytest.raises(ValueError):
        K.kept_degree(hc.rowptr, hc.col, seed=SEED, p=0.5, accumulate=True)


def test_transposed_pass_is_the_adjoint():
    from dgraph_amd.ops import kernels as K

    csr, x, g = _case()
    t = csr.transpose()
    gen = torch.Generator().manual_seed(13)
    row_ids = torch.randperm(R, generator=gen) + BIG
    col_ids = torch.randperm(N, generator=gen)
    for und in (False, True):
        kw = dict(seed=SEED, p=0.5, undirected=und)
        y = K.spmm_drop(csr.rowptr, csr.col, x, row_ids=row_ids, col_ids=col_ids, **kw)
        gx = K.spmm_drop(t.rowptr, t.col, g, transposed=True, row_ids=col_ids, col_ids=row_ids,
                         **kw)
        assert (y * g).sum().item() == pytest.approx((x * gx).sum().item(), rel=1e-12)
        ref, _ = drop_contract(t.rowptr, t.col, g, SEED, 0.5, undirected=und, transposed=True,
                               row_ids=col_ids, col_ids=row_ids)
        torch.testing.assert_close(gx, ref, atol=1e-12, rtol=1e-12)
        # the kept entries of the transposed pass are the forward's
        kf = K.kept_degree(csr.rowptr, csr.col, row_ids=row_ids, col_ids=col_ids, num_cols=N,
                           **kw)
        kt = K.kept_degree(t.rowptr, t.col, transposed=True, row_ids=col_ids, col_ids=row_ids,
                           num_cols=R, **kw)
        assert int(kf.sum()) == int(kt.sum())


def test_parallel_entries_share_one_fate():
    rowptr, col, rows = pattern()
    pairs = rows * N + col
    uniq, inv, cnt = torch.unique(pairs, return_inverse=True, return_counts=True)
    # 694 of the 1293 entries repeat an earlier (dst, src) pair
    assert pairs.numel() == 1293 and pairs.numel() - uniq.numel() == 694
    _, _, keep = keep_of(rowptr, col, SEED, 0.5)
    first = torch.zeros(uniq.numel(), dtype=torch.bool)
    first[inv] = keep
    assert torch.equal(first[inv], keep)


def test_empty_patterns():
    from dgraph_amd.ops.aggregate import aggregate
    from dgraph_amd.ops.csr import CSR

    empty = CSR(torch.zeros(6, dtype=torch.long), torch.zeros(0, dtype=torch.long), 4)
    x = torch.randn(4, 3, dtype=torch.float64, requires_grad=True)
    for reduce in ("sum", "mean"):
        out = aggregate(x, empty, reduce=reduce, drop=_drop())
        assert out.shape == (5, 3) and not out.any()
        out.sum().backward()
        assert not x.grad.any()
    norows = CSR(torch.zeros(1, dtype=torch.long), torch.zeros(0, dtype=torch.long), 4)
    assert aggregate(x, norows, reduce="mean", drop=_drop()).shape == (0, 3)


@pytest.mark.parametrize("undirected", [False, True], ids=["directed", "undirected"])
@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_gradcheck_fp64(reduce, undirected):
    from dgraph_amd.ops.aggregate import aggregate

    csr, x, _ = _case()
    x = x.clone().requires_grad_()
    drop = _drop(0.5, undirected)
    assert torch.autograd.gradcheck(lambda t: aggregate(t, csr, reduce=reduce, drop=drop), (x,))


@pytest.mark.parametrize("undirected", [False, True], ids=["directed", "undirected"])
def test_symmetric_pattern_runs_its_backward_on_itself(undirected):
    """A symmetric pattern (with parallel entries) marked ``symmetric``: the gradient equals
    the one over the unmarked pattern's real transpose, in both modes."""
    from dgraph_amd.ops.aggregate import aggregate
    from dgraph_amd.ops.csr import CSR

    gen = torch.Generator().manual_seed(14)
    a, b = torch.randint(0, 23, (2, 150), generator=gen)
    rows, cols = torch.cat([a, b]), torch.cat([b, a])
    x = torch.randn(23, F, generator=gen).double()
    g = torch.randn(23, F, generator=gen).double()
    grads = []
    for sym in (True, False):
        csr = CSR.from_coo(rows, cols, 23, 23)
        csr.symmetric = sym
        xr = x.clone().requires_grad_()
        aggregate(xr, csr, reduce="mean", drop=_drop(0.5, undirected)).backward(g)
        assert (csr.transpose() is csr) == sym
        grads.append(xr.grad)
    torch.testing.assert_close(grads[0], grads[1], atol=1e-12, rtol=1e-12)


def test_p0_and_none_are_the_plain_call_bitwise():
    from dgraph_amd.ops.aggregate import aggregate

    csr, x, g = _case(torch.float32)
    for reduce in ("sum", "mean"):
        outs, grads = [], []
        for drop in (None, _drop(0.0), _drop(0.0, True)):
            xr = x.clone().requires_grad_()
            out = aggregate(xr, csr, reduce=reduce, drop=drop)
            out.backward(g)
            outs.append(out.detach())
            grads.append(xr.grad)
        plain = aggregate(x, csr, reduce=reduce)
        assert all(torch.equal(o, plain) for o in outs)
        assert all(torch.equal(gr, grads[0]) for gr in grads)


def test_argument_errors():
    from dgraph_amd.ops import EdgeDrop
    from dgraph_amd.ops.aggregate import EdgeDrop as E2, aggregate

    assert EdgeDrop is E2
    csr, x, _ = _case()
    with pytest.raises(ValueError):
        aggregate(x, csr, edge_weight=torch.ones(csr.nnz), drop=_drop())
    with pytest.raises(ValueError):
        aggregate(x, csr, heads=2, drop=_drop())
    for reduce in ("max", "min", "std", "softmax", "prod"):
        with pytest.raises(ValueError):
            aggregate(x, csr, reduce=reduce, drop=_drop())


# ------------------------------------------------------------------ distributed
def _shape():
    from dgraph_amd.data.synthetic import SHAPES

    return SHAPES["ogbn-arxiv"].scaled(0.01)


DF = 5


def _global_inputs():
    g = torch.Generator().manual_seed(3)
    n = _shape().num_nodes
    return torch.randn(n, DF, generator=g).double(), torch.randn(n, DF, generator=g).double()


def _rank_graph(rank, world):
    """(graph with vertex_ids = global ids, lo, hi) of rank ``rank`` of ``world``."""
    from dgraph_amd.data.synthetic import build_partition
    from dgraph_amd.parallel.dist_graph import DistGraph

    p = build_partition(_shape(), rank, world, "cpu")
    lo, hi = p["offsets"][rank], p["offsets"][rank + 1]
    if world == 1:
        g = DistGraph(p["csr"], p["L"], 0)
        g.vertex_ids = torch.arange(p["L"])
    else:
        g = DistGraph(p["csr"], p["L"], p["H"], p["send_local_idx"], p["send_splits"],
                      p["recv_splits"])
        g.vertex_ids = torch.cat([torch.arange(lo, hi), p["halo_gids"].long()])
    return g, lo, hi


def dist_drop_body(rank, world):
    from dgraph_amd.parallel.dist_graph import dist_aggregate

    x, gy = _global_inputs()
    g1, _, _ = _rank_graph(0, 1)
    g, lo, hi = _rank_graph(rank, world)
    for mean in (True, False):
        for und in (False, True):
            drop = _drop(0.5, und)
            xr = x.clone().requires_grad_()
            ref, ref_kept = g1.aggregate_drop(xr.detach(), drop, mean)
            dist_aggregate(xr, g1, mean, drop=drop).backward(gy)
            dense, kept64 = drop_contract(g1.interior.rowptr, g1.interior.col, x, SEED, 0.5,
                                          undirected=und)
            if mean:
                assert torch.equal(ref_kept.long(), kept64)
                dense = dense * mean_scale(kept64)[:, None]
            torch.testing.assert_close(ref, dense, atol=1e-9, rtol=1e-9)
            xl = x[lo:hi].clone().requires_grad_()
            e0 = g.edges_aggregated
            out, kept = g.aggregate_drop(xl.detach(), drop, mean)
            assert g.edges_aggregated - e0 == g.nnz
            if mean:
                assert kept.dtype == torch.int32 and torch.equal(kept, ref_kept[lo:hi])
            else:
                assert kept is None
            torch.testing.assert_close(out, ref[lo:hi], atol=1e-9, rtol=1e-9)
            e0 = g.edges_aggregated
            o2 = dist_aggregate(xl, g, mean, drop=drop)
            o2.backward(gy[lo:hi])
            assert g.edges_aggregated - e0 == 2 * g.nnz
            assert torch.equal(o2.detach(), out)
            torch.testing.assert_close(xl.grad, xr.grad[lo:hi], atol=1e-9, rtol=1e-9)
    # p = 0 is the plain call
    assert torch.equal(dist_aggregate(xl.detach(), g, True, drop=_drop(0.0)),
                       dist_aggregate(xl.detach(), g, True))
    with pytest.raises(ValueError):
        dist_aggregate(xl.detach(), g, reduce="max", drop=_drop())


@pytest.mark.parametrize("world", [2, 3])
def test_dist_drop_matches_single_rank(ranks, world):
    ranks(dist_drop_body, world)


def test_local_numbering_is_the_default_and_bad_ids_raise():
    g1, _, _ = _rank_graph(0, 1)
    x, _ = _global_inputs()
    want, kept = g1.aggregate_drop(x, _drop(), True)
    g1.vertex_ids = None
    got, kept2 = g1.aggregate_drop(x, _drop(), True)
    assert torch.equal(got, want) and torch.equal(kept, kept2)
    g1.vertex_ids = torch.arange(3)
    with pytest.raises(ValueError):
        g1.aggregate_drop(x, _drop(), True)


def _sends_without_halo_body(rank, world):
    """The partition of test_pna._sends_without_halo_body: rank 0 has sends and H == 0, and
    must still post both exchanges."""
    from dgraph_amd.ops.aggregate import aggregate
    from dgraph_amd.ops.csr import CSR
    from dgraph_amd.parallel.dist_graph import DistGraph, dist_aggregate

    grow = torch.tensor([0, 0, 1, 2, 3, 3, 3, 4, 4])
    gcol = torch.tensor([1, 2, 0, 0, 0, 4, 2, 2, 3])
    gcsr = CSR.from_coo(grow, gcol, 5, 5)
    x = torch.tensor([[0.5, -1.0], [2.0, 0.25], [-3.0, 4.0], [1.5, -2.5], [0.75, 3.5]]).double()
    gy = torch.arange(1.0, 11.0, dtype=torch.float64).reshape(5, 2)
    if rank == 0:
        csr = CSR.from_coo(torch.tensor([0, 0, 1, 2]), torch.tensor([1, 2, 0, 0]), 3, 3)
        g = DistGraph(csr, 3, 0, torch.tensor([0, 2], dtype=torch.int32), [0, 2], [0, 0])
        assert g.halo is not None and g.H == 0
        g.vertex_ids, sl = torch.tensor([0, 1, 2]), slice(0, 3)
    else:
        csr = CSR.from_coo(torch.tensor([0, 0, 0, 1, 1]), torch.tensor([2, 1, 3, 3, 0]), 2, 4)
        g = DistGraph(csr, 2, 2, torch.zeros(0, dtype=torch.int32), [0, 0], [2, 0])
        g.vertex_ids, sl = torch.tensor([3, 4, 0, 2]), slice(3, 5)
    for seed in (SEED, 5):
        drop = _drop(0.5, seed=seed)
        xg = x.clone().requires_grad_()
        ref = aggregate(xg, gcsr, reduce="mean", drop=drop)
        ref.backward(gy)
        _, _, keep = keep_of(gcsr.rowptr, gcsr.col, seed, 0.5)
        assert 0 < int(keep.sum()) < 9
        xl = x[sl].clone().requires_grad_()
        out = dist_aggregate(xl, g, True, drop=drop)
        out.backward(gy[sl])
        torch.testing.assert_close(out.detach(), ref.detach()[sl], atol=1e-12, rtol=1e-12)
        torch.testing.assert_close(xl.grad, xg.grad[sl], atol=1e-9, rtol=1e-9)


def test_rank_with_sends_and_no_halo_rows(ranks):
    ranks(_sends_without_halo_body, 2)


# ------------------------------------------------------------------ the layer
LF, LOUT = 6, 5


def _layer(**kw):
    from dgraph_amd.models.sage import SAGEConv

    torch.manual_seed(0)
    layer = SAGEConv(LF, LOUT, **kw).double()
    with torch.no_grad():
        layer.bias.uniform_(-1, 1)
    return layer


def _layer_inputs():
    g = torch.Generator().manual_seed(12)
    n = _shape().num_nodes
    return torch.randn(n, LF, generator=g).double(), torch.randn(n, LOUT, generator=g).double()


def _dense_layer_reference(layer, csr, x, gy, seed, p, undirected):
    """``relu(x Ws + (D_keep^-1 A_keep x) Wn + b)`` with dense matrices and autograd."""
    xr = x.clone().requires_grad_()
    ws, wn, b = (t.detach().clone().requires_grad_()
                 for t in (layer.w_self, layer.w_neigh, layer.bias))
    _, rows, keep = keep_of(csr.rowptr, csr.col, seed, p, undirected)
    A = torch.zeros(csr.num_rows, csr.num_cols, dtype=torch.float64)
    A.index_put_((rows[keep], csr.col.long()[keep]), torch.ones((), dtype=torch.float64),
                 accumulate=True)
    A = A / A.sum(1).clamp(min=1)[:, None]
    out = (xr @ ws + (A @ xr) @ wn + b).relu()
    (out * gy).sum().backward()
    return out.detach(), xr.grad, ws.grad, wn.grad, b.grad


def layer_body(rank, world, undirected=False):
    import torch.distributed as dist

    x, gy = _layer_inputs()
    layer = _layer(drop_edge=0.5, drop_undirected=undirected)
    g1, _, _ = _rank_graph(0, 1)
    ro, rdx, rws, rwn, rb = _dense_layer_reference(layer, g1.interior, x, gy, SEED, 0.5,
                                                   undirected)
    graph, lo, hi = _rank_graph(rank, world)
    xl = x[lo:hi].clone().requires_grad_()
    out = layer(xl, graph, drop_seed=SEED)
    (out * gy[lo:hi]).sum().backward()
    grads = [layer.w_self.grad, layer.w_neigh.grad, layer.bias.grad]
    if world > 1:
        for t in grads:
            dist.all_reduce(t)
    kw = dict(atol=1e-9, rtol=1e-9)
    torch.testing.assert_close(out.detach(), ro[lo:hi], **kw)
    torch.testing.assert_close(xl.grad, rdx[lo:hi], **kw)
    for got, want in zip(grads, (rws, rwn, rb)):
        torch.testing.assert_close(got, want, **kw)


@pytest.mark.parametrize("undirected", [False, True], ids=["directed", "undirected"])
def test_layer_training_matches_dense(undirected):
    layer_body(0, 1, undirected)


@pytest.mark.parametrize("world", [2, 3])
def test_layer_ranks_match_single_rank(ranks, world):
    ranks(layer_body, world)


def test_layer_eval_and_seeds():
    from dgraph_amd.models.sage import SAGEConv

    x, _ = _layer_inputs()
    graph, _, _ = _rank_graph(0, 1)
    layer, plain = _layer(drop_edge=0.5), _layer()
    assert set(plain.state_dict()) == {"w_self", "w_neigh", "bias"}  # no new buffers at 0
    assert torch.equal(layer.w_self, plain.w_self)
    a, b = layer(x, graph), layer(x, graph)  # training: the step counter advances
    assert int(layer.drop_step) == 2 and not torch.equal(a, b)
    stride, base = SAGEConv.DROP_SEED_STRIDE, int(layer.drop_base_seed)
    assert stride % 2 == 1
    assert torch.equal(a, layer(x, graph, drop_seed=base))
    assert torch.equal(b, layer(x, graph, drop_seed=torch.tensor([base + stride])))
    assert int(layer.drop_step) == 2  # a fixed seed leaves the counter alone
    layer.eval()
    assert torch.equal(layer(x, graph), plain(x, graph))
    assert int(layer.drop_step) == 2
    assert torch.equal(_layer(drop_edge=0.0).train()(x, graph), plain(x, graph))
    for kw in (dict(aggr="max", drop_edge=0.5), dict(drop_edge=1.0), dict(drop_edge=-0.5)):
        with pytest.raises(ValueError):
            SAGEConv(LF, LOUT, **kw)
