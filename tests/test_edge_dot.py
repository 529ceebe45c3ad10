"""Per-edge dot products (SDDMM) on the CPU: the op against a contract written here (it shares
no code with ops/reference.py), its gradients, ``aggregate``'s edge-weight gradient routed
through it, the distributed op at W = 2, 3 against W = 1, and the link-prediction decoder,
loss and negatives against dense ``z @ z.T`` indexing."""
import pytest
import torch

from dgraph_amd.data.synthetic import SHAPES, build_partition
from dgraph_amd.models.link_pred import InnerProductDecoder, negative_pattern, recon_loss
from dgraph_amd.ops import kernels as K
from dgraph_amd.ops.aggregate import aggregate
from dgraph_amd.ops.csr import CSR
from dgraph_amd.parallel.dist_graph import DistGraph, dist_edge_dot
from test_pna import small_csr, values


# ------------------------------------------------------------------ the contract, by slots
def slot_rows(rowptr):
    """The row that holds each slot, from a walk over ``rowptr`` (empty rows hold none)."""
    rp = rowptr.tolist()
    rows = []
    for r in range(len(rp) - 1):
        rows.extend([r] * (rp[r + 1] - rp[r]))
    return torch.tensor(rows, dtype=torch.long)


def edge_dot_contract(rowptr, col, a, b, heads=1, scale=1.0, row_scale=None,
                      dtype=torch.float64):
    """``s[k, h] = scale * row_scale[r(k)] * sum_d a[r(k), hD + d] * b[col[k], hD + d]`` in
    ``dtype``, every slot on its own (a slot's value depends on no other slot, so the slots
    are evaluated side by side). fp32: one term at a time, left to right, each product
    rounded before it is added (what "the contract evaluated in fp32" means,
    ``test_pna._sum_rows``); fp64: ``Tensor.sum``. ``a`` / ``b`` are taken as given (bf16
    inputs are rounded by the caller; their products are exact in fp32). Differentiable."""
    a, b = a.to(dtype), b.to(dtype)
    H, D = heads, a.shape[1] // heads
    rows = slot_rows(rowptr)
    ar = a[rows].reshape(-1, H, D)
    bc = b[col.long()].reshape(-1, H, D)
    if dtype == torch.float32:
        s = torch.zeros(rows.numel(), H, dtype=dtype)
        for d in range(D):
            s = s + ar[:, :, d] * bc[:, :, d]
    else:
        s = (ar * bc).sum(-1)
    f = torch.full((rows.numel(), 1), scale, dtype=dtype)
    if row_scale is not None:
        f = f * row_scale.to(dtype)[rows].unsqueeze(1)
    return f * s


def square_csr():
    """The first 30 rows of ``small_csr`` (30 x 30: an empty row, degrees 1 and 2)."""
    c = small_csr()
    return CSR(c.rowptr[:31].clone(), c.col[:int(c.rowptr[30])].clone(), 30)


def edge_dot_op():
    from dgraph_amd.ops import edge_dot

    return edge_dot


# ------------------------------------------------------------------ the op
@pytest.mark.parametrize("heads", [1, 2, 3])
def test_op_matches_contract_fp64(heads):
    csr = small_csr()
    a, b = values("plain", 40, 6, 1).double(), values("plain", 30, 6, 2).double()
    s = edge_dot_op()(a, b, csr, heads=heads, scale=0.7)
    assert s.shape == (csr.nnz, heads) and s.dtype == torch.float64
    ref = edge_dot_contract(csr.rowptr, csr.col, a, b, heads, 0.7)
    torch.testing.assert_close(s, ref, atol=1e-13, rtol=1e-13)
    # fp32 inputs: fp32 scores
    s32 = edge_dot_op()(a.float(), b.float(), csr, heads=heads, scale=0.7)
    assert s32.dtype == torch.float32
    torch.testing.assert_close(s32.double(), ref, atol=1e-5, rtol=1e-5)


def test_kernel_entry_row_scale_and_out():
    csr = small_csr()
    a, b = values("plain", 40, 6, 1).double(), values("plain", 30, 6, 2).double()
    rs = csr.inv_degree()
    ref = edge_dot_contract(csr.rowptr, csr.col, a, b, 2, -1.5, rs)
    s = K.edge_dot(csr.rowptr, csr.col, a, b, heads=2, scale=-1.5, row_scale=rs)
    torch.testing.assert_close(s, ref, atol=1e-13, rtol=1e-13)
    out = torch.full((csr.nnz, 2), 9.0, dtype=torch.float64)
    assert K.edge_dot(csr.rowptr, csr.col, a, b, out, heads=2, scale=-1.5, row_scale=rs) is out
    assert torch.equal(out, s)
    assert torch.equal(K.edge_dot(csr.rowptr, csr.col.long(), a, b, heads=2, scale=-1.5,
                                  row_scale=rs), s)


@pytest.mark.parametrize("heads", [1, 2, 3])
def test_gradcheck_fp64(heads):
    csr = small_csr()
    a = values("plain", 40, 6, 3).double().requires_grad_()
    b = values("plain", 30, 6, 4).double().requires_grad_()
    assert torch.autograd.gradcheck(lambda p, q: edge_dot_op()(p, q, csr, heads, 0.6), (a, b))
    ar, br = a.detach().clone().requires_grad_(), b.detach().clone().requires_grad_()
    g = values("plain", csr.nnz, heads, 5).double()
    edge_dot_op()(a, b, csr, heads, 0.6).backward(g)
    edge_dot_contract(csr.rowptr, csr.col, ar, br, heads, 0.6).backward(g)
    torch.testing.assert_close(a.grad, ar.grad, atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(b.grad, br.grad, atol=1e-12, rtol=1e-12)


def test_self_scores_sum_both_gradients():
    csr = square_csr()
    z = values("plain", 30, 6, 6).double().requires_grad_()
    zr = z.detach().clone().requires_grad_()
    g = values("plain", csr.nnz, 2, 7).double()
    s = edge_dot_op()(z, z, csr, heads=2)
    s.backward(g)
    ref = edge_dot_contract(csr.rowptr, csr.col, zr, zr, 2)
    ref.backward(g)
    torch.testing.assert_close(s.detach(), ref.detach(), atol=1e-13, rtol=1e-13)
    torch.testing.assert_close(z.grad, zr.grad, atol=1e-12, rtol=1e-12)
    assert torch.autograd.gradcheck(lambda p: edge_dot_op()(p, p, csr, 2), (z,))
    # a symmetric pattern's transpose is the pattern alone: the slot map is still right
    sym = CSR(csr.rowptr, csr.col, 30, symmetric=True)
    z2 = z.detach().clone().requires_grad_()
    edge_dot_op()(z2, z2, sym, heads=2).backward(g)
    torch.testing.assert_close(z2.grad, zr.grad, atol=1e-12, rtol=1e-12)


def test_empty_rows_no_entries_and_strided_inputs():
    csr = small_csr()
    assert int(csr.degree()[3]) == 0
    buf = values("plain", 40, 12, 8).double()
    a, b = buf[:, :6], buf[:30, 6:]  # column halves of one buffer
    s = edge_dot_op()(a, b, csr, heads=3)
    ref = edge_dot_contract(csr.rowptr, csr.col, a.contiguous(), b.contiguous(), 3)
    torch.testing.assert_close(s, ref, atol=1e-13, rtol=1e-13)
    # b with more rows than the pattern has columns: the extra rows get a zero gradient
    bb = values("plain", 33, 6, 9).double().requires_grad_()
    edge_dot_op()(a, bb, csr, heads=1).sum().backward()
    assert bb.grad.shape == (33, 6) and torch.count_nonzero(bb.grad[30:]) == 0
    empty = CSR(torch.zeros(41, dtype=torch.long), torch.zeros(0, dtype=torch.int32), 30)
    ar = a.contiguous().requires_grad_()
    s0 = edge_dot_op()(ar, b, empty, heads=3)
    assert s0.shape == (0, 3)
    s0.sum().backward()
    assert torch.count_nonzero(ar.grad) == 0
    assert K.edge_dot(empty.rowptr, empty.col, a, b, heads=2).shape == (0, 2)


def test_bad_arguments_raise():
    csr = small_csr()
    a, b = torch.zeros(40, 6), torch.zeros(30, 6)
    with pytest.raises(ValueError, match="heads"):
        edge_dot_op()(a, b, csr, heads=4)
    with pytest.raises(ValueError, match="rows"):
        edge_dot_op()(a[:39], b, csr)
    with pytest.raises(ValueError, match="columns"):
        edge_dot_op()(a, b[:29], csr)
    with pytest.raises(ValueError, match="width"):
        edge_dot_op()(a, torch.zeros(30, 5), csr)
    with pytest.raises(ValueError, match="heads"):
        K.edge_dot(csr.rowptr, csr.col, a, b, heads=4)


# ------------------------------------------------------------------ aggregate's backward
@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("heads", [1, 2])
def test_aggregate_edge_weight_gradient_is_the_contract(reduce, heads):
    csr = small_csr()
    x = values("plain", 30, 6, 10).double()
    g = values("plain", 40, 6, 11).double()
    w = values("plain", csr.nnz, heads, 12).double().requires_grad_()
    aggregate(x, csr, edge_weight=w, reduce=reduce, heads=heads).backward(g)
    rs = csr.inv_degree() if reduce == "mean" else None
    ref = edge_dot_contract(csr.rowptr, csr.col, g, x, heads, 1.0, rs)
    torch.testing.assert_close(w.grad, ref, atol=1e-13, rtol=1e-13)
    # fp32 weights: an fp32 gradient of the same function
    w32 = w.detach().float().requires_grad_()
    aggregate(x.float(), csr, edge_weight=w32, reduce=reduce, heads=heads).backward(g.float())
    assert w32.grad.dtype == torch.float32 and w32.grad.shape == w32.shape
    torch.testing.assert_close(w32.grad.double(), ref, atol=1e-5, rtol=1e-5)
    # a flat [nnz] weight keeps its shape
    if heads == 1:
        wf = w.detach().reshape(-1).clone().requires_grad_()
        aggregate(x, csr, edge_weight=wf, reduce=reduce).backward(g)
        torch.testing.assert_close(wf.grad, ref.reshape(-1), atol=1e-13, rtol=1e-13)


# ------------------------------------------------------------------ distributed
SHAPE = SHAPES["ogbn-arxiv"].scaled(0.01)
DF, DH, DSCALE = 12, 3, 0.8


def global_inputs(dtype, device, shape=SHAPE, F=DF):
    g = torch.Generator().manual_seed(21)
    a = torch.randn(shape.num_nodes, F, generator=g)
    b = torch.randn(shape.num_nodes, F, generator=g)
    return a.to(dtype).to(device), b.to(dtype).to(device)


def score_weights(grow, gcol, heads, dtype):
    """dL/ds of an edge as a function of its global (row, column, head), so that every
    partition of the graph weighs the same edge alike."""
    h = torch.arange(heads, device=grow.device)
    return torch.sin(0.37 * grow.unsqueeze(1) + 0.11 * gcol.unsqueeze(1) + h).to(dtype)


def rank_graph(shape, rank, world, device):
    """(graph, lo, global rows, global columns of the scores ``dist_edge_dot`` returns)."""
    p = build_partition(shape, rank, world, device)
    lo = p["offsets"][rank]
    if world == 1:
        g = DistGraph(p["csr"], p["L"], 0)
        return g, lo, p["csr"].row_ids(), p["csr"].col.long()
    g = DistGraph(p["csr"], p["L"], p["H"], p["send_local_idx"], p["send_splits"],
                  p["recv_splits"])
    grow = torch.cat([g.interior.row_ids(), g.halo.row_ids()]) + lo
    gcol = torch.cat([g.interior.col.long() + lo, p["halo_gids"][g.halo.col.long()]])
    return g, lo, grow, gcol


def run_dist(dtype, graph, lo, grow, gcol, device, shape=SHAPE, same=False):
    """(scores, da, db) of ``dist_edge_dot`` on one rank's graph under the loss
    ``sum(s * score_weights)``; ``same``: ``a is b`` (one gradient, the sum)."""
    a, b = global_inputs(dtype, device, shape)
    al = a[lo:lo + graph.L].clone().requires_grad_()
    bl = al if same else b[lo:lo + graph.L].clone().requires_grad_()
    s = dist_edge_dot(al, bl, graph, heads=DH, scale=DSCALE)
    (s * score_weights(grow, gcol, DH, s.dtype)).sum().backward()
    return s.detach(), al.grad, bl.grad


def expected_scores(dtype, grow, gcol, shape=SHAPE, same=False):
    a, b = global_inputs(dtype, "cpu", shape)
    b = a if same else b
    ar = a[grow.cpu()].view(-1, DH, DF // DH)
    return DSCALE * (ar * b[gcol.cpu()].view(-1, DH, DF // DH)).sum(-1)


def dist_edge_dot_body(rank, world):
    for same in (False, True):
        g1, _, r1, c1 = rank_graph(SHAPE, 0, 1, "cpu")
        s1, da1, db1 = run_dist(torch.float64, g1, 0, r1, c1, "cpu", same=same)
        torch.testing.assert_close(s1, expected_scores(torch.float64, r1, c1, same=same),
                                   atol=1e-12, rtol=1e-12)
        g, lo, grow, gcol = rank_graph(SHAPE, rank, world, "cpu")
        e0 = g.edges_aggregated
        s, da, db = run_dist(torch.float64, g, lo, grow, gcol, "cpu", same=same)
        assert g.edges_aggregated - e0 == 2 * g.nnz
        assert s.shape == (g.nnz, DH)
        torch.testing.assert_close(s, expected_scores(torch.float64, grow, gcol, same=same),
                                   atol=1e-12, rtol=1e-12)
        torch.testing.assert_close(da, da1[lo:lo + g.L], atol=1e-10, rtol=1e-10)
        torch.testing.assert_close(db, db1[lo:lo + g.L], atol=1e-10, rtol=1e-10)


@pytest.mark.parametrize("world", [2, 3])
def test_dist_edge_dot_matches_single_rank(ranks, world):
    ranks(dist_edge_dot_body, world)


def _sends_without_halo_body(rank, world):
    """Rank 0 owns vertices 0-2 and reads only those; rank 1 owns 3-4 and reads vertices 0
    and 2 of rank 0: rank 0 has sends and H == 0, and must still post both exchanges."""
    grow = torch.tensor([0, 0, 1, 2, 3, 3, 3, 4, 4])
    gcol = torch.tensor([1, 2, 0, 0, 0, 4, 2, 2, 3])
    gcsr = CSR.from_coo(grow, gcol, 5, 5)
    z = torch.tensor([[0.5, -1.0], [2.0, 0.25], [-3.0, 4.0], [1.5, -2.5], [0.75, 3.5]]).double()
    zg = z.clone().requires_grad_()
    ref = edge_dot_op()(zg, zg, gcsr, heads=2, scale=0.5)
    (ref * score_weights(grow, gcol, 2, ref.dtype)).sum().backward()
    if rank == 0:
        csr = CSR.from_coo(torch.tensor([0, 0, 1, 2]), torch.tensor([1, 2, 0, 0]), 3, 3)
        g = DistGraph(csr, 3, 0, torch.tensor([0, 2], dtype=torch.int32), [0, 2], [0, 0])
        assert g.halo is not None and g.H == 0
        sl, lrow, lcol = slice(0, 3), grow[:4], gcol[:4]
    else:
        csr = CSR.from_coo(torch.tensor([0, 0, 0, 1, 1]), torch.tensor([2, 1, 3, 3, 0]), 2, 4)
        g = DistGraph(csr, 2, 2, torch.zeros(0, dtype=torch.int32), [0, 0], [2, 0])
        halo_gids = torch.tensor([0, 2])
        lrow = torch.cat([g.interior.row_ids(), g.halo.row_ids()]) + 3
        lcol = torch.cat([g.interior.col.long() + 3, halo_gids[g.halo.col.long()]])
        sl = slice(3, 5)
    zl = z[sl].clone().requires_grad_()
    s = dist_edge_dot(zl, zl, g, heads=2, scale=0.5)
    (s * score_weights(lrow, lcol, 2, s.dtype)).sum().backward()
    want = 0.5 * (z[lrow].view(-1, 2, 1) * z[lcol].view(-1, 2, 1)).sum(-1)
    torch.testing.assert_close(s.detach(), want, atol=1e-13, rtol=1e-13)
    torch.testing.assert_close(zl.grad, zg.grad[sl], atol=1e-12, rtol=1e-12)


def test_rank_with_sends_and_no_halo_rows(ranks):
    ranks(_sends_without_halo_body, 2)


# ------------------------------------------------------------------ decoder, loss, negatives
def test_decoder_and_loss_match_dense():
    csr = square_csr()
    z = values("plain", 30, 6, 13).double().requires_grad_()
    neg = negative_pattern(csr, 3, torch.Generator().manual_seed(3))
    rows, nrows = slot_rows(csr.rowptr), slot_rows(neg.rowptr)
    dec = InnerProductDecoder()
    dense = z.detach() @ z.detach().t()
    torch.testing.assert_close(dec(z, csr).detach(), dense[rows, csr.col.long()].unsqueeze(1),
                               atol=1e-13, rtol=1e-13)
    torch.testing.assert_close(dec(z, csr, sigmoid=True).detach(),
                               torch.sigmoid(dense[rows, csr.col.long()]).unsqueeze(1),
                               atol=1e-13, rtol=1e-13)
    # two heads: the dense product of each column half
    d2 = torch.stack([z.detach()[:, :3] @ z.detach()[:, :3].t(),
                      z.detach()[:, 3:] @ z.detach()[:, 3:].t()], -1)
    torch.testing.assert_close(InnerProductDecoder(heads=2)(z, csr).detach(),
                               d2[rows, csr.col.long()], atol=1e-13, rtol=1e-13)
    loss = recon_loss(z, csr, neg)
    loss.backward()
    zr = z.detach().clone().requires_grad_()
    dr = zr @ zr.t()
    want = -torch.log(torch.sigmoid(dr[rows, csr.col.long()])).mean() \
        - torch.log(1 - torch.sigmoid(dr[nrows, neg.col.long()])).mean()
    want.backward()
    torch.testing.assert_close(loss.detach(), want.detach(), atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(z.grad, zr.grad, atol=1e-12, rtol=1e-12)
    # on a DistGraph without peers: the same scores
    g1 = DistGraph(square_csr(), 30, 0)
    torch.testing.assert_close(dec(z.detach(), g1), dec(z.detach(), csr), atol=0, rtol=0)


def test_negative_pattern():
    csr = small_csr()
    gen = torch.Generator().manual_seed(5)
    neg = negative_pattern(csr, 4, gen)
    deg = csr.degree()
    assert neg.num_rows == csr.num_rows and neg.num_cols == csr.num_cols
    assert torch.equal(neg.degree(), (deg > 0).long() * 4)
    assert int(neg.degree()[3]) == 0  # the empty row stays empty
    assert neg.col.dtype == csr.col.dtype
    assert int(neg.col.min()) >= 0 and int(neg.col.max()) < csr.num_cols
    assert len(set(neg.col.tolist())) > 10  # not one column
    again = negative_pattern(csr, 4, torch.Generator().manual_seed(5))
    assert torch.equal(again.col, neg.col)
    assert negative_pattern(csr, 0).nnz == 0
