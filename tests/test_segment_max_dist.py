"""Distributed max aggregation on gloo: W ranks against W = 1 (forward rows bitwise, the
gradient at 1e-5), a plan where one rank sends but has no halo rows, and a GraphSAGE
(aggr="max") training curve across world sizes."""
import pytest
import torch

from dgraph_amd.data.synthetic import SHAPES, build_partition, node_data
from dgraph_amd.models.sage import GraphSAGE
from dgraph_amd.ops.aggregate import aggregate
from dgraph_amd.ops.csr import CSR
from dgraph_amd.parallel.dist_graph import DistGraph, dist_aggregate

SHAPE = SHAPES["ogbn-arxiv"].scaled(0.01)
F = 16
X_SEED = 3  # a seed at which no two distinct sources tie for a row's maximum (asserted)


def _global_inputs(device="cpu"):
    g = torch.Generator().manual_seed(X_SEED)
    x = torch.randn(SHAPE.num_nodes, F, generator=g)
    gy = torch.randn(SHAPE.num_nodes, F, generator=g)
    return x.to(device), gy.to(device)


def _single_rank_reference(device="cpu"):
    """W = 1 forward and gradient; asserts that every non-empty (row, f) has its maximum
    attained by ONE distinct source, so the gradient's assignment is partition-independent
    (the slot order within a row differs between partitions)."""
    p = build_partition(SHAPE, 0, 1, device)
    csr = p["csr"]
    x, gy = _global_inputs(device)
    x.requires_grad_()
    g1 = DistGraph(csr, p["L"], 0, symmetric=True)
    out = dist_aggregate(x, g1, reduce="max")
    out.backward(gy)
    rows = csr.row_ids()
    col = csr.col.long()
    best = x.detach()[col] == out.detach()[rows]
    idx = rows.unsqueeze(1).expand(-1, F)
    cc = col.unsqueeze(1).expand(-1, F)
    lo = torch.full((p["L"], F), 2**62, dtype=torch.long, device=x.device)
    hi = torch.full((p["L"], F), -1, dtype=torch.long, device=x.device)
    lo.scatter_reduce_(0, idx, torch.where(best, cc, 2**62), "amin")
    hi.scatter_reduce_(0, idx, torch.where(best, cc, -1), "amax")
    nonempty = (csr.degree() > 0).unsqueeze(1).expand(-1, F)
    assert torch.equal(lo[nonempty], hi[nonempty]), "distinct sources tie: pick another seed"
    return out.detach(), x.grad


def _dist_max_body(rank, world, device="cpu"):
    ref_out, ref_gx = _single_rank_reference(device)
    p = build_partition(SHAPE, rank, world, device)
    g = DistGraph(p["csr"], p["L"], p["H"], p["send_local_idx"], p["send_splits"],
                  p["recv_splits"])
    lo, hi = p["offsets"][rank], p["offsets"][rank + 1]
    x, gy = _global_inputs(device)
    xl = x[lo:hi].clone().requires_grad_()
    e0 = g.edges_aggregated
    out = dist_aggregate(xl, g, reduce="max")
    out.backward(gy[lo:hi])
    assert torch.equal(out.detach(), ref_out[lo:hi])
    torch.testing.assert_close(xl.grad, ref_gx[lo:hi], atol=1e-5, rtol=1e-5)
    assert g.edges_aggregated - e0 == 2 * g.nnz
    # the default path is untouched by the new argument
    assert torch.equal(dist_aggregate(xl, g), dist_aggregate(xl, g, True, None))


@pytest.mark.parametrize("world", [2, 3])
def test_dist_max_matches_single_rank(ranks, world):
    ranks(_dist_max_body, world)


def _sends_without_halo_body(rank, world):
    """Rank 0 owns vertices 0-2 and reads only those; rank 1 owns 3-4 and reads vertices 0
    and 2 of rank 0: rank 0 has sends and H == 0, and must still post both exchanges."""
    grow = torch.tensor([0, 0, 1, 2, 3, 3, 3, 4, 4])
    gcol = torch.tensor([1, 2, 0, 0, 0, 4, 2, 2, 3])
    gcsr = CSR.from_coo(grow, gcol, 5, 5)
    x = torch.tensor([[0.5, -1.0], [2.0, 0.25], [-3.0, 4.0], [1.5, -2.5], [0.75, 3.5]])
    gy = torch.tensor([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0], [7.0, 8.0], [9.0, 10.0]])
    xg = x.clone().requires_grad_()
    ref = aggregate(xg, gcsr, reduce="max")
    ref.backward(gy)
    if rank == 0:
        csr = CSR.from_coo(torch.tensor([0, 0, 1, 2]), torch.tensor([1, 2, 0, 0]), 3, 3)
        g = DistGraph(csr, 3, 0, torch.tensor([0, 2], dtype=torch.int32), [0, 2], [0, 0])
        assert g.halo is not None and g.H == 0
        sl = slice(0, 3)
    else:
        # local columns: 0, 1 = vertices 3, 4; halo columns 2, 3 = vertices 0, 2
        csr = CSR.from_coo(torch.tensor([0, 0, 0, 1, 1]), torch.tensor([2, 1, 3, 3, 0]), 2, 4)
        g = DistGraph(csr, 2, 2, torch.zeros(0, dtype=torch.int32), [0, 0], [2, 0])
        sl = slice(3, 5)
    xl = x[sl].clone().requires_grad_()
    out = dist_aggregate(xl, g, reduce="max")
    out.backward(gy[sl])
    assert torch.equal(out.detach(), ref.detach()[sl])
    assert torch.equal(xl.grad, xg.grad[sl])


def test_rank_with_sends_and_no_halo_rows(ranks):
    ranks(_sends_without_halo_body, 2)


def _train_losses(rank, world, steps, out):
    import torch.distributed as dist

    from dgraph_amd.parallel.grad_sync import GradSync

    p = build_partition(SHAPE, rank, world, "cpu")
    g = DistGraph(p["csr"], p["L"], p["H"], p["send_local_idx"], p["send_splits"],
                  p["recv_splits"], symmetric=(world == 1))
    x, y, tr = node_data(SHAPE, rank, p["offsets"], "cpu", dtype=torch.float32)
    idx = torch.nonzero(tr).squeeze(1)
    n = torch.tensor([idx.numel()])
    if world > 1:
        dist.all_reduce(n)
    torch.manual_seed(0)
    m = GraphSAGE(SHAPE.num_features, 32, SHAPE.num_classes, 3, aggr="max")
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    sync = GradSync(m.parameters())
    losses = []
    for _ in range(steps):
        logits = m(x, g, out_rows=idx)
        loss = torch.nn.functional.cross_entropy(logits, y[idx], reduction="sum") / n.item()
        loss.backward()
        sync.all_reduce()
        opt.step()
        opt.zero_grad()
        lt = loss.detach().clone()
        if world > 1:
            dist.all_reduce(lt)
        losses.append(float(lt))
    if rank == 0:
        torch.save(torch.tensor(losses), out)


def test_max_training_curve_matches_single_rank(ranks, tmp_path):
    """4 steps of GraphSAGE(aggr="max") at W = 2 follow the W = 1 loss curve. Hidden
    activations tie at exactly 0 after ReLU; such a tie routes gradient to units whose ReLU
    derivative is 0, so the choice among them cannot change the curve."""
    _train_losses(0, 1, 4, tmp_path / "w1.pt")
    ranks(_train_losses, 2, 4, str(tmp_path / "wn.pt"))
    a = torch.load(tmp_path / "w1.pt", weights_only=True)
    b = torch.load(tmp_path / "wn.pt", weights_only=True)
    torch.testing.assert_close(a, b, atol=1e-5, rtol=1e-5)
