"""The layer-0 input aggregate handed from a step's backward to the next step's forward
through layer 0's output buffer (``ExecutorConfig.reuse_agg0``): bitwise the step that
aggregates the input in every forward, over several optimizer steps, on one rank and
vertex-partitioned over two gloo ranks (resident and streamed halos); which shapes take
it; invalidation; the aggregated-edge count."""
import pytest
import torch
import torch.distributed as dist

from dgraph_amd.data.synthetic import (SHAPES, SPLIT_TEST, SPLIT_TRAIN, SPLIT_VALID,
                                       GraphShape, build_partition, contiguous_offsets,
                                       node_data)
from dgraph_amd.models.sage import GraphSAGE
from dgraph_amd.models.sage_fused import FusedSAGE
from dgraph_amd.parallel.dist_graph import DistGraph
from dgraph_amd.utils.config import ExecutorConfig

SCALE = 2e-5  # the tiny graph of test_sage_fused.py: ~2.2K vertices, ~65K messages
STEPS = 3


def _executor(rank, world, reuse, dev="cpu", hidden=256, feat=None, **knobs):
    """A fresh model (seed 0) and its executor on the tiny graph, ``keep_agg0`` off."""
    shape = SHAPES["ogbn-papers100M"].scaled(SCALE)
    if feat is not None:
        shape = GraphShape("w", shape.num_nodes, shape.num_directed_edges, feat, 40, 0.3,
                           0.1, 0.1)
    part = build_partition(shape, rank, world, dev, global_frac=0.3, window=64)
    csr = part["csr"]
    if world == 1:
        csr.num_cols = part["L"]
    group = dist.group.WORLD if world > 1 else None
    g = DistGraph(csr, part["L"], part["H"], part["send_local_idx"], part["send_splits"],
                  part["recv_splits"], group, symmetric=True)
    offs = contiguous_offsets(shape.num_nodes, world)
    x, y, split = node_data(shape, rank, offs, dev, dtype=torch.float32, return_split=True)
    tr = torch.nonzero(split == SPLIT_TRAIN).reshape(-1)
    ev = torch.nonzero((split == SPLIT_VALID) | (split == SPLIT_TEST)).reshape(-1)
    n_tr = torch.tensor([tr.numel()])
    if world > 1:
        dist.all_reduce(n_tr)
    torch.manual_seed(0)
    model = GraphSAGE(shape.num_features, hidden, shape.num_classes, 3).to(dev)
    cfg = ExecutorConfig(keep_agg0="off", reuse_agg0=reuse, **knobs)
    ex = FusedSAGE(model, g, x, tr, y[tr], ev, y[ev], split[ev] == SPLIT_VALID, int(n_tr),
                   chunk_rows=300, config=cfg)
    return ex, model, g


def _train(ex, model, g, world=1, steps=STEPS, invalidate_before=()):
    """``steps`` training steps (SGD on the all-reduced gradients); per step the loss, every
    gradient, the hits and the edges the step aggregated."""
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    out = []
    for i in range(steps):
        if i in invalidate_before:
            ex.invalidate_input_aggregate()
        e0 = g.edges_aggregated
        loss = ex.step().clone()
        edges = g.edges_aggregated - e0
        grads = [p.grad.clone() for p in model.parameters()]
        out.append((loss, grads, ex.correct.clone(), edges))
        if world > 1:
            for p in model.parameters():
                dist.all_reduce(p.grad)
        opt.step()
    return out


def _assert_same_steps(a, b):
    assert len(a) == len(b)
    for (la, ga, ca, _), (lb, gb, cb, _) in zip(a, b):
        assert torch.equal(la, lb)
        assert len(ga) == len(gb)
        for x, y in zip(ga, gb):
            assert torch.equal(x, y)
        assert torch.equal(ca, cb)


def _on_off(rank, world, dev="cpu", **kw):
    res = {}
    for reuse in ("auto", "off"):
        ex, model, g = _executor(rank, world, reuse, dev=dev, **kw)
        res[reuse] = (_train(ex, model, g, world), ex)
    return res


def test_reuse_agg0_bitwise_w1():
    res = _on_off(0, 1)
    (on, ex_on), (off, ex_off) = res["auto"], res["off"]
    assert ex_on.schedule["keep_agg0"] is False and ex_off.schedule["keep_agg0"] is False
    assert ex_on.schedule["reuse_agg0"] is True and ex_off.schedule["reuse_agg0"] is False
    _assert_same_steps(on, off)
    # more than one chunk ran, and the gradients moved the weights between the steps
    assert len(ex_on.chunks) > 1
    assert not torch.equal(on[0][0], on[1][0])
    # from the second step on, one full input aggregation less per step
    nnz = ex_on.nnz_it + ex_on.nnz_h
    assert nnz > 0
    assert on[0][3] == off[0][3]
    for k in range(1, STEPS):
        assert off[k][3] == off[0][3]
        assert on[k][3] == off[k][3] - nnz


def _w2_body(rank, world, stream):
    knobs = dict(halo_stream="on" if stream else "off")
    res = {}
    for reuse in ("auto", "off"):
        ex, model, g = _executor(rank, world, reuse, **knobs)
        assert ex.stream == stream
        assert ex.schedule["reuse_agg0"] is (reuse == "auto")
        res[reuse] = _train(ex, model, g, world)
    _assert_same_steps(res["auto"], res["off"])
    nnz = ex.nnz_it + ex.nnz_h
    assert res["auto"][1][3] == res["off"][1][3] - nnz


@pytest.mark.parametrize("stream", [False, True])
def test_reuse_agg0_bitwise_w2(ranks, stream):
    ranks(_w2_body, 2, stream)


def test_reuse_agg0_eligibility_by_width():
    """d0 == hidden (100 features padded to 128, hidden 128) takes the reuse; d0 > hidden
    (300 features padded to 320, hidden 256) has no room in layer 0's rows and does not."""
    res = _on_off(0, 1, hidden=128, feat=100)
    (on, ex_on), (off, _) = res["auto"], res["off"]
    assert ex_on.d0 == 128 == ex_on.hid and ex_on.schedule["reuse_agg0"] is True
    _assert_same_steps(on, off)
    nnz = ex_on.nnz_it + ex_on.nnz_h
    assert on[1][3] == off[1][3] - nnz
    ex, model, g = _executor(0, 1, "auto", hidden=256, feat=300)
    assert ex.d0 > ex.hid and ex.schedule["reuse_agg0"] is False
    wide = _train(ex, model, g)
    assert wide[1][3] == wide[0][3]
    # a kept agg0 (the plan had room) leaves nothing to reuse
    shape = SHAPES["ogbn-papers100M"].scaled(SCALE)
    part = build_partition(shape, 0, 1, "cpu", global_frac=0.3, window=64)
    part["csr"].num_cols = part["L"]
    gk = DistGraph(part["csr"], part["L"], 0, symmetric=True)
    xk, yk, sk = node_data(shape, 0, contiguous_offsets(shape.num_nodes, 1), "cpu",
                           dtype=torch.float32, return_split=True)
    tr = torch.nonzero(sk == SPLIT_TRAIN).reshape(-1)
    ev = torch.nonzero((sk == SPLIT_VALID) | (sk == SPLIT_TEST)).reshape(-1)
    mk = GraphSAGE(shape.num_features, 256, shape.num_classes, 3)
    exk = FusedSAGE(mk, gk, xk, tr, yk[tr], ev, yk[ev], sk[ev] == SPLIT_VALID, tr.numel(),
                    chunk_rows=300, config=ExecutorConfig(keep_agg0="on"))
    assert exk.schedule["keep_agg0"] is True and exk.schedule["reuse_agg0"] is False


def test_invalidate_input_aggregate():
    """After an invalidation the next step aggregates the input in its forward again (the
    full edge count), with the results of the uninterrupted run."""
    ex, model, g = _executor(0, 1, "auto")
    plain = _train(ex, model, g)
    ex2, model2, g2 = _executor(0, 1, "auto")
    inv = _train(ex2, model2, g2, invalidate_before=(1,))
    _assert_same_steps(plain, inv)
    nnz = ex.nnz_it + ex.nnz_h
    assert inv[1][3] == inv[0][3] and inv[2][3] == inv[0][3] - nnz
    assert plain[1][3] == plain[0][3] - nnz


def test_reuse_agg0_config_env(monkeypatch):
    monkeypatch.setenv("DGRAPH_FUSED_REUSE_AGG0", "off")
    assert ExecutorConfig.from_env().reuse_agg0 == "off"
    monkeypatch.delenv("DGRAPH_FUSED_REUSE_AGG0")
    assert ExecutorConfig.from_env().reuse_agg0 == "auto"
    with pytest.raises(ValueError):
        ExecutorConfig(reuse_agg0="on")
