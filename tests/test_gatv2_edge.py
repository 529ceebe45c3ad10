"""GATv2 attention with edge features on the CPU: the dense per-edge reference of
csrc/kernels/gatv2_edge_f32.hip (the fp64 oracle of tests/test_gatv2_edge_gpu.py, and at fp32
the source of its bound), its input conditions, ``gatv2_attention(..., edge=)`` and
``CommAwareGATv2Conv(edge_dim=)``. Pattern: ``test_gat_kernels.pattern()``; ``l, r, g, a``:
``test_gatv2.case``; ``ee``: a seeded generator of its own times ``EE_STD``."""
from __future__ import annotations

import functools
import types

import pytest
import torch
import torch.nn.functional as F

from test_dot_attn import CIN, ND, NS, _edges
from test_dot_attn_edge import _edge_attr
from test_gat_kernels import HS, LS, N, PAIRS, R, pattern
from test_gatv2 import SCALES, SLOPE, case

E = int(pattern()[0][-1])
EE_STD = 0.25
EDIM = 7
TOL = dict(atol=1e-10, rtol=1e-10)


@functools.lru_cache(maxsize=None)
def edge_rows(C: int, heads: int, s: float) -> torch.Tensor:
    """``ee [E, C]`` for one (C, heads, score scale), fp32 values on the CPU."""
    gen = torch.Generator().manual_seed(7000 * C + 10 * heads + int(s))
    return torch.randn(E, C, generator=gen) * EE_STD


def dense_reference(l, r, ee, att, g, heads, slope, dtype=torch.float64):
    """The edge kernels' contract on ``pattern()``, dense per edge in ``dtype``: out, alpha
    (= w), stat_m, stat_l, c and, through autograd, dl, dr, dee, da (plus e and pre)."""
    rowptr, col, rows = pattern()
    l, r, ee, att = (t.detach().to(dtype).requires_grad_() for t in (l, r, ee, att.reshape(-1)))
    g = g.to(dtype)
    C = l.shape[1]
    D = C // heads
    pre = (l[rows] + r[col]) + ee
    e = (att * F.leaky_relu(pre, slope)).view(E, heads, D).sum(-1)
    m = torch.full((R, heads), -float("inf"), dtype=dtype).index_reduce(
        0, rows, e.detach(), "amax", include_self=True)
    p = torch.exp(e - m[rows])
    den = torch.zeros(R, heads, dtype=dtype).index_add(0, rows, p)
    alpha = p / den[rows]
    msg = (r[col].view(E, heads, D) * alpha.unsqueeze(-1)).reshape(E, C)
    out = torch.zeros(R, C, dtype=dtype).index_add(0, rows, msg)
    dl, dr, dee, da = torch.autograd.grad(out, (l, r, ee, att), g)
    inv = torch.where(den > 0, 1.0 / den, torch.zeros_like(den)).detach()
    out = out.detach()
    return dict(out=out, alpha=alpha.detach(), stat_m=m, stat_l=inv, dl=dl, dr=dr, dee=dee,
                da=da, c=(g * out).view(R, heads, D).sum(-1), e=e.detach(), pre=pre.detach())


@functools.lru_cache(maxsize=None)
def oracle(C: int, heads: int, s: float):
    """(fp64, fp32) :func:`dense_reference` on ``case(C, heads, s)`` + ``edge_rows``."""
    d = case(C, heads, s)
    args = (d["l"], d["r"], edge_rows(C, heads, s), d["a"], d["g"], heads, SLOPE)
    return dense_reference(*args), dense_reference(*args, dtype=torch.float32)


@pytest.mark.parametrize("C,heads", PAIRS)
def test_input_conditions(C, heads):
    from dgraph_amd.ops.gat import GatPattern

    small, big = oracle(C, heads, SCALES[0]), oracle(C, heads, SCALES[1])
    for r64, r32 in (small, big):  # pre is two fp32 adds: the same LeakyReLU branch all the same
        assert torch.equal(r64["pre"] > 0, r32["pre"] > 0)
    assert float(small[0]["alpha"].min()) >= 1e-4  # one wrong slot moves an output visibly
    assert float(big[0]["e"].max()) > 89.0         # exp needs the maximum subtracted
    rowptr, col, _ = pattern()
    assert not torch.equal(GatPattern(rowptr, col, LS, HS).t_slot.long(), torch.arange(E))


def _op(d, ee, heads, ns, nh, dtype=torch.float64, dev="cpu", pat=None, halves=False, **kw):
    """``gatv2_attention`` forward + gradients on ``pat = (rowptr, col)`` (``pattern()``) with
    ``ns`` local and ``nh`` halo sources: out, dl, dr (local | halo), da, dee. ``halves``:
    ``xd`` / ``xs`` are the column halves of one [ns, 2C] leaf."""
    from dgraph_amd.ops import gatv2_attention
    from dgraph_amd.ops.gat import GatPattern

    rowptr, col = pat or pattern()[:2]
    nq, C = rowptr.numel() - 1, d["C"]
    mk = lambda t: t.to(dev, dtype).clone().requires_grad_()  # noqa: E731
    a, rh = mk(d["a"].view(heads, -1)), mk(d["r"][ns:ns + nh]) if nh else None
    if halves:
        lr = mk(torch.cat([torch.cat([d["l"], d["r"][nq:ns]]), d["r"][:ns]], 1))
        ins, l, r = [lr, a], lr[:nq, :C], lr[:, C:]
    else:
        l, r = mk(d["l"][:nq]), mk(d["r"][:ns])
        ins = [l, r, a] + ([rh] if nh else [])
    if ee is not None:
        kw["edge"] = mk(ee[:col.numel()])
        ins.append(kw["edge"])
    out = gatv2_attention(l, r, a, GatPattern(rowptr.to(dev), col.to(dev), ns, nh), rh,
                          heads=heads, **kw)
    gr = list(torch.autograd.grad(out, ins, d["g"][:nq].to(dev, dtype)))
    if halves:
        gr = [gr[0][:nq, :C], gr[0][:, C:]] + gr[1:]
    res = {"out": out.detach(), "dl": gr[0], "da": gr[2].reshape(-1),
           "dr": torch.cat([gr[1], gr[3]]) if nh else gr[1]}
    if ee is not None:
        res["dee"] = gr[-1]
    return res


@pytest.mark.parametrize("ns,nh", [(N, 0), (LS, HS)])
@pytest.mark.parametrize("C,heads,s", [(64, 2, 0.5), (128, 8, 40.0), (256, 1, 0.5)])
def test_op_cpu_matches_dense_reference(C, heads, s, ns, nh):
    got = _op(case(C, heads, s), edge_rows(C, heads, s), heads, ns, nh)
    for k in got:
        torch.testing.assert_close(got[k], oracle(C, heads, s)[0][k], **TOL)


def test_op_edge_none_is_the_plain_call_and_bad_edges_raise():
    from dgraph_amd.ops import gatv2_attention
    from dgraph_amd.ops.gat import GatPattern

    d, ee = case(64, 2, 0.5), edge_rows(64, 2, 0.5)
    a, b = _op(d, None, 2, LS, HS), _op(d, None, 2, LS, HS, edge=None)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.allclose(a["out"], _op(d, ee, 2, LS, HS)["out"])
    pat = GatPattern(*pattern()[:2], N, 0)
    for bad in (ee[:-1], ee[:, :32], ee.reshape(-1)):
        with pytest.raises(ValueError, match="edge must be"):
            gatv2_attention(d["l"], d["r"], d["a"], pat, heads=2, edge=bad)


# ------------------------------------------------------------------------------- the layer
def dense_edge_gatv2(layer, x_dst, x_src, edges, edge_attr):
    """PyG's formula per edge: ``edge_attr`` has one row per column of ``edges``."""
    H, C = layer.heads, layer.out_channels
    l, r = layer.lin_dst(x_dst), layer.lin_src(x_src)
    src, dst = edges
    pre = l[dst] + r[src] + layer.lin_edge(edge_attr)
    e = (F.leaky_relu(pre, layer.negative_slope).view(-1, H, C // H) * layer.att).sum(-1)
    out = torch.zeros(x_dst.shape[0], C, dtype=x_dst.dtype, device=x_dst.device)
    for i in dst.unique():
        sel = dst == i
        a = torch.softmax(e[sel], 0)  # [deg, H]
        out[i] = (r[src[sel]].view(-1, H, C // H) * a.unsqueeze(-1)).sum(0).reshape(C)
    return out + layer.res_net(x_dst) + layer.bias


def _layer_run(heads, rank=0, world=1, comm=None, dev="cpu", dtype=torch.float64, cout=8,
               dense=False):
    """``CommAwareGATv2Conv(CIN, cout, residual, hetero, edge_dim=EDIM)`` on one rank's part of
    the graph (``dense``: :func:`dense_edge_gatv2` instead, W = 1) -> the layer, [out, dx,
    dx_j, dedge_attr scattered to the order of ``edges``, parameter gradients], min |pre|."""
    from dgraph_amd.data.hetero import (build_relation_graph, get_vertex_offsets,
                                        relation_edge_order)
    from dgraph_amd.models import CommAwareGATv2Conv

    edges = _edges()
    offs = {0: get_vertex_offsets(ND, world), 1: get_vertex_offsets(NS, world)}
    order = relation_edge_order(edges, offs, 0, rank)
    gen = torch.Generator().manual_seed(1)
    xd, xs, w = (torch.randn(n, c, generator=gen) for n, c in ((ND, CIN), (NS, CIN), (ND, cout)))
    (d0, d1), (s0, s1) = ((int(offs[t][rank]), int(offs[t][rank + 1])) for t in (0, 1))
    torch.manual_seed(0)
    layer = CommAwareGATv2Conv(CIN, cout, comm=comm, heads=heads, residual=True, hetero=True,
                               edge_dim=EDIM)
    with torch.no_grad():
        layer.bias.normal_()
    layer = layer.to(dev, dtype)
    ea = _edge_attr(edges, EDIM, torch.float32)
    x, xj, e = (t.to(dev, dtype).requires_grad_() for t in (xd[d0:d1], xs[s0:s1], ea[order]))
    if dense:
        out = dense_edge_gatv2(layer, x, xj, edges[:, order].to(dev), e)
    else:
        rel = build_relation_graph(edges, 1, 0, offs, rank, world).to(dev)
        out = layer(x, rel, x_j=xj, edge_attr=e)
    gr = list(torch.autograd.grad(out, [x, xj, e] + list(layer.parameters()),
                                  w[d0:d1].to(dev, dtype)))
    gr[2] = torch.zeros(edges.shape[1], EDIM, dtype=dtype, device=dev).index_copy(
        0, order.to(dev), gr[2])
    with torch.no_grad():
        pre = layer.lin_edge(e)
        if world == 1:
            pre = pre + layer.lin_dst(x)[edges[1, order]] + layer.lin_src(xj)[edges[0, order]]
    return layer, [out.detach()] + gr, float(pre.abs().min())


@pytest.mark.parametrize("heads", [1, 2])
def test_layer_matches_dense(heads):
    layer, got, _ = _layer_run(heads)
    assert len(got) == 4 + 8 and layer.lin_edge.weight.shape == (8, EDIM)
    for a, b in zip(got, _layer_run(heads, dense=True)[1]):
        assert float(b.abs().max()) > 0
        torch.testing.assert_close(a, b)


def test_layer_without_edge_dim_is_unchanged_and_mismatches_raise():
    """(The layer's output without ``edge_dim``: tests/test_gatv2.py, untouched.)"""
    from dgraph_amd.models import CommAwareGATv2Conv

    plain, layer = CommAwareGATv2Conv(CIN, 8, heads=2, residual=True), _layer_run(2)[0]
    keys = ["lin_src.weight", "lin_src.bias", "lin_dst.weight", "lin_dst.bias", "att",
            "res_net.weight", "bias"]
    assert sorted(plain.state_dict()) == sorted(keys) and not hasattr(plain, "lin_edge")
    assert sorted(layer.state_dict()) == sorted(keys + ["lin_edge.weight"])
    x = torch.randn(ND, CIN)
    with pytest.raises(ValueError, match="edge_attr"):
        plain(x, None, edge_attr=torch.randn(3, EDIM))
    with pytest.raises(ValueError, match="edge_attr"):  # the layer has edge_dim
        layer(x.double(), None)


def _layer_dist(rank, world, heads):
    import torch.distributed as dist

    from dgraph_amd import Communicator
    from dgraph_amd.data.hetero import get_vertex_offsets

    comm = Communicator.init_process_group("nccl")  # gloo underneath on the CPU
    try:
        got = _layer_run(heads, rank, world, comm)[1]
        for t in got[3:]:  # each edge row's gradient comes from its destination's rank alone
            dist.all_reduce(t)
        ref = _layer_run(heads, comm=types.SimpleNamespace(get_world_size=lambda: 1))[1]
        (d0, d1), (s0, s1) = (get_vertex_offsets(n, world)[rank:rank + 2].tolist()
                              for n in (ND, NS))
        for a, b in zip(got, [ref[0][d0:d1], ref[1][d0:d1], ref[2][s0:s1]] + ref[3:]):
            torch.testing.assert_close(a, b)
    finally:
        comm.destroy()


def test_layer_distributed_needs_only_rank_local_edge_rows(ranks):
    ranks(_layer_dist, 2, 2)
