"""The contract of the fused dot-product attention kernels with edge features
(csrc/kernels/dot_attn_edge_f32.hip) written out per edge in plain PyTorch, the op's CPU path
with ``edge=``, ``GatPattern.t_slot``, ``relation_edge_order`` and
``CommAwareTransformerConv(edge_dim=)`` (tests/test_dot_attn_edge_gpu.py imports the contract
and its inputs from here).

:func:`dot_attn_edge_contract` takes what the three kernels take — the CSR pattern, ``q``, the
two gathered ``k`` / ``v`` sources, the per-slot edge rows ``ee``, dL/dout, ``scale``,
``beta`` and ``out`` on entry — and returns every array they write, the per-edge gradient
``dee`` and the per-slot weights ``w`` included. It shares no code with ``ops/``. Run in fp64
it is the oracle; run in fp32 it gives the error a faithful fp32 evaluation of the same
formula has, from which the GPU tests derive their bound (``test_gat_kernels.bound``).

Pattern: ``test_gat_kernels.pattern()``; ``q, k, v, g, out0``: ``test_dot_attn.case``; ``ee``
from a generator of its own (std 0.25 at score scale 0.5, std 20 at 40).
"""
from __future__ import annotations

import functools
import math
import types

import pytest
import torch

from test_dot_attn import CIN, ND, NS, SCALES, TOL, _edges, case
from test_gat_kernels import HS, LS, N, PAIRS, R, bound, pattern

OUTPUTS = ("out", "stat_m", "stat_l", "dq", "dk", "dv", "dee", "w")
E = int(pattern()[0][-1])


@functools.lru_cache(maxsize=None)
def edge_rows(C: int, heads: int, s: float) -> torch.Tensor:
    """``ee [E, C]`` for one (C, heads, score scale), fp32 values on the CPU."""
    gen = torch.Generator().manual_seed(9000 * C + 10 * heads + int(s))
    return torch.randn(E, C, generator=gen) * (0.25 if s < 1 else 20.0)


def dot_attn_edge_contract(rowptr, col, q, k, v, k2, v2, nsplit, ee, g, heads, scale, beta,
                           out, c=None, dtype=torch.float64):
    """What dot_attn_edge_fwd / dot_attn_edge_bwd_dst / dot_attn_edge_bwd_src compute, per
    edge, in ``dtype``.

    ``k`` / ``v`` serve columns below ``nsplit`` (all of them without ``k2``), ``k2`` / ``v2``
    the columns from ``nsplit`` on; row ``p`` of ``ee`` belongs to CSR slot ``p``. ``c``
    [rows, heads] is the backward kernels' input (``None``: this evaluation's own
    ``sum_j alpha ga``). Returns out, stat_m, stat_l, c, dq over the destination rows, dk, dv
    over all source rows (``[k rows | k2 rows]``), dee [E, C] and w [E, 2 heads] =
    (alpha | de without scale) over the slots, plus the per-edge ``alpha`` and scores ``e``."""
    cv = lambda t: t.detach().cpu().to(dtype)  # noqa: E731
    rowptr, col = rowptr.cpu().long(), col.cpu().long()
    if k2 is not None:
        ka, va = torch.cat([cv(k)[:nsplit], cv(k2)]), torch.cat([cv(v)[:nsplit], cv(v2)])
    else:
        ka, va = cv(k), cv(v)
    q, g, ee = cv(q), cv(g), cv(ee)
    nr, ns, C = rowptr.numel() - 1, ka.shape[0], ka.shape[1]
    D = C // heads
    rows = torch.repeat_interleave(torch.arange(nr), rowptr[1:] - rowptr[:-1])
    ne = rows.numel()
    qe, ge = q[rows].view(ne, heads, D), g[rows].view(ne, heads, D)
    kk = (ka[col] + ee).view(ne, heads, D)
    vv = (va[col] + ee).view(ne, heads, D)
    e = (qe * kk).sum(-1) * scale                                          # [E, heads]
    m = torch.full((nr, heads), -float("inf"), dtype=dtype).index_reduce(
        0, rows, e, "amax", include_self=True)
    p = torch.exp(e - m[rows])
    den = torch.zeros(nr, heads, dtype=dtype).index_add(0, rows, p)
    inv = torch.where(den > 0, 1.0 / den, torch.zeros_like(den))
    alpha = p * inv[rows]
    agg = torch.zeros(nr, C, dtype=dtype).index_add(
        0, rows, (alpha.unsqueeze(-1) * vv).reshape(ne, C))
    res = {"out": agg if beta == 0 else beta * cv(out) + agg, "stat_m": m, "stat_l": inv}
    ga = (ge * vv).sum(-1)                                                 # [E, heads]
    cc = torch.zeros(nr, heads, dtype=dtype).index_add(0, rows, alpha * ga) if c is None \
        else cv(c)
    de = alpha * (ga - cc[rows])
    res["c"] = cc
    res["dq"] = scale * torch.zeros(nr, C, dtype=dtype).index_add(
        0, rows, (de.unsqueeze(-1) * kk).reshape(ne, C))
    res["dk"] = scale * torch.zeros(ns, C, dtype=dtype).index_add(
        0, col, (de.unsqueeze(-1) * qe).reshape(ne, C))
    res["dv"] = torch.zeros(ns, C, dtype=dtype).index_add(
        0, col, (alpha.unsqueeze(-1) * ge).reshape(ne, C))
    res["dee"] = (alpha.unsqueeze(-1) * ge + scale * de.unsqueeze(-1) * qe).reshape(ne, C)
    res["w"] = torch.cat([alpha, de], 1)
    res["alpha"], res["e"] = alpha, e
    return res


@functools.lru_cache(maxsize=None)
def oracle(C: int, heads: int, s: float, beta: float):
    """(fp64, fp32) results of :func:`dot_attn_edge_contract` on ``case(C, heads, s)`` with
    ``edge_rows(C, heads, s)``."""
    rowptr, col, _ = pattern()
    d = case(C, heads, s)
    args = (rowptr, col, d["q"], d["k"], d["v"], None, None, N, edge_rows(C, heads, s), d["g"],
            heads, d["scale"], beta, d["out0"])
    return dot_attn_edge_contract(*args), dot_attn_edge_contract(*args, dtype=torch.float32)


# ------------------------------------------------------------------------ the contract
def _rowwise_forward(rowptr, col, q, k, v, ee, heads, scale):
    """out_i = sum_j softmax_j(scale <q_i, k_j + ee_p>) (v_j + ee_p) per head, row by row."""
    C = q.shape[1]
    D = C // heads
    outs = []
    for i in range(rowptr.numel() - 1):
        sl = slice(int(rowptr[i]), int(rowptr[i + 1]))
        j = col[sl]
        kk, vv = k[j] + ee[sl], v[j] + ee[sl]
        e = torch.einsum("kd,ekd->ek", q[i].view(heads, D), kk.view(-1, heads, D)) * scale
        a = torch.softmax(e, 0)                                            # [deg, heads]
        outs.append(torch.einsum("ek,ekd->kd", a, vv.view(-1, heads, D)).reshape(C))
    return torch.stack(outs)


@pytest.mark.parametrize("beta", [0.0, 0.5])
@pytest.mark.parametrize("two_sources", [False, True])
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("C,heads", [(64, 1), (64, 8), (128, 4), (256, 2)])
def test_contract_matches_autograd(C, heads, s, two_sources, beta):
    rowptr, col, _ = pattern()
    d = case(C, heads, s)
    q, k, v = (d[n].double().requires_grad_() for n in ("q", "k", "v"))
    ee = edge_rows(C, heads, s).double().requires_grad_()
    g = d["g"].double()
    out = _rowwise_forward(rowptr, col, q, k, v, ee, heads, d["scale"])
    gq, gk, gv, gee = torch.autograd.grad(out, (q, k, v, ee), g)
    if two_sources:
        ref = dot_attn_edge_contract(rowptr, col, d["q"], d["k"][:LS], d["v"][:LS],
                                     d["k"][LS:], d["v"][LS:], LS, ee, g, heads, d["scale"],
                                     beta, d["out0"])
    else:
        ref = dot_attn_edge_contract(rowptr, col, d["q"], d["k"], d["v"], None, None, N, ee, g,
                                     heads, d["scale"], beta, d["out0"])
    torch.testing.assert_close(ref["out"], beta * d["out0"].double() + out.detach(), **TOL)
    torch.testing.assert_close(ref["dq"], gq, **TOL)
    torch.testing.assert_close(ref["dk"], gk, **TOL)
    torch.testing.assert_close(ref["dv"], gv, **TOL)
    torch.testing.assert_close(ref["dee"], gee, **TOL)
    own = ref["out"] - beta * d["out0"].double()
    torch.testing.assert_close(ref["c"], (g * own).view(R, heads, -1).sum(-1), **TOL)
    assert ref["dee"].shape == (E, C) and ref["w"].shape == (E, 2 * heads)
    # the source side from w alone: dv_j = sum alpha g_i, dk_j = scale sum de q_i
    rows = pattern()[2]
    al, de = ref["w"][:, :heads], ref["w"][:, heads:]
    D = C // heads
    dv = torch.zeros(N, C, dtype=torch.float64).index_add(
        0, col, (al.unsqueeze(-1) * g[rows].view(E, heads, D)).reshape(E, C))
    dk = d["scale"] * torch.zeros(N, C, dtype=torch.float64).index_add(
        0, col, (de.unsqueeze(-1) * d["q"].double()[rows].view(E, heads, D)).reshape(E, C))
    torch.testing.assert_close(dv, gv, **TOL)
    torch.testing.assert_close(dk, gk, **TOL)


@pytest.mark.parametrize("C,heads", PAIRS)
def test_input_conditions(C, heads):
    # s = 0.5: every edge carries weight, so one misplaced edge row moves an output by
    # several times the 2e-5 floor
    small = oracle(C, heads, 0.5, 0.0)
    print(f"C={C} heads={heads}: smallest alpha {float(small[0]['alpha'].min()):.3e}")
    assert float(small[0]["alpha"].min()) >= 1e-4
    # s = 40: exp overflows in fp32 unless the row maximum is subtracted
    big = oracle(C, heads, 40.0, 0.0)
    print(f"C={C} heads={heads}: largest score {float(big[0]['e'].max()):.1f}")
    assert float(big[0]["e"].max()) > 89.0
    rowptr = pattern()[0]
    full = rowptr[1:] > rowptr[:-1]  # (an empty row's maximum is -inf)
    for res in (small[0], big[0]):
        for name in OUTPUTS + ("c",):
            t = res[name]
            assert torch.isfinite(t[full] if name == "stat_m" else t).all(), name


def test_t_slot_is_not_the_identity_here():
    from dgraph_amd.ops.gat import GatPattern

    rowptr, col, _ = pattern()
    pat = GatPattern(rowptr, col, LS, HS)
    assert not torch.equal(pat.t_slot.long(), torch.arange(E))


@pytest.mark.parametrize("C,heads", PAIRS)
def test_a_wrong_slot_exceeds_the_bound(C, heads):
    """With ``ee`` rolled by one slot, or not added at all, every row of degree >= 2 of
    ``out`` moves by at least five times the bound the GPU tests allow; empty rows stay."""
    rowptr, col, _ = pattern()
    d = case(C, heads, 0.5)
    ee = edge_rows(C, heads, 0.5)
    r64, r32 = oracle(C, heads, 0.5, 0.0)
    bd = bound(r64["out"], r32["out"])
    deg = rowptr[1:] - rowptr[:-1]
    for wrong_ee in (torch.roll(ee, 1, 0), torch.zeros_like(ee)):
        wrong = dot_attn_edge_contract(rowptr, col, d["q"], d["k"], d["v"], None, None, N,
                                       wrong_ee, d["g"], heads, d["scale"], 0.0, None)
        diff = (wrong["out"] - r64["out"]).abs().amax(1)
        print(f"C={C} heads={heads}: smallest movement / bound "
              f"{float(diff[deg >= 2].min()) / bd:.0f}")
        assert (diff[deg >= 2] >= 5 * bd).all(), (diff[deg >= 2].min(), bd)
        assert (diff[deg == 0] <= 1e-12).all()


# ------------------------------------------------------------------------ the op on the CPU
@pytest.mark.parametrize("two_sources", [False, True])
@pytest.mark.parametrize("C,heads,s", [(64, 2, 0.5), (128, 8, 40.0), (256, 1, 0.5)])
def test_op_cpu_matches_contract(C, heads, s, two_sources):
    from dgraph_amd.ops import dot_attention
    from dgraph_amd.ops.gat import GatPattern

    rowptr, col, _ = pattern()
    d = case(C, heads, s)
    ns, nh = (LS, HS) if two_sources else (N, 0)
    pat = GatPattern(rowptr, col, ns, nh)
    mk = lambda t: t.double().clone().requires_grad_()  # noqa: E731
    q, k, v, ee = mk(d["q"]), mk(d["k"][:ns]), mk(d["v"][:ns]), mk(edge_rows(C, heads, s))
    kh, vh = (mk(d["k"][ns:]), mk(d["v"][ns:])) if two_sources else (None, None)
    out = dot_attention(q, k, v, pat, kh, vh, heads=heads, edge=ee)
    ins = [t for t in (q, k, v, ee, kh, vh) if t is not None]
    grads = torch.autograd.grad(out, ins, d["g"].double())
    ref = oracle(C, heads, s, 0.0)[0]
    torch.testing.assert_close(out.detach(), ref["out"], **TOL)
    torch.testing.assert_close(grads[0], ref["dq"], **TOL)
    torch.testing.assert_close(grads[3], ref["dee"], **TOL)
    if two_sources:
        torch.testing.assert_close(torch.cat([grads[1], grads[4]]), ref["dk"], **TOL)
        torch.testing.assert_close(torch.cat([grads[2], grads[5]]), ref["dv"], **TOL)
    else:
        torch.testing.assert_close(grads[1], ref["dk"], **TOL)
        torch.testing.assert_close(grads[2], ref["dv"], **TOL)
    # fp32 inputs come back as fp32 (evaluated at fp64 inside)
    assert dot_attention(d["q"], d["k"][:ns], d["v"][:ns], pat,
                         None if kh is None else d["k"][ns:],
                         None if vh is None else d["v"][ns:], heads=heads,
                         edge=edge_rows(C, heads, s)).dtype == torch.float32


def _small(two_sources):
    from dgraph_amd.ops.gat import GatPattern

    gen = torch.Generator().manual_seed(3)
    deg = torch.tensor([3, 0, 1, 5, 2, 4, 1])
    rowptr = torch.zeros(8, dtype=torch.long)
    rowptr[1:] = torch.cumsum(deg, 0)
    nl, nh = (5, 3) if two_sources else (8, 0)
    col = torch.randint(0, nl + nh, (int(rowptr[-1]),), generator=gen)
    pat = GatPattern(rowptr, col, nl, nh)
    rn = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64).requires_grad_()  # noqa: E731
    q, k, v = rn(7, 6), rn(nl, 6), rn(nl, 6)
    halo = (rn(nh, 6), rn(nh, 6)) if two_sources else ()
    return pat, (q, k, v) + halo, rn(int(rowptr[-1]), 6)


@pytest.mark.parametrize("two_sources", [False, True])
def test_op_cpu_gradcheck_with_edge(two_sources):
    from dgraph_amd.ops import dot_attention

    pat, ins, ee = _small(two_sources)
    fn = lambda e, *t: dot_attention(t[0], t[1], t[2], pat, *t[3:], scale=0.7, heads=2,  # noqa: E731
                                     edge=e)
    assert torch.autograd.gradcheck(fn, (ee,) + ins)


@pytest.mark.parametrize("two_sources", [False, True])
def test_op_edge_none_is_the_plain_call(two_sources):
    from dgraph_amd.ops import dot_attention

    pat, ins, ee = _small(two_sources)
    a = dot_attention(ins[0], ins[1], ins[2], pat, *ins[3:], scale=0.7, heads=2)
    b = dot_attention(ins[0], ins[1], ins[2], pat, *ins[3:], scale=0.7, heads=2, edge=None)
    assert torch.equal(a, b)
    ga = torch.autograd.grad(a.sum(), ins)
    gb = torch.autograd.grad(b.sum(), ins)
    assert all(torch.equal(x, y) for x, y in zip(ga, gb))
    # and the edge term is not a no-op
    c = dot_attention(ins[0], ins[1], ins[2], pat, *ins[3:], scale=0.7, heads=2, edge=ee)
    assert not torch.allclose(a, c)


def test_op_edge_argument_checks():
    from dgraph_amd.ops import dot_attention

    pat, ins, ee = _small(False)
    with pytest.raises(ValueError):  # one row short
        dot_attention(*ins, pat, heads=2, edge=ee[:-1])
    with pytest.raises(ValueError):  # another width
        dot_attention(*ins, pat, heads=2, edge=ee[:, :4])
    with pytest.raises(ValueError):
        dot_attention(*ins, pat, heads=2, edge=ee.reshape(-1))


# ---------------------------------------------------------------------- GatPattern.t_slot
def test_t_slot_maps_transposed_entries_to_forward_slots():
    from dgraph_amd.ops.gat import GatPattern

    rowptr, col, rows = pattern()
    pat = GatPattern(rowptr, col, LS, HS)
    assert pat._t_slot is None  # built on first use only
    ts = pat.t_slot
    assert ts.dtype == pat.t_col.dtype == torch.int32 and ts.shape == pat.t_col.shape
    assert pat.t_slot is ts
    src = torch.repeat_interleave(torch.arange(N), pat.t_rowptr[1:] - pat.t_rowptr[:-1])
    assert torch.equal(pat.col.long()[ts.long()], src)
    assert torch.equal(rows[ts.long()], pat.t_col.long())
    assert torch.equal(torch.sort(ts.long()).values, torch.arange(E))


# -------------------------------------------------------------------- relation_edge_order
def _dup_edges():
    """A relation's edge list with repeated (src, dst) pairs, in no particular order."""
    g = torch.Generator().manual_seed(11)
    e = torch.stack([torch.randint(0, NS, (70,), generator=g),
                     torch.randint(0, ND, (70,), generator=g)])
    e = torch.cat([e, e[:, 5:25], e[:, 10:15]], 1)
    return e[:, torch.randperm(e.shape[1], generator=g)]


def _check_edge_order(edges, rel, offs, rank):
    from dgraph_amd.data.hetero import relation_edge_order

    order = relation_edge_order(edges, offs, 0, rank)
    assert order.dtype == torch.long and order.shape == (rel.csr.nnz,)
    assert torch.unique(order).numel() == order.numel()
    rows = rel.csr.row_ids().long() + int(offs[0][rank])
    col = rel.csr.col.long()
    Ls = rel.num_local_src
    halo = rel.pattern.halo_vertices.long()
    gcol = torch.where(col < Ls, col + int(offs[1][rank]),
                       halo[(col - Ls).clamp_(min=0)] if halo.numel() else col)
    assert torch.equal(edges[1, order], rows)
    assert torch.equal(edges[0, order], gcol)
    return order


def _edge_order_dist(rank, world, dup):
    from dgraph_amd import Communicator
    from dgraph_amd.data.hetero import build_relation_graph, get_vertex_offsets

    comm = Communicator.init_process_group("nccl")  # gloo underneath on the CPU
    try:
        edges = _dup_edges() if dup else _edges()
        offs = {0: get_vertex_offsets(ND, world), 1: get_vertex_offsets(NS, world)}
        rel = build_relation_graph(edges, 1, 0, offs, rank, world)
        _check_edge_order(edges, rel, offs, rank)
    finally:
        comm.destroy()


@pytest.mark.parametrize("dup", [False, True], ids=["unique", "repeated"])
def test_relation_edge_order_one_rank(dup):
    from dgraph_amd.data.hetero import build_relation_graph, get_vertex_offsets

    edges = _dup_edges() if dup else _edges()
    offs = {0: get_vertex_offsets(ND, 1), 1: get_vertex_offsets(NS, 1)}
    rel = build_relation_graph(edges, 1, 0, offs, 0, 1)
    order = _check_edge_order(edges, rel, offs, 0)
    assert order.numel() == edges.shape[1]
    if dup:  # repeated pairs keep their input order (a stable sort)
        assert torch.unique(edges, dim=1).shape[1] < edges.shape[1]
        key = edges[1, order] * (edges.shape[1] + 1)
        assert bool(((key[1:] > key[:-1]) | (order[1:] > order[:-1])).all())


@pytest.mark.parametrize("world,dup", [(2, True), (3, False), (3, True)])
def test_relation_edge_order_distributed(ranks, world, dup):
    ranks(_edge_order_dist, world, dup)


# ------------------------------------------------------------------------------- the layer
EDIM = 5


def _edge_attr(edges, edim=EDIM, dtype=torch.float64):
    gen = torch.Generator().manual_seed(6)
    return torch.randn(edges.shape[1], edim, generator=gen, dtype=dtype)


def _dense_edge_transformer(layer, x_dst, x_src, edges, edge_attr):
    """Reference formulation: per-edge q / k / v rows with the projected edge row added to
    key and value, softmax per destination. ``edge_attr``: one row per column of ``edges``."""
    H, C = layer.heads, layer.out_channels
    D = C // H
    q = layer.lin_query(x_dst)
    kv = layer.lin_kv(x_src)
    src, dst = edges
    ee = layer.lin_edge(edge_attr)
    k, v = kv[src, :C] + ee, kv[src, C:] + ee
    e = (q[dst].view(-1, H, D) * k.view(-1, H, D)).sum(-1) / math.sqrt(D)
    out = torch.zeros(x_dst.shape[0], C, dtype=x_dst.dtype, device=x_dst.device)
    for i in range(x_dst.shape[0]):
        sel = dst == i
        if sel.any():
            a = torch.softmax(e[sel], 0)  # [deg, H]
            out[i] = (v[sel].view(-1, H, D) * a.unsqueeze(-1)).sum(0).reshape(C)
    return out + layer.lin_skip(x_dst) + layer.bias


def _layer(heads, comm=None, edge_dim=EDIM):
    from dgraph_amd.models.transformer_conv import CommAwareTransformerConv

    torch.manual_seed(0)
    layer = CommAwareTransformerConv(CIN, 8, comm=comm, heads=heads, hetero=True,
                                     edge_dim=edge_dim).double()
    with torch.no_grad():
        layer.bias.normal_()
    return layer


@pytest.mark.parametrize("heads", [1, 2])
def test_layer_matches_dense(heads):
    from dgraph_amd.data.hetero import (build_relation_graph, get_vertex_offsets,
                                        relation_edge_order)

    edges = _edges()
    offs = {0: get_vertex_offsets(ND, 1), 1: get_vertex_offsets(NS, 1)}
    rel = build_relation_graph(edges, 1, 0, offs, 0, 1)
    order = relation_edge_order(edges, offs, 0, 0)
    layer = _layer(heads)
    torch.manual_seed(1)
    xd = torch.randn(ND, CIN, dtype=torch.float64, requires_grad=True)
    xs = torch.randn(NS, CIN, dtype=torch.float64, requires_grad=True)
    ea = _edge_attr(edges).requires_grad_()
    out = layer(xd, rel, x_j=xs, edge_attr=ea[order])
    ref = _dense_edge_transformer(layer, xd, xs, edges, ea)
    torch.testing.assert_close(out, ref)
    w = torch.randn_like(out)
    ins = [xd, xs, ea] + list(layer.parameters())
    assert len(ins) == 3 + 7  # W_q, b_q, W_kv, b_kv, W_edge, W_skip, bias
    ga = torch.autograd.grad((out * w).sum(), ins)
    gb = torch.autograd.grad((ref * w).sum(), ins)
    for a, b in zip(ga, gb):
        assert float(b.abs().max()) > 0
        torch.testing.assert_close(a, b)
    with pytest.raises(ValueError):  # the layer has edge_dim: edge_attr is required
        layer(xd, rel, x_j=xs)


def test_layer_without_edge_dim_is_unchanged():
    from dgraph_amd.models.transformer_conv import CommAwareTransformerConv

    plain = CommAwareTransformerConv(CIN, 8, heads=2, hetero=True)
    none = CommAwareTransformerConv(CIN, 8, heads=2, hetero=True, edge_dim=None)
    keys = ["lin_query.weight", "lin_query.bias", "lin_kv.weight", "lin_kv.bias",
            "lin_skip.weight", "bias"]
    for layer in (plain, none):
        assert len(list(layer.parameters())) == 6
        assert sorted(layer.state_dict().keys()) == sorted(keys)
        assert [n for n, _ in layer.named_modules() if n] == ["lin_query", "lin_kv",
                                                              "lin_skip"]
    with_edge = CommAwareTransformerConv(CIN, 8, heads=2, hetero=True, edge_dim=EDIM)
    assert sorted(with_edge.state_dict().keys()) == sorted(keys + ["lin_edge.weight"])
    assert with_edge.lin_edge.weight.shape == (8, EDIM) and with_edge.lin_edge.bias is None


def test_layer_rejects_overlap_with_edge_dim():
    from dgraph_amd.models.transformer_conv import CommAwareTransformerConv

    with pytest.raises(ValueError):
        CommAwareTransformerConv(CIN, 8, heads=2, hetero=True, overlap=True, edge_dim=EDIM)


def _layer_dist(rank, world, heads, skew):
    import torch.distributed as dist

    from dgraph_amd import Communicator
    from dgraph_amd.comm.alltoallv import CommStats
    from dgraph_amd.data.hetero import (build_relation_graph, get_vertex_offsets,
                                        relation_edge_order)

    comm = Communicator.init_process_group("nccl")  # gloo underneath on the CPU
    try:
        edges = _edges(world if skew else 0)
        offs = {0: get_vertex_offsets(ND, world), 1: get_vertex_offsets(NS, world)}
        rel = build_relation_graph(edges, 1, 0, offs, rank, world)
        order = relation_edge_order(edges, offs, 0, rank)
        gen = torch.Generator().manual_seed(1)
        xd = torch.randn(ND, CIN, generator=gen, dtype=torch.float64)
        xs = torch.randn(NS, CIN, generator=gen, dtype=torch.float64)
        w = torch.randn(ND, 8, generator=gen, dtype=torch.float64)
        ea = _edge_attr(edges)
        d0, d1 = int(offs[0][rank]), int(offs[0][rank + 1])
        s0, s1 = int(offs[1][rank]), int(offs[1][rank + 1])
        layer = _layer(heads, comm)
        xdl = xd[d0:d1].clone().requires_grad_()
        xsl = xs[s0:s1].clone().requires_grad_()
        eal = ea[order].clone().requires_grad_()
        CommStats.reset()
        out = layer(xdl, rel, x_j=xsl, edge_attr=eal)
        assert CommStats.calls == 1, CommStats.calls   # one exchange of the [k | v] rows
        (out * w[d0:d1]).sum().backward()
        assert CommStats.calls == 2, CommStats.calls   # and its adjoint: edge rows stay home
        got = [p.grad.clone() for p in layer.parameters()]
        assert len(got) == 7
        for t in got:
            dist.all_reduce(t)
        # the same layer at W = 1 on the whole graph, in this process
        one = _layer(heads, types.SimpleNamespace(get_world_size=lambda: 1))
        offs1 = {0: get_vertex_offsets(ND, 1), 1: get_vertex_offsets(NS, 1)}
        rel1 = build_relation_graph(edges, 1, 0, offs1, 0, 1)
        order1 = relation_edge_order(edges, offs1, 0, 0)
        xd1, xs1 = xd.clone().requires_grad_(), xs.clone().requires_grad_()
        ea1 = ea.clone().requires_grad_()
        ref = one(xd1, rel1, x_j=xs1, edge_attr=ea1[order1])
        assert CommStats.calls == 2
        (ref * w).sum().backward()
        torch.testing.assert_close(out.detach(), ref.detach()[d0:d1])
        torch.testing.assert_close(xdl.grad, xd1.grad[d0:d1])
        torch.testing.assert_close(xsl.grad, xs1.grad[s0:s1])
        torch.testing.assert_close(eal.grad, ea1.grad[order])
        for a, p in zip(got, one.parameters()):
            torch.testing.assert_close(a, p.grad)
    finally:
        comm.destroy()


@pytest.mark.parametrize("world,heads,skew", [(2, 2, False), (3, 1, False), (2, 1, True),
                                              (3, 2, True)])
def test_layer_distributed(ranks, world, heads, skew):
    ranks(_layer_dist, world, heads, skew)
