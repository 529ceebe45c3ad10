"""The contract of the fused dot-product attention kernels (csrc/kernels/dot_attn_f32.hip)
written out per edge in plain PyTorch, the op's CPU path and the ``CommAwareTransformerConv``
layer (tests/test_dot_attn_gpu.py imports the contract and its inputs from here).

:func:`dot_attn_contract` takes exactly what the three kernels take — the CSR pattern, ``q``,
the two gathered ``k`` / ``v`` sources, dL/dout, ``scale``, ``beta`` and ``out`` on entry —
and returns every array they write. It shares no code with ``ops/dot_attn.py``. Run in fp64
it is the oracle; run in fp32 it gives the error a faithful fp32 evaluation of the same
formula has, from which the GPU tests derive their bound (``test_gat_kernels.bound``).

The pattern is ``test_gat_kernels.pattern()`` (37 rows over 41 local + 19 halo sources,
degrees 0, 1, LPR +- 1 and a 301-entry hub; its conditions are asserted there). Inputs at
score scale 0.5 (every edge carries at least 1e-4 of its row) and 40 (``exp`` overflows in
fp32 unless the row maximum is subtracted).
"""
from __future__ import annotations

import functools
import math
import types

import pytest
import torch

from test_gat_kernels import HS, LS, N, PAIRS, R, bound, pattern

SCALES = [0.5, 40.0]
OUTPUTS = ("out", "stat_m", "stat_l", "dq", "dk", "dv")
TOL = dict(atol=1e-10, rtol=1e-10)


@functools.lru_cache(maxsize=None)
def case(C: int, heads: int, s: float):
    """The kernels' inputs for one (C, heads, score scale), fp32 values on the CPU: k and v
    over all N sources (the tests split them at LS)."""
    gen = torch.Generator().manual_seed(7000 * C + 10 * heads + int(s))
    rn = lambda *shape: torch.randn(*shape, generator=gen)  # noqa: E731
    q, k = rn(R, C), rn(N, C) * s
    return dict(C=C, heads=heads, q=q, k=k, v=rn(N, C), g=rn(R, C), out0=rn(R, C),
                scale=1.0 / math.sqrt(C // heads))


def dot_attn_contract(rowptr, col, q, k, v, k2, v2, nsplit, g, heads, scale, beta, out,
                      c=None, dtype=torch.float64, perm=None):
    """What dot_attn_fwd / dot_attn_bwd_dst / dot_attn_bwd_src compute, per edge, in
    ``dtype``.

    ``k`` / ``v`` serve columns below ``nsplit`` (all of them without ``k2``), ``k2`` / ``v2``
    the columns from ``nsplit`` on. ``c`` [rows, heads] is the backward kernels' input
    (``None``: this evaluation's own ``sum_j alpha ga``). ``perm``: the order in which the D
    products of a score are summed. Returns out, stat_m, stat_l, c, dq over the destination
    rows and dk, dv over all source rows (``[k rows | k2 rows]``), plus the per-edge
    ``alpha`` and scores ``e``."""
    cv = lambda t: t.detach().cpu().to(dtype)  # noqa: E731
    rowptr, col = rowptr.cpu().long(), col.cpu().long()
    if k2 is not None:
        ka, va = torch.cat([cv(k)[:nsplit], cv(k2)]), torch.cat([cv(v)[:nsplit], cv(v2)])
    else:
        ka, va = cv(k), cv(v)
    q, g = cv(q), cv(g)
    nr, ns, C = rowptr.numel() - 1, ka.shape[0], ka.shape[1]
    D = C // heads
    rows = torch.repeat_interleave(torch.arange(nr), rowptr[1:] - rowptr[:-1])
    E = rows.numel()
    qe, ge = q[rows].view(E, heads, D), g[rows].view(E, heads, D)
    ke, ve = ka[col].view(E, heads, D), va[col].view(E, heads, D)
    prod = qe * ke
    if perm is not None:
        prod = prod[..., perm]
    e = prod.sum(-1) * scale                                               # [E, heads]
    m = torch.full((nr, heads), -float("inf"), dtype=dtype).index_reduce(
        0, rows, e, "amax", include_self=True)
    p = torch.exp(e - m[rows])
    den = torch.zeros(nr, heads, dtype=dtype).index_add(0, rows, p)
    inv = torch.where(den > 0, 1.0 / den, torch.zeros_like(den))
    alpha = p * inv[rows]
    agg = torch.zeros(nr, C, dtype=dtype).index_add(
        0, rows, (alpha.unsqueeze(-1) * ve).reshape(E, C))
    res = {"out": agg if beta == 0 else beta * cv(out) + agg, "stat_m": m, "stat_l": inv}
    ga = (ge * ve).sum(-1)                                                 # [E, heads]
    cc = torch.zeros(nr, heads, dtype=dtype).index_add(0, rows, alpha * ga) if c is None \
        else cv(c)
    de = alpha * (ga - cc[rows])
    res["c"] = cc
    res["dq"] = scale * torch.zeros(nr, C, dtype=dtype).index_add(
        0, rows, (de.unsqueeze(-1) * ke).reshape(E, C))
    res["dk"] = scale * torch.zeros(ns, C, dtype=dtype).index_add(
        0, col, (de.unsqueeze(-1) * qe).reshape(E, C))
    res["dv"] = torch.zeros(ns, C, dtype=dtype).index_add(
        0, col, (alpha.unsqueeze(-1) * ge).reshape(E, C))
    res["alpha"], res["e"] = alpha, e
    return res


@functools.lru_cache(maxsize=None)
def oracle(C: int, heads: int, s: float, beta: float):
    """(fp64, fp32, fp32 with the D-sum in a second order) results of
    :func:`dot_attn_contract` on ``case(C, heads, s)``."""
    rowptr, col, _ = pattern()
    d = case(C, heads, s)
    args = (rowptr, col, d["q"], d["k"], d["v"], None, None, N, d["g"], heads, d["scale"],
            beta, d["out0"])
    D = C // heads
    perm = torch.randperm(D, generator=torch.Generator().manual_seed(D))
    return (dot_attn_contract(*args), dot_attn_contract(*args, dtype=torch.float32),
            dot_attn_contract(*args, dtype=torch.float32, perm=perm))


# ------------------------------------------------------------------------ the contract
def _rowwise_forward(rowptr, col, q, k, v, heads, scale):
    """out_i = sum_j softmax_j(scale <q_i, k_j>) v_j per head, row by row."""
    C = q.shape[1]
    D = C // heads
    outs = []
    for i in range(rowptr.numel() - 1):
        j = col[rowptr[i]:rowptr[i + 1]]
        e = torch.einsum("kd,ekd->ek", q[i].view(heads, D), k[j].view(-1, heads, D)) * scale
        a = torch.softmax(e, 0)                                            # [deg, heads]
        outs.append(torch.einsum("ek,ekd->kd", a, v[j].view(-1, heads, D)).reshape(C))
    return torch.stack(outs)


@pytest.mark.parametrize("beta", [0.0, 0.5])
@pytest.mark.parametrize("two_sources", [False, True])
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("C,heads", [(64, 1), (64, 8), (128, 4), (256, 2)])
def test_contract_matches_autograd(C, heads, s, two_sources, beta):
    rowptr, col, _ = pattern()
    d = case(C, heads, s)
    q, k, v = (d[n].double().requires_grad_() for n in ("q", "k", "v"))
    g = d["g"].double()
    out = _rowwise_forward(rowptr, col, q, k, v, heads, d["scale"])
    gq, gk, gv = torch.autograd.grad(out, (q, k, v), g)
    if two_sources:
        ref = dot_attn_contract(rowptr, col, d["q"], d["k"][:LS], d["v"][:LS], d["k"][LS:],
                                d["v"][LS:], LS, g, heads, d["scale"], beta, d["out0"])
    else:
        ref = dot_attn_contract(rowptr, col, d["q"], d["k"], d["v"], None, None, N, g, heads,
                                d["scale"], beta, d["out0"])
    torch.testing.assert_close(ref["out"], beta * d["out0"].double() + out.detach(), **TOL)
    torch.testing.assert_close(ref["dq"], gq, **TOL)
    torch.testing.assert_close(ref["dk"], gk, **TOL)
    torch.testing.assert_close(ref["dv"], gv, **TOL)
    # c is the FlashAttention delta of this call's own attention sum
    own = ref["out"] - beta * d["out0"].double()
    torch.testing.assert_close(ref["c"], (g * own).view(R, heads, -1).sum(-1), **TOL)
    deg = rowptr[1:] - rowptr[:-1]
    assert (ref["stat_l"][deg == 0] == 0).all() and (ref["stat_l"][deg > 0] > 0).all()
    assert (ref["stat_l"][deg == 1] == 1).all()


@pytest.mark.parametrize("C,heads", PAIRS)
def test_score_scale_conditions(C, heads):
    # s = 0.5: every edge carries weight — one dropped or misattributed edge moves an output
    # by several times the 2e-5 floor
    small = oracle(C, heads, 0.5, 0.0)
    assert float(small[0]["alpha"].min()) >= 1e-4
    # s = 40: exp overflows in fp32 (e^89 > FLT_MAX) unless the row maximum is subtracted
    big = oracle(C, heads, 40.0, 0.0)
    assert float(big[0]["e"].max()) > 89.0
    assert not torch.isfinite(torch.exp(big[0]["e"].max().float()))
    rowptr = pattern()[0]
    full = rowptr[1:] > rowptr[:-1]  # (an empty row's maximum is -inf)
    for res in small + big:
        for name in OUTPUTS + ("c",):
            t = res[name]
            assert torch.isfinite(t[full] if name == "stat_m" else t).all(), name


@pytest.mark.parametrize("C,heads", PAIRS)
def test_one_wrong_edge_exceeds_the_bound(C, heads):
    """What the alpha condition is for: with the last entry of a row dropped, or gathered
    from another source, that row of ``out`` moves by at least five times the bound the GPU
    tests allow — at every row length around a lane-group width and in the hub."""
    rowptr, col, rows = pattern()
    d = case(C, heads, 0.5)
    r64, r32, _ = oracle(C, heads, 0.5, 0.0)
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
        wrong = dot_attn_contract(rp, cl, d["q"], d["k"], d["v"], None, None, N, d["g"], heads,
                                  d["scale"], 0.0, None)
        diff = (wrong["out"] - r64["out"]).abs().amax(1)
        assert (diff[picked] >= 5 * bd).all(), (diff[picked], bd)
        assert (diff[hit == 0] <= 1e-12).all()


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
    q, k, v = mk(d["q"]), mk(d["k"][:ns]), mk(d["v"][:ns])
    kh, vh = (mk(d["k"][ns:]), mk(d["v"][ns:])) if two_sources else (None, None)
    out = dot_attention(q, k, v, pat, kh, vh, heads=heads)  # default scale: 1 / sqrt(D)
    ins = [t for t in (q, k, v, kh, vh) if t is not None]
    grads = torch.autograd.grad(out, ins, d["g"].double())
    ref = oracle(C, heads, s, 0.0)[0]
    torch.testing.assert_close(out.detach(), ref["out"], **TOL)
    torch.testing.assert_close(grads[0], ref["dq"], **TOL)
    if two_sources:
        torch.testing.assert_close(torch.cat([grads[1], grads[3]]), ref["dk"], **TOL)
        torch.testing.assert_close(torch.cat([grads[2], grads[4]]), ref["dv"], **TOL)
    else:
        torch.testing.assert_close(grads[1], ref["dk"], **TOL)
        torch.testing.assert_close(grads[2], ref["dv"], **TOL)
    # fp32 inputs come back as fp32 (evaluated at fp64 inside)
    assert dot_attention(d["q"], d["k"][:ns], d["v"][:ns], pat,
                         None if kh is None else d["k"][ns:],
                         None if vh is None else d["v"][ns:], heads=heads).dtype == torch.float32


@pytest.mark.parametrize("two_sources", [False, True])
def test_op_cpu_gradcheck(two_sources):
    from dgraph_amd.ops import dot_attention
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
    fn = lambda *t: dot_attention(t[0], t[1], t[2], pat, *t[3:], scale=0.7, heads=2)  # noqa: E731
    assert torch.autograd.gradcheck(fn, (q, k, v) + halo)


def test_op_argument_checks():
    from dgraph_amd.ops import dot_attention
    from dgraph_amd.ops.gat import GatPattern

    rowptr, col, _ = pattern()
    pat = GatPattern(rowptr, col, LS, HS)
    d = case(64, 2, 0.5)
    with pytest.raises(ValueError):  # halo columns but no halo rows
        dot_attention(d["q"], d["k"][:LS], d["v"][:LS], pat, heads=2)
    with pytest.raises(ValueError):
        dot_attention(d["q"], d["k"][:LS], d["v"][:LS], pat, d["k"][LS:], None, heads=2)
    with pytest.raises(ValueError):
        dot_attention(d["q"], d["k"][:LS], d["v"][:LS], pat, d["k"][LS:], d["v"][LS:], heads=3)


# ------------------------------------------------------------------------------- the layer
NS, ND, NE, CIN = 23, 17, 90, 6


def _edges(skew_world: int = 0):
    """(src, dst) ids of the test relation. ``skew_world`` = W > 1: the destinations owned
    by the last of W ranks only have sources owned by that rank (it receives no halo rows
    but still sends its rows to the others)."""
    from dgraph_amd.data.hetero import get_vertex_offsets

    g = torch.Generator().manual_seed(4)
    edges = torch.stack([torch.randint(0, NS, (NE,), generator=g),
                         torch.randint(0, ND, (NE,), generator=g)])
    if skew_world > 1:
        s0 = int(get_vertex_offsets(NS, skew_world)[-2])
        d0 = int(get_vertex_offsets(ND, skew_world)[-2])
        mine = edges[1] >= d0
        edges[0, mine] = s0 + edges[0, mine] % (NS - s0)
    return torch.unique(edges, dim=1)


def _dense_transformer(layer, x_dst, x_src, edges):
    """Reference formulation: per-edge q / k / v rows, softmax per destination."""
    H, C = layer.heads, layer.out_channels
    D = C // H
    q = layer.lin_query(x_dst)
    kv = layer.lin_kv(x_src)
    k, v = kv[:, :C], kv[:, C:]
    src, dst = edges
    e = (q[dst].view(-1, H, D) * k[src].view(-1, H, D)).sum(-1) / math.sqrt(D)
    out = torch.zeros(x_dst.shape[0], C, dtype=x_dst.dtype)
    for i in range(x_dst.shape[0]):
        sel = dst == i
        if sel.any():
            a = torch.softmax(e[sel], 0)  # [deg, H]
            out[i] = (v[src[sel]].view(-1, H, D) * a.unsqueeze(-1)).sum(0).reshape(C)
    return out + layer.lin_skip(x_dst) + layer.bias


def _layer(heads, comm=None):
    from dgraph_amd.models.transformer_conv import CommAwareTransformerConv

    torch.manual_seed(0)
    layer = CommAwareTransformerConv(CIN, 8, comm=comm, heads=heads, hetero=True).double()
    with torch.no_grad():
        layer.bias.normal_()
    return layer


@pytest.mark.parametrize("heads", [1, 2])
def test_layer_matches_dense(heads):
    from dgraph_amd.data.hetero import build_relation_graph, get_vertex_offsets

    edges = _edges()
    offs = {0: get_vertex_offsets(ND, 1), 1: get_vertex_offsets(NS, 1)}
    rel = build_relation_graph(edges, 1, 0, offs, 0, 1)
    layer = _layer(heads)
    torch.manual_seed(1)
    xd = torch.randn(ND, CIN, dtype=torch.float64, requires_grad=True)
    xs = torch.randn(NS, CIN, dtype=torch.float64, requires_grad=True)
    out = layer(xd, rel, x_j=xs)
    assert layer(xd, rel, x_j=xs) is not None and "dot_attn_pattern" in rel._cache
    ref = _dense_transformer(layer, xd, xs, edges)
    torch.testing.assert_close(out, ref)
    w = torch.randn_like(out)
    ins = [xd, xs] + list(layer.parameters())
    assert len(ins) == 2 + 6  # W_q, b_q, W_kv, b_kv, W_skip, bias
    ga = torch.autograd.grad((out * w).sum(), ins)
    gb = torch.autograd.grad((ref * w).sum(), ins)
    for a, b in zip(ga, gb):
        torch.testing.assert_close(a, b)


def _layer_dist(rank, world, heads, skew):
    import torch.distributed as dist

    from dgraph_amd import Communicator
    from dgraph_amd.comm.alltoallv import CommStats
    from dgraph_amd.data.hetero import build_relation_graph, get_vertex_offsets

    comm = Communicator.init_process_group("nccl")  # gloo underneath on the CPU
    try:
        edges = _edges(world if skew else 0)
        offs = {0: get_vertex_offsets(ND, world), 1: get_vertex_offsets(NS, world)}
        rel = build_relation_graph(edges, 1, 0, offs, rank, world)
        if skew and rank == world - 1:
            # the shape that must not hang or lose gradient: sends rows, receives none
            assert rel.num_halo == 0 and sum(rel.pattern.send_splits()) > 0
        gen = torch.Generator().manual_seed(1)
        xd = torch.randn(ND, CIN, generator=gen, dtype=torch.float64)
        xs = torch.randn(NS, CIN, generator=gen, dtype=torch.float64)
        w = torch.randn(ND, 8, generator=gen, dtype=torch.float64)
        d0, d1 = int(offs[0][rank]), int(offs[0][rank + 1])
        s0, s1 = int(offs[1][rank]), int(offs[1][rank + 1])
        layer = _layer(heads, comm)
        xdl = xd[d0:d1].clone().requires_grad_()
        xsl = xs[s0:s1].clone().requires_grad_()
        CommStats.reset()
        out = layer(xdl, rel, x_j=xsl)
        assert CommStats.calls == 1, CommStats.calls   # one exchange of the [k | v] rows
        (out * w[d0:d1]).sum().backward()
        assert CommStats.calls == 2, CommStats.calls   # and its adjoint
        got = [p.grad.clone() for p in layer.parameters()]
        for t in got:
            dist.all_reduce(t)
        # the same layer at W = 1 on the whole graph, in this process
        one = _layer(heads, types.SimpleNamespace(get_world_size=lambda: 1))
        offs1 = {0: get_vertex_offsets(ND, 1), 1: get_vertex_offsets(NS, 1)}
        rel1 = build_relation_graph(edges, 1, 0, offs1, 0, 1)
        xd1, xs1 = xd.clone().requires_grad_(), xs.clone().requires_grad_()
        ref = one(xd1, rel1, x_j=xs1)
        assert CommStats.calls == 2
        (ref * w).sum().backward()
        torch.testing.assert_close(out.detach(), ref.detach()[d0:d1])
        torch.testing.assert_close(xdl.grad, xd1.grad[d0:d1])
        torch.testing.assert_close(xsl.grad, xs1.grad[s0:s1])
        for a, p in zip(got, one.parameters()):
            torch.testing.assert_close(a, p.grad)
    finally:
        comm.destroy()


@pytest.mark.parametrize("world,heads,skew", [(2, 2, False), (3, 1, False), (2, 1, True),
                                              (3, 2, True)])
def test_layer_distributed(ranks, world, heads, skew):
    ranks(_layer_dist, world, heads, skew)
