"""The contract of the fused GATv2 attention kernels (csrc/kernels/gatv2_f32.hip) written out
per edge in plain PyTorch, the op's CPU path and the ``CommAwareGATv2Conv`` layer
(tests/test_gatv2_gpu.py imports the contract and its inputs from here).

:func:`gatv2_contract` takes exactly what the three kernels take — the CSR pattern, the
destination rows ``l``, the two gathered ``r`` sources, the attention vector, dL/dout, the
slope, ``beta`` and ``out`` on entry — and returns every array they write (``da`` as the full
sum). It shares no code with ``ops/gatv2.py``. Run in fp64 it is the oracle; run in fp32 it
gives the error a faithful fp32 evaluation of the same formula has, from which the GPU tests
derive their bound (``test_gat_kernels.bound``).

The pattern is ``test_gat_kernels.pattern()`` (37 rows over 41 local + 19 halo sources,
degrees 0, 1, LPR +- 1 and a 301-entry hub; its conditions are asserted there). Inputs:
``l``, ``r``, ``g`` ~ N(0, 1) and ``a = s randn(C) / sqrt(D)`` at score scale 0.5 (every edge
carries at least 1e-4 of its row) and 40 (``exp`` overflows in fp32 unless the row maximum
is subtracted).
"""
from __future__ import annotations

import functools
import math
import types

import pytest
import torch
import torch.nn.functional as F

from test_dot_attn import CIN, ND, NS, _edges
from test_gat_kernels import HS, LS, N, PAIRS, R, bound, pattern, transpose  # noqa: F401

SLOPE = 0.2
SCALES = [0.5, 40.0]
OUTPUTS = ("out", "stat_m", "stat_l", "dl", "dr", "da")
TOL = dict(atol=1e-10, rtol=1e-10)


@functools.lru_cache(maxsize=None)
def case(C: int, heads: int, s: float):
    """The kernels' inputs for one (C, heads, score scale), fp32 values on the CPU: r over
    all N sources (the tests split it at LS)."""
    gen = torch.Generator().manual_seed(9000 * C + 10 * heads + int(s))
    rn = lambda *shape: torch.randn(*shape, generator=gen)  # noqa: E731
    l, r, g = rn(R, C), rn(N, C), rn(R, C)
    a = s * rn(C) / math.sqrt(C // heads)
    return dict(C=C, heads=heads, l=l, r=r, g=g, a=a, out0=rn(R, C), slope=SLOPE)


def gatv2_contract(rowptr, col, l, r, r2, nsplit, a, g, heads, slope, beta, out, c=None,
                   dtype=torch.float64):
    """What gatv2_fwd / gatv2_bwd_dst / gatv2_bwd_src compute, per edge, in ``dtype``.

    ``r`` serves columns below ``nsplit`` (all of them without ``r2``), ``r2`` the columns
    from ``nsplit`` on. ``c`` [rows, heads] is the backward kernels' input (``None``: this
    evaluation's own ``sum_j alpha ga``). Returns out, stat_m, stat_l, c, dl over the
    destination rows, dr over all source rows (``[r rows | r2 rows]``), da [C], plus the
    per-edge ``alpha``, scores ``e`` and pre-activations ``pre`` [E, C]."""
    cv = lambda t: t.detach().cpu().to(dtype)  # noqa: E731
    rowptr, col = rowptr.cpu().long(), col.cpu().long()
    ra = torch.cat([cv(r)[:nsplit], cv(r2)]) if r2 is not None else cv(r)
    l, g, a = cv(l), cv(g), cv(a).reshape(-1)
    nr, ns, C = rowptr.numel() - 1, ra.shape[0], ra.shape[1]
    D = C // heads
    rows = torch.repeat_interleave(torch.arange(nr), rowptr[1:] - rowptr[:-1])
    E = rows.numel()
    re, ge = ra[col], g[rows]                                              # [E, C]
    pre = l[rows] + re                                                     # one add
    act = torch.where(pre > 0, pre, slope * pre)
    lam = torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, slope))
    e = (a * act).view(E, heads, D).sum(-1)                                # [E, heads]
    m = torch.full((nr, heads), -float("inf"), dtype=dtype).index_reduce(
        0, rows, e, "amax", include_self=True)
    p = torch.exp(e - m[rows])
    den = torch.zeros(nr, heads, dtype=dtype).index_add(0, rows, p)
    inv = torch.where(den > 0, 1.0 / den, torch.zeros_like(den))
    alpha = p * inv[rows]
    wide = lambda t: t.unsqueeze(-1).expand(E, heads, D).reshape(E, C)  # noqa: E731
    agg = torch.zeros(nr, C, dtype=dtype).index_add(0, rows, wide(alpha) * re)
    res = {"out": agg if beta == 0 else beta * cv(out) + agg, "stat_m": m, "stat_l": inv}
    ga = (ge * re).view(E, heads, D).sum(-1)                               # [E, heads]
    cc = torch.zeros(nr, heads, dtype=dtype).index_add(0, rows, alpha * ga) if c is None \
        else cv(c)
    de = alpha * (ga - cc[rows])
    res["c"] = cc
    dpre = wide(de) * a * lam                                              # [E, C]
    res["dl"] = torch.zeros(nr, C, dtype=dtype).index_add(0, rows, dpre)
    res["dr"] = torch.zeros(ns, C, dtype=dtype).index_add(0, col, wide(alpha) * ge + dpre)
    res["da"] = (wide(de) * act).sum(0)
    res["alpha"], res["e"], res["pre"] = alpha, e, pre
    return res


@functools.lru_cache(maxsize=None)
def oracle(C: int, heads: int, s: float, beta: float):
    """(fp64, fp32) results of :func:`gatv2_contract` on ``case(C, heads, s)``."""
    rowptr, col, _ = pattern()
    d = case(C, heads, s)
    args = (rowptr, col, d["l"], d["r"], None, N, d["a"], d["g"], heads, SLOPE, beta,
            d["out0"])
    return gatv2_contract(*args), gatv2_contract(*args, dtype=torch.float32)


# ------------------------------------------------------------------------ the contract
def _rowwise_forward(rowptr, col, l, r, a, heads, slope):
    """out_i = sum_j softmax_j(a . leaky_relu(l_i + r_j)) r_j per head, row by row."""
    C = l.shape[1]
    D = C // heads
    outs = []
    for i in range(rowptr.numel() - 1):
        j = col[rowptr[i]:rowptr[i + 1]]
        act = F.leaky_relu(l[i] + r[j], slope).view(-1, heads, D)
        al = torch.softmax((act * a.view(heads, D)).sum(-1), 0)            # [deg, heads]
        outs.append(torch.einsum("ek,ekd->kd", al, r[j].view(-1, heads, D)).reshape(C))
    return torch.stack(outs)


@pytest.mark.parametrize("beta", [0.0, 0.5])
@pytest.mark.parametrize("two_sources", [False, True])
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("C,heads", PAIRS)
def test_contract_matches_autograd(C, heads, s, two_sources, beta):
    rowptr, col, _ = pattern()
    d = case(C, heads, s)
    l, r, a = (d[n].double().requires_grad_() for n in ("l", "r", "a"))
    g = d["g"].double()
    out = _rowwise_forward(rowptr, col, l, r, a, heads, SLOPE)
    gl, gr, ga = torch.autograd.grad(out, (l, r, a), g)
    if two_sources:
        ref = gatv2_contract(rowptr, col, d["l"], d["r"][:LS], d["r"][LS:], LS, d["a"], g,
                             heads, SLOPE, beta, d["out0"])
    else:
        ref = gatv2_contract(rowptr, col, d["l"], d["r"], None, N, d["a"], g, heads, SLOPE,
                             beta, d["out0"])
    torch.testing.assert_close(ref["out"], beta * d["out0"].double() + out.detach(), **TOL)
    torch.testing.assert_close(ref["dl"], gl, **TOL)
    torch.testing.assert_close(ref["dr"], gr, **TOL)
    torch.testing.assert_close(ref["da"], ga, **TOL)
    # c is the FlashAttention delta of this call's own attention sum
    own = ref["out"] - beta * d["out0"].double()
    torch.testing.assert_close(ref["c"], (g * own).view(R, heads, -1).sum(-1), **TOL)
    deg = rowptr[1:] - rowptr[:-1]
    assert (ref["stat_l"][deg == 0] == 0).all() and (ref["stat_l"][deg > 0] > 0).all()
    assert (ref["stat_l"][deg == 1] == 1).all()


@pytest.mark.parametrize("C,heads", PAIRS)
def test_input_conditions(C, heads):
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
    # pre is one correctly rounded add of the same fp32 inputs: the fp32 evaluation takes
    # the LeakyReLU branch of the fp64 one on every (edge, channel)
    for r64, r32 in (small, big):
        assert torch.equal(r64["pre"] > 0, r32["pre"] > 0)


@pytest.mark.parametrize("C,heads", PAIRS)
def test_one_wrong_edge_exceeds_the_bound(C, heads):
    """What the alpha condition is for: with the last entry of a row dropped, or gathered
    from another source, that row of ``out`` moves by at least five times the bound the GPU
    tests allow — at every row length around a lane-group width and in the hub."""
    rowptr, col, rows = pattern()
    d = case(C, heads, 0.5)
    r64, r32 = oracle(C, heads, 0.5, 0.0)
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
        wrong = gatv2_contract(rp, cl, d["l"], d["r"], None, N, d["a"], d["g"], heads, SLOPE,
                               0.0, None)
        diff = (wrong["out"] - r64["out"]).abs().amax(1)
        assert (diff[picked] >= 5 * bd).all(), (diff[picked], bd)
        assert (diff[hit == 0] <= 1e-12).all()


# ------------------------------------------------------------------------ the op on the CPU
@pytest.mark.parametrize("two_sources", [False, True])
@pytest.mark.parametrize("C,heads,s", [(64, 2, 0.5), (128, 8, 40.0), (256, 1, 0.5)])
def test_op_cpu_matches_contract(C, heads, s, two_sources):
    from dgraph_amd.ops import gatv2_attention
    from dgraph_amd.ops.gat import GatPattern

    rowptr, col, _ = pattern()
    d = case(C, heads, s)
    ns, nh = (LS, HS) if two_sources else (N, 0)
    pat = GatPattern(rowptr, col, ns, nh)
    mk = lambda t: t.double().clone().requires_grad_()  # noqa: E731
    l, r = mk(d["l"]), mk(d["r"][:ns])
    a = mk(d["a"].view(heads, -1))  # [heads, D]
    rh = mk(d["r"][ns:]) if two_sources else None
    out = gatv2_attention(l, r, a, pat, rh, heads=heads)  # default slope: 0.2
    ins = [t for t in (l, r, a, rh) if t is not None]
    grads = torch.autograd.grad(out, ins, d["g"].double())
    ref = oracle(C, heads, s, 0.0)[0]
    torch.testing.assert_close(out.detach(), ref["out"], **TOL)
    torch.testing.assert_close(grads[0], ref["dl"], **TOL)
    dr = torch.cat([grads[1], grads[3]]) if two_sources else grads[1]
    torch.testing.assert_close(dr, ref["dr"], **TOL)
    assert grads[2].shape == (heads, C // heads)
    torch.testing.assert_close(grads[2].reshape(-1), ref["da"], **TOL)
    # fp32 inputs come back as fp32 (evaluated at fp64 inside); att as a flat [C] vector
    out32 = gatv2_attention(d["l"], d["r"][:ns], d["a"], pat,
                            d["r"][ns:] if two_sources else None, heads=heads)
    assert out32.dtype == torch.float32
    torch.testing.assert_close(out32.double(), ref["out"], atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("two_sources", [False, True])
def test_op_cpu_gradcheck(two_sources):
    from dgraph_amd.ops import gatv2_attention
    from dgraph_amd.ops.gat import GatPattern

    gen = torch.Generator().manual_seed(3)
    deg = torch.tensor([3, 0, 1, 5, 2, 4, 1])
    rowptr = torch.zeros(8, dtype=torch.long)
    rowptr[1:] = torch.cumsum(deg, 0)
    nl, nh = (5, 3) if two_sources else (8, 0)
    col = torch.randint(0, nl + nh, (int(rowptr[-1]),), generator=gen)
    pat = GatPattern(rowptr, col, nl, nh)
    rn = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64).requires_grad_()  # noqa: E731
    l, r, a = rn(7, 6), rn(nl, 6), rn(2, 3)
    halo = (rn(nh, 6),) if two_sources else ()
    fn = lambda *t: gatv2_attention(t[0], t[1], t[2], pat, *t[3:], heads=2,  # noqa: E731
                                    negative_slope=0.3)
    assert torch.autograd.gradcheck(fn, (l, r, a) + halo)


def test_op_argument_checks():
    from dgraph_amd.ops import gatv2_attention
    from dgraph_amd.ops.gat import GatPattern

    rowptr, col, _ = pattern()
    pat = GatPattern(rowptr, col, LS, HS)
    d = case(64, 2, 0.5)
    l, r, a = d["l"], d["r"], d["a"]
    gatv2_attention(l, r[:LS], a, pat, r[LS:], heads=2)  # the valid call
    with pytest.raises(ValueError):  # halo columns but no halo rows
        gatv2_attention(l, r[:LS], a, pat, heads=2)
    with pytest.raises(ValueError):  # xsh given but xs does not have nsplit rows
        gatv2_attention(l, r, a, pat, r[LS:], heads=2)
    with pytest.raises(ValueError):  # too few halo rows
        gatv2_attention(l, r[:LS], a, pat, r[LS:-1], heads=2)
    with pytest.raises(ValueError):  # rows against pat.R
        gatv2_attention(l[:-1], r[:LS], a, pat, r[LS:], heads=2)
    with pytest.raises(ValueError):  # width not divisible by heads
        gatv2_attention(l, r[:LS], a, pat, r[LS:], heads=3)
    with pytest.raises(ValueError):  # att of another width
        gatv2_attention(l, r[:LS], a[:32], pat, r[LS:], heads=2)
    with pytest.raises(ValueError):  # att [D, heads] is not [heads, D]
        gatv2_attention(l, r[:LS], a.view(32, 2), pat, r[LS:], heads=2)
    with pytest.raises(ValueError):  # xs of another width
        gatv2_attention(l, r[:LS, :32], a, pat, r[LS:], heads=2)


# ------------------------------------------------------------------------------- the layer
def _dense_gatv2(layer, x_dst, x_src, edges):
    """Reference formulation: per-edge l / r rows, softmax per destination."""
    H, C = layer.heads, layer.out_channels
    D = C // H
    l, r = layer.lin_dst(x_dst), layer.lin_src(x_src)
    src, dst = edges
    act = F.leaky_relu(l[dst] + r[src], layer.negative_slope).view(-1, H, D)
    e = (act * layer.att).sum(-1)
    out = torch.zeros(x_dst.shape[0], C, dtype=x_dst.dtype, device=x_dst.device)
    for i in range(x_dst.shape[0]):
        sel = dst == i
        if sel.any():
            a = torch.softmax(e[sel], 0)  # [deg, H]
            out[i] = (r[src[sel]].view(-1, H, D) * a.unsqueeze(-1)).sum(0).reshape(C)
    if layer.res_net is not None:
        out = out + layer.res_net(x_dst)
    return out + layer.bias


def _layer(heads, comm=None, share=False, hetero=True, cin=CIN, cout=8):
    from dgraph_amd.models import CommAwareGATv2Conv

    torch.manual_seed(0)
    layer = CommAwareGATv2Conv(cin, cout, comm=comm, heads=heads, residual=True,
                               share_weights=share, hetero=hetero).double()
    with torch.no_grad():
        layer.bias.normal_()
    return layer


@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("heads", [1, 2])
def test_layer_matches_dense(heads, share):
    from dgraph_amd.data.hetero import build_relation_graph, get_vertex_offsets

    edges = _edges()
    offs = {0: get_vertex_offsets(ND, 1), 1: get_vertex_offsets(NS, 1)}
    rel = build_relation_graph(edges, 1, 0, offs, 0, 1)
    layer = _layer(heads, share=share)
    assert (layer.lin_src is layer.lin_dst) == share and layer.att.shape == (heads, 8 // heads)
    torch.manual_seed(1)
    xd = torch.randn(ND, CIN, dtype=torch.float64, requires_grad=True)
    xs = torch.randn(NS, CIN, dtype=torch.float64, requires_grad=True)
    out = layer(xd, rel, x_j=xs)
    assert layer(xd, rel, x_j=xs) is not None and "gatv2_pattern" in rel._cache
    ref = _dense_gatv2(layer, xd, xs, edges)
    torch.testing.assert_close(out, ref)
    w = torch.randn_like(out)
    ins = [xd, xs] + list(layer.parameters())
    # W_src, b_src (, W_dst, b_dst), att, W_res, bias
    assert len(ins) == 2 + (5 if share else 7)
    ga = torch.autograd.grad((out * w).sum(), ins)
    gb = torch.autograd.grad((ref * w).sum(), ins)
    for a, b in zip(ga, gb):
        torch.testing.assert_close(a, b)


@pytest.mark.parametrize("share", [False, True])
def test_layer_one_input_matches_dense(share):
    """One input for both sides (a square relation): unshared weights run as one GEMM into a
    [N, 2C] buffer whose halves the op reads in place."""
    from dgraph_amd.data.hetero import build_relation_graph, get_vertex_offsets

    gen = torch.Generator().manual_seed(6)
    edges = torch.unique(torch.randint(0, NS, (2, 80), generator=gen), dim=1)
    offs = {0: get_vertex_offsets(NS, 1)}
    rel = build_relation_graph(edges, 0, 0, offs, 0, 1)
    layer = _layer(2, share=share, hetero=False)
    x = torch.randn(NS, CIN, generator=gen, dtype=torch.float64).requires_grad_()
    out = layer(x, rel)
    ref = _dense_gatv2(layer, x, x, edges)
    torch.testing.assert_close(out, ref)
    w = torch.randn(out.shape, generator=gen, dtype=torch.float64)
    ins = [x] + list(layer.parameters())
    for a, b in zip(torch.autograd.grad((out * w).sum(), ins),
                    torch.autograd.grad((ref * w).sum(), ins)):
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
        assert CommStats.calls == 1, CommStats.calls   # one exchange of the r rows
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
        assert len(got) == 7
        for a, p in zip(got, one.parameters()):
            torch.testing.assert_close(a, p.grad)
    finally:
        comm.destroy()


@pytest.mark.parametrize("world,heads,skew", [(2, 2, False), (3, 1, False), (2, 1, True),
                                              (3, 2, True)])
def test_layer_distributed(ranks, world, heads, skew):
    ranks(_layer_dist, world, heads, skew)
