"""One softmax over several edge sets: the carry-in contract of ``dot_attn_fwd_carry_f32``
written out per edge, ``GatPattern.split()``, the ``dot_attention_parts`` op on the CPU and
``CommAwareTransformerConv(overlap=True)`` on gloo (tests/test_dot_attn_parts_gpu.py imports
the contract and the edge partitions from here).

The pattern and the inputs are those of tests/test_dot_attn.py (37 rows over 41 local + 19
halo sources, degrees 0, 1, LPR +- 1 and a 301-entry hub; score scales 0.5 and 40). Its
entries are partitioned four ways (:func:`partition`), each part a pattern over the same 37
rows that reads rows ``[lo, hi)`` of ``k`` / ``v``:

    P1  by column: ``< LS``, then ``>= LS`` rebased, reading ``k[LS:]`` / ``v[LS:]``
    P2  by row parity: even rows' entries, then odd rows' (in the second pass the even rows
        have no entries, and every odd row starts from ``stat_l = 0``)
    P3  entry slot index mod 3: three chained passes
    P4  nothing, then everything

:func:`chain` is how a chained forward is checked everywhere: the plain forward over the
first part, every ``(row, head)`` with ``stat_l == 0`` poisoned with NaN in ``out`` and
``stat_m``, then one carry pass per further part. fp64 comparisons use ``TOL`` of
tests/test_dot_attn.py.
"""
from __future__ import annotations

import functools
import types

import pytest
import torch

from test_dot_attn import (CIN, ND, NS, SCALES, TOL, _edges, case, dot_attn_contract, oracle)
from test_gat_kernels import HS, LS, N, R, pattern

PARTITIONS = ("P1", "P2", "P3", "P4")


@functools.lru_cache(maxsize=None)
def partition(name: str):
    """[(rowptr [R+1], col [E_p] int64 rebased to ``[0, hi - lo)``, lo, hi)] per part."""
    rowptr, col, rows = pattern()
    E = col.numel()
    slot = torch.arange(E) - rowptr[rows]
    if name == "P1":
        sels = [(col < LS, 0, LS), (col >= LS, LS, N)]
    elif name == "P2":
        sels = [(rows % 2 == 0, 0, N), (rows % 2 == 1, 0, N)]
    elif name == "P3":
        sels = [(slot % 3 == p, 0, N) for p in range(3)]
    elif name == "P4":
        sels = [(torch.zeros(E, dtype=torch.bool), 0, N), (torch.ones(E, dtype=torch.bool), 0, N)]
    else:
        raise KeyError(name)
    parts = []
    for sel, lo, hi in sels:
        rp = torch.zeros(R + 1, dtype=torch.long)
        rp[1:] = torch.cumsum(torch.bincount(rows[sel], minlength=R), 0)
        parts.append((rp, col[sel] - lo, lo, hi))
    return parts


def _deg(rp):
    return rp[1:] - rp[:-1]


def test_partitions_hold_their_row_classes():
    rowptr, col, rows = pattern()
    deg = _deg(rowptr)
    for name in PARTITIONS:
        parts = partition(name)
        assert sum(int(p[0][-1]) for p in parts) == col.numel()
        assert torch.equal(sum(_deg(p[0]) for p in parts), deg)
        for r in range(R):  # the union of the parts, per row, is the row
            got = torch.cat([p[1][p[0][r]:p[0][r + 1]] + p[2] for p in parts])
            assert torch.equal(got.sort().values, col[rowptr[r]:rowptr[r + 1]].sort().values)
    a, b = (_deg(p[0]) for p in partition("P1"))
    assert ((a > 0) & (b > 0)).any()        # carried state and new entries
    assert ((a > 0) & (b == 0)).any()       # carried state, untouched by the second pass
    assert ((deg > 0) & (a == 0)).sum() == 0  # the pattern has no all-halo row: P2 has them
    assert int(b.max()) > 64                # the hub spans several chunks in the carry pass
    a, b = (_deg(p[0]) for p in partition("P2"))
    even = torch.arange(R) % 2 == 0
    assert (b[even] == 0).all() and (a[even] > 0).any()  # rows the carry pass must not touch
    assert (a[~even] == 0).all() and (b[~even] > 0).any()  # rows that start from stat_l = 0
    assert (b[~even] == 0).any()            # and rows that have nothing at all
    d3 = torch.stack([_deg(p[0]) for p in partition("P3")])
    assert (d3 > 0).all(0).any()            # rows carried through all three passes
    assert ((d3[0] > 0) & (d3[1] == 0)).any() and ((d3[1] > 0) & (d3[2] == 0)).any()
    assert int(d3[2].max()) > 64
    a, b = (_deg(p[0]) for p in partition("P4"))
    assert int(a.sum()) == 0 and torch.equal(b, deg)


# ------------------------------------------------------------------------ the carry contract
def carry_contract(rowptr, col, q, k, v, heads, scale, out, stat_m, stat_l,
                   dtype=torch.float64):
    """What ``dot_attn_fwd_carry_f32`` computes, per edge and row by row, in ``dtype``:
    returns the new ``(out, stat_m, stat_l)``. A row without entries keeps its state; a
    ``(row, head)`` with ``stat_l == 0`` does not read ``out`` or ``stat_m``."""
    cv = lambda t: t.detach().cpu().to(dtype)  # noqa: E731
    rowptr, col = rowptr.cpu().long(), col.cpu().long()
    q, k, v = cv(q), cv(k), cv(v)
    out, m, l = cv(out).clone(), cv(stat_m).clone(), cv(stat_l).clone()
    C = q.shape[1]
    D = C // heads
    zero = torch.zeros(heads, dtype=dtype)
    for r in range(rowptr.numel() - 1):
        j = col[rowptr[r]:rowptr[r + 1]]
        if j.numel() == 0:
            continue
        e = (q[r].view(1, heads, D) * k[j].view(-1, heads, D)).sum(-1) * scale   # [deg, heads]
        L = l[r]
        assert (L >= 0).all()
        have = L > 0
        m0 = torch.where(have, m[r], torch.full_like(zero, -float("inf")))
        s0 = torch.where(have, 1.0 / L, zero)
        acc0 = torch.where(have.unsqueeze(-1), out[r].view(heads, D) / L.unsqueeze(-1),
                           torch.zeros(heads, D, dtype=dtype))
        m1 = torch.maximum(m0, e.max(0).values)
        w = torch.where(have, torch.exp(m0 - m1), zero)
        p = torch.exp(e - m1)
        s1 = s0 * w + p.sum(0)
        acc = acc0 * w.unsqueeze(-1) + (p.unsqueeze(-1) * v[j].view(-1, heads, D)).sum(0)
        out[r] = (acc / s1.unsqueeze(-1)).reshape(C)
        m[r] = m1
        l[r] = 1.0 / s1
    return out, m, l


def poison_unset(out, stat_m, stat_l):
    """NaN into ``out`` and ``stat_m`` wherever ``stat_l == 0`` (nothing accumulated yet)."""
    heads = stat_l.shape[1]
    unset = stat_l == 0
    stat_m[unset] = float("nan")
    o = out.view(out.shape[0], heads, -1)
    o[unset] = float("nan")
    return unset


def chain(name, first, carry, C, heads, s):
    """The chained forward over partition ``name``: ``first(rowptr, col, k, v)`` is the plain
    forward and returns ``(out, stat_m, stat_l)``; the state is poisoned where unset; then
    ``carry(rowptr, col, k, v, out, stat_m, stat_l)`` per further part (returns the state).
    Also returns the state before each carry pass."""
    d = case(C, heads, s)
    before = []
    state = None
    for p, (rp, cl, lo, hi) in enumerate(partition(name)):
        k, v = d["k"][lo:hi], d["v"][lo:hi]
        if p == 0:
            state = first(rp, cl, k, v)
            poison_unset(*state)
        else:
            before.append(tuple(t.clone() for t in state))
            state = carry(rp, cl, k, v, *state)
    return state, before


def check_chain_vs_single_pass(state, cmp):
    """``cmp(name, got, rows)`` compares ``got`` with rows ``rows`` of the single-pass
    oracle's ``name``: out / stat_m over the non-empty rows, stat_l everywhere. Rows that
    have no entry in any part were never written: still poisoned, ``stat_l`` 0."""
    out, m, l = (t.detach().cpu() for t in state)
    full = _deg(pattern()[0]) > 0
    assert torch.isnan(out[~full]).all() and (l[~full] == 0).all()
    assert torch.isfinite(out[full]).all() and torch.isfinite(m[full]).all()
    cmp("out", out[full], full)
    cmp("stat_m", m[full], full)
    cmp("stat_l", l, slice(None))


def check_idle_rows_untouched(name, before, state):
    """A row without entries in a carry pass keeps ``out``, ``stat_m``, ``stat_l`` bitwise."""
    parts = partition(name)
    after = before[1:] + [state]
    assert len(before) == len(parts) - 1
    for (rp, _, _, _), b, a in zip(parts[1:], before, after):
        idle = _deg(rp) == 0
        for x, y in zip(b, a):
            x, y = x.detach().cpu()[idle].contiguous(), y.detach().cpu()[idle].contiguous()
            bits = torch.int64 if x.dtype == torch.float64 else torch.int32
            assert torch.equal(x.view(bits), y.view(bits))


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("name", PARTITIONS)
@pytest.mark.parametrize("C,heads", [(64, 1), (64, 8), (128, 4), (256, 2)])
def test_carry_contract_chains_to_the_single_pass(C, heads, name, s):
    d = case(C, heads, s)

    def first(rp, cl, k, v):
        r = dot_attn_contract(rp, cl, d["q"], k, v, None, None, k.shape[0], d["g"], heads,
                              d["scale"], 0.0, None)
        return r["out"], r["stat_m"], r["stat_l"]

    def carry(rp, cl, k, v, out, m, l):
        return carry_contract(rp, cl, d["q"], k, v, heads, d["scale"], out, m, l)

    state, before = chain(name, first, carry, C, heads, s)
    ref = oracle(C, heads, s, 0.0)[0]
    check_chain_vs_single_pass(
        state, lambda n, a, rows: torch.testing.assert_close(a, ref[n][rows], **TOL, msg=n))
    check_idle_rows_untouched(name, before, state)


# -------------------------------------------------------------------------- GatPattern.split
def _check_split(rowptr, col, ns, nh):
    from dgraph_amd.ops.gat import GatPattern
    from test_gat_kernels import transpose

    pat = GatPattern(rowptr, col, ns, nh)
    inner, outer = pat.split()
    assert pat.split()[0] is inner and pat.split()[1] is outer  # built once
    assert (inner.R, inner.nsplit, inner.H) == (pat.R, ns, 0)
    assert (outer.R, outer.nsplit + outer.H) == (pat.R, nh)
    for part, ncols in ((inner, ns), (outer, nh)):
        assert part.col.dtype == torch.int32 and part.rowptr.dtype == torch.long
        if part.col.numel():
            assert int(part.col.min()) >= 0 and int(part.col.max()) < ncols
        t_rowptr, t_col = transpose(part.rowptr, part.col, ncols)
        assert torch.equal(part.t_rowptr, t_rowptr)
        assert torch.equal(part.t_col.long(), t_col)
    for r in range(pat.R):
        a = inner.col[inner.rowptr[r]:inner.rowptr[r + 1]].long()
        b = outer.col[outer.rowptr[r]:outer.rowptr[r + 1]].long() + ns
        assert (a < ns).all()
        merged = pat.col[pat.rowptr[r]:pat.rowptr[r + 1]].long()
        assert torch.equal(torch.cat([a, b]).sort().values, merged.sort().values)
    return inner, outer


def test_pattern_split():
    rowptr, col, _ = pattern()
    inner, outer = _check_split(rowptr, col, LS, HS)
    assert inner.col.numel() == int((col < LS).sum()) and outer.col.numel() > 0
    # no halo rows, and halo rows that no entry names
    for ns, nh in ((N, 0), (N, 5)):
        inner, outer = _check_split(rowptr, col, ns, nh)
        assert outer.col.numel() == 0 and int(outer.rowptr[-1]) == 0
        assert torch.equal(inner.col.long(), col) and torch.equal(inner.rowptr, rowptr)
        assert outer.t_rowptr.numel() == nh + 1


# ------------------------------------------------------------------ dot_attention_parts, CPU
def _gat_parts(name, dev="cpu"):
    from dgraph_amd.ops.gat import GatPattern

    return [(GatPattern(rp.to(dev), cl.to(dev), hi - lo, 0), lo, hi)
            for rp, cl, lo, hi in partition(name)]


def run_parts(name, dev, dtype, C, heads, s):
    """``dot_attention_parts`` over partition ``name`` with every part reading its rows of
    one ``k`` / ``v`` and the one ``q``: out and the gradients of q, k, v."""
    from dgraph_amd.ops import dot_attention_parts

    d = case(C, heads, s)
    q, k, v = (d[n].to(dev, dtype).requires_grad_() for n in ("q", "k", "v"))
    parts = [(q, k[lo:hi], v[lo:hi], pat) for pat, lo, hi in _gat_parts(name, dev)]
    out = dot_attention_parts(parts, heads=heads)
    gq, gk, gv = torch.autograd.grad(out, (q, k, v), d["g"].to(dev, dtype))
    return {"out": out.detach(), "dq": gq, "dk": gk, "dv": gv}


@pytest.mark.parametrize("name", PARTITIONS)
@pytest.mark.parametrize("C,heads,s", [(64, 2, 0.5), (128, 8, 40.0), (256, 1, 0.5)])
def test_parts_cpu_match_the_merged_pattern(C, heads, s, name):
    from dgraph_amd.ops import dot_attention
    from dgraph_amd.ops.gat import GatPattern

    rowptr, col, _ = pattern()
    d = case(C, heads, s)
    got = run_parts(name, "cpu", torch.float64, C, heads, s)
    q, k, v = (d[n].double().requires_grad_() for n in ("q", "k", "v"))
    out = dot_attention(q, k, v, GatPattern(rowptr, col, N, 0), heads=heads)
    gq, gk, gv = torch.autograd.grad(out, (q, k, v), d["g"].double())
    for n, b in (("out", out.detach()), ("dq", gq), ("dk", gk), ("dv", gv)):
        torch.testing.assert_close(got[n], b, **TOL, msg=n)
    ref = oracle(C, heads, s, 0.0)[0]
    for n in got:
        torch.testing.assert_close(got[n], ref[n], **TOL, msg=n)
    assert run_parts(name, "cpu", torch.float32, C, heads, s)["out"].dtype == torch.float32


def test_single_part_cpu_is_dot_attention():
    from dgraph_amd.ops import dot_attention, dot_attention_parts
    from dgraph_amd.ops.gat import GatPattern

    rowptr, col, _ = pattern()
    d = case(64, 2, 0.5)
    pat = GatPattern(rowptr, col, N, 0)
    q, k, v = d["q"].double(), d["k"].double(), d["v"].double()
    assert torch.equal(dot_attention_parts([(q, k, v, pat)], heads=2),
                       dot_attention(q, k, v, pat, heads=2))


def _small_parts(gen, n_parts, heads, C, R_=7):
    """Random small parts with their own q / k / v and their own source counts."""
    from dgraph_amd.ops.gat import GatPattern

    parts = []
    for p in range(n_parts):
        deg = torch.randint(0, 5, (R_,), generator=gen)
        deg[1] = 0           # a row empty in every part
        if p > 0:
            deg[2] = 0       # a row only the first part reaches
        else:
            deg[3] = 0       # a row no earlier part has reached when the second arrives
        rowptr = torch.zeros(R_ + 1, dtype=torch.long)
        rowptr[1:] = torch.cumsum(deg, 0)
        n = 4 + p
        col = torch.randint(0, n, (int(rowptr[-1]),), generator=gen)
        rn = lambda *shape: torch.randn(*shape, generator=gen,  # noqa: E731
                                        dtype=torch.float64).requires_grad_()
        parts.append((rn(R_, C), rn(n, C), rn(n, C), GatPattern(rowptr, col, n, 0)))
    return parts


def _dense_union(parts, heads, scale):
    """Per destination: one softmax over the scores of every part's edges (plain autograd)."""
    R_, C = parts[0][0].shape
    D = C // heads
    rows = []
    for i in range(R_):
        es, vs = [], []
        for q, k, v, pat in parts:
            j = pat.col[pat.rowptr[i]:pat.rowptr[i + 1]].long()
            es.append(torch.einsum("kd,ekd->ek", q[i].view(heads, D),
                                   k[j].view(-1, heads, D)) * scale)
            vs.append(v[j].view(-1, heads, D))
        e, vv = torch.cat(es), torch.cat(vs)
        if e.shape[0] == 0:
            rows.append(torch.zeros(C, dtype=parts[0][0].dtype))
        else:
            rows.append(torch.einsum("ek,ekd->kd", torch.softmax(e, 0), vv).reshape(C))
    return torch.stack(rows)


@pytest.mark.parametrize("n_parts,heads", [(2, 1), (3, 2)])
def test_parts_cpu_own_operands_match_dense_union(n_parts, heads):
    from dgraph_amd.ops import dot_attention_parts

    gen = torch.Generator().manual_seed(5)
    parts = _small_parts(gen, n_parts, heads, 6)
    ins = [t for p in parts for t in p[:3]]
    w = torch.randn(7, 6, generator=gen, dtype=torch.float64)
    out = dot_attention_parts(parts, 0.7, heads=heads)
    ref = _dense_union(parts, heads, 0.7)
    torch.testing.assert_close(out, ref, **TOL)
    assert (out[1] == 0).all()
    for a, b in zip(torch.autograd.grad(out, ins, w), torch.autograd.grad(ref, ins, w)):
        torch.testing.assert_close(a, b, **TOL)


def test_parts_cpu_gradcheck():
    from dgraph_amd.ops import dot_attention_parts

    parts = _small_parts(torch.Generator().manual_seed(6), 2, 2, 6)
    pats = [p[3] for p in parts]
    ins = tuple(t for p in parts for t in p[:3])
    fn = lambda *t: dot_attention_parts(  # noqa: E731
        [(t[3 * i], t[3 * i + 1], t[3 * i + 2], pats[i]) for i in range(2)], 0.7, heads=2)
    assert torch.autograd.gradcheck(fn, ins)


def test_parts_argument_checks():
    from dgraph_amd.ops import dot_attention_parts
    from dgraph_amd.ops.gat import GatPattern

    rowptr, col, _ = pattern()
    pat = GatPattern(rowptr, col, N, 0)
    short = GatPattern(rowptr[:R], col[:int(rowptr[R - 1])], N, 0)  # one row fewer
    d = case(64, 2, 0.5)
    d128 = case(128, 2, 0.5)
    q, k, v = d["q"], d["k"], d["v"]
    dot_attention_parts([(q, k, v, pat), (q, k, v, pat)], heads=2)
    with pytest.raises(ValueError):  # another row count
        dot_attention_parts([(q, k, v, pat), (q[:R - 1], k, v, short)], heads=2)
    with pytest.raises(ValueError):  # q's rows are not the pattern's
        dot_attention_parts([(q[:R - 1], k, v, pat)], heads=2)
    with pytest.raises(ValueError):  # another width in the second part
        dot_attention_parts([(q, k, v, pat), (d128["q"], d128["k"], d128["v"], pat)], heads=2)
    with pytest.raises(ValueError):  # k and q widths differ
        dot_attention_parts([(q, d128["k"], d128["v"], pat)], heads=2)
    with pytest.raises(ValueError):  # fewer source rows than the pattern's columns
        dot_attention_parts([(q, k[:LS], v[:LS], pat)], heads=2)
    with pytest.raises(ValueError):
        dot_attention_parts([(q, k, v, pat)], heads=3)
    with pytest.raises(ValueError):
        dot_attention_parts([], heads=1)


# ------------------------------------------------------------------- the layer, overlap=True
def _overlap_layer(heads, comm):
    from dgraph_amd.models.transformer_conv import CommAwareTransformerConv

    torch.manual_seed(0)
    layer = CommAwareTransformerConv(CIN, 8, comm=comm, heads=heads, hetero=True,
                                     overlap=True).double()
    with torch.no_grad():
        layer.bias.normal_()
    return layer


def _overlap_layer_dist(rank, world, heads, skew):
    import torch.distributed as dist

    from dgraph_amd import Communicator
    from dgraph_amd.comm.alltoallv import CommStats
    from dgraph_amd.data.hetero import build_relation_graph, get_vertex_offsets

    comm = Communicator.init_process_group("nccl")  # gloo underneath on the CPU
    try:
        edges = _edges(world if skew else 0)
        offs = {0: get_vertex_offsets(ND, world), 1: get_vertex_offsets(NS, world)}
        rel = build_relation_graph(edges, 1, 0, offs, rank, world)
        if skew and rank == world - 1:  # sends rows, receives none: still one exchange each way
            assert rel.num_halo == 0 and sum(rel.pattern.send_splits()) > 0
        gen = torch.Generator().manual_seed(1)
        xd = torch.randn(ND, CIN, generator=gen, dtype=torch.float64)
        xs = torch.randn(NS, CIN, generator=gen, dtype=torch.float64)
        w = torch.randn(ND, 8, generator=gen, dtype=torch.float64)
        d0, d1 = int(offs[0][rank]), int(offs[0][rank + 1])
        s0, s1 = int(offs[1][rank]), int(offs[1][rank + 1])
        layer = _overlap_layer(heads, comm)
        assert layer.overlap
        xdl = xd[d0:d1].clone().requires_grad_()
        xsl = xs[s0:s1].clone().requires_grad_()
        CommStats.reset()
        out = layer(xdl, rel, x_j=xsl)
        assert CommStats.calls == 1, CommStats.calls   # one exchange of the [k | v] rows
        assert "dot_attn_halo_plan" in rel._cache
        (out * w[d0:d1]).sum().backward()
        assert CommStats.calls == 2, CommStats.calls   # and its adjoint
        got = [p.grad.clone() for p in layer.parameters()]
        for t in got:
            dist.all_reduce(t)
        # the same layer at W = 1 on the whole graph, in this process (no exchange at all)
        one = _overlap_layer(heads, types.SimpleNamespace(get_world_size=lambda: 1))
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
def test_layer_overlap_distributed(ranks, world, heads, skew):
    ranks(_overlap_layer_dist, world, heads, skew)
