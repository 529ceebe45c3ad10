"""Attention dropout in the fused dot-product attention: the Philox4x32-10 keep-mask generator
(``csrc/kernels/philox.h`` on the host against ``dgraph_amd/ops/philox.py``), the contract of
the three kernels of csrc/kernels/dot_attn_drop_f32.hip written out per edge, the CPU path of
``dot_attention(..., dropout_p=, dropout_seed=)`` and ``CommAwareTransformerConv(dropout=)``
(tests/test_dot_attn_drop_gpu.py imports the contract, the dense evaluation and the seed from
here).

Pattern and inputs are those of tests/test_dot_attn.py (37 rows over 41 local + 19 halo
sources, degrees 0, 1, LPR +- 1 and a 301-entry hub; score scales 0.5 and 40). The keep mask
is a deterministic function of ``(seed, CSR slot, head)``, so every comparison here is exact
at fp64 (1e-10), none statistical. ``SEED`` was searched on the CPU so that, at 1, 2, 4 and 8
heads and at p = 0.1 and 0.5, the mask on that pattern has a degree-1 row that is dropped and
one that is kept, a hub with kept and dropped edges in every head and, at p = 0.5, a row of
two or more edges that are all dropped; ``test_seed_conditions`` asserts them.

:func:`dense_dropout_attention` is the independent evaluation: per head the dense no-dropout
softmax matrix of the rows over the pattern's entries (``[R, E]``: the pattern has repeated
``(row, column)`` pairs, which a ``[R, N]`` matrix cannot hold apart, and the mask is per
entry), times the keep mask laid out on the same ``[R, E]`` grid, divided by ``1 - p``, times
the entries' ``v`` rows. It uses ``torch.softmax`` and matrix products only and shares no code
with ``ops/dot_attn.py`` or with :func:`drop_contract`.
"""
from __future__ import annotations

import functools
import math

import pytest
import torch

from test_dot_attn import CIN, ND, NS, TOL, _edges, case, dot_attn_contract
from test_gat_kernels import HS, LS, N, R, pattern

SEED = 83
PS = [0.1, 0.5]
DROP_OUTPUTS = ("out", "stat_m", "stat_l", "dq", "dk", "dv")

KNOWN = [
    ("00000000 00000000 00000000 00000000", "00000000 00000000",
     "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff",
     "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0",
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


def _words(s):
    return torch.tensor([int(w, 16) for w in s.split()], dtype=torch.int64)


def keep_mask(heads: int, p: float, seed: int = SEED) -> torch.Tensor:
    """keep [E, heads] of ``pattern()``'s entries."""
    from dgraph_amd.ops.philox import attn_keep_mask

    return attn_keep_mask(seed, pattern()[1].numel(), heads, p)


# ---------------------------------------------------------------------------- the generator
def test_philox_known_answers():
    from dgraph_amd.ops.philox import philox4x32_10

    for ctr, key, want in KNOWN:
        assert torch.equal(philox4x32_10(_words(ctr), _words(key)), _words(want))
    # batched: the three at once
    got = philox4x32_10(torch.stack([_words(c) for c, _, _ in KNOWN]),
                        torch.stack([_words(k) for _, k, _ in KNOWN]))
    assert torch.equal(got, torch.stack([_words(w) for _, _, w in KNOWN]))


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("heads", [1, 4, 8])
@pytest.mark.parametrize("first,count", [(0, 4096), (2 ** 32 - 8, 16)],
                         ids=["low", "high-word carry"])
@pytest.mark.parametrize("seed", [0, 1, 2 ** 62 - 1])
def test_host_mask_equals_torch_mask(seed, first, count, heads, p):
    from dgraph_amd import _native
    from dgraph_amd.ops.philox import attn_keep_mask

    assert _native.load(), "native library missing"
    host = _native.ops().attn_keep_mask_host(seed, count, heads, p, first)
    ours = attn_keep_mask(seed, count, heads, p, first_slot=first)
    assert host.dtype == torch.bool and host.shape == (count, heads)
    assert torch.equal(host, ours)
    assert torch.equal(attn_keep_mask(torch.tensor([seed]), count, heads, p, first_slot=first),
                       ours)  # the seed as the 1-element tensor the op takes


def test_first_slot_is_an_offset_and_p0_keeps_everything():
    from dgraph_amd import _native
    from dgraph_amd.ops.philox import attn_keep_mask

    full = attn_keep_mask(5, 64, 8, 0.5)
    assert torch.equal(attn_keep_mask(5, 24, 8, 0.5, first_slot=40), full[40:])
    assert attn_keep_mask(5, 4096, 8, 0.0).all()
    assert _native.ops().attn_keep_mask_host(5, 4096, 8, 0.0).all()
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError):
            attn_keep_mask(5, 4, 1, bad)
        with pytest.raises(RuntimeError):
            _native.ops().attn_keep_mask_host(5, 4, 1, bad)


@pytest.mark.parametrize("p", PS)
def test_keep_rate(p):
    """Over n = 2^20 slots x 4 heads the keep rate lies within 5 sigma of ``1 - thr / 2^32``,
    sigma = sqrt(p (1 - p) / n) (a fixed seed: deterministic)."""
    from dgraph_amd.ops.philox import attn_keep_mask, keep_threshold

    keep = attn_keep_mask(SEED, 2 ** 20, 4, p)
    n = keep.numel()
    rate = float(keep.double().mean())
    want = 1.0 - keep_threshold(p) / 2 ** 32
    sigma = math.sqrt(p * (1 - p) / n)
    print(f"p={p}: keep rate {rate:.6f}, expected {want:.6f}, {abs(rate - want) / sigma:.2f} sigma")
    assert abs(rate - want) <= 5 * sigma
    for h in range(4):  # and per head (n / 4 draws each)
        assert abs(float(keep[:, h].double().mean()) - want) <= 5 * 2 * sigma


@pytest.mark.parametrize("p", PS)
def test_masks_of_seeds_and_heads_are_independent(p):
    """Two seeds, and heads 0 and 4 of one seed (the two Philox calls of an 8-head edge),
    agree on a share of the slots within 5 sigma of the independent ``p^2 + (1 - p)^2``."""
    from dgraph_amd.ops.philox import attn_keep_mask

    n = 2 ** 18
    a, b = attn_keep_mask(SEED, n, 8, p), attn_keep_mask(SEED + 1, n, 8, p)
    want = p * p + (1 - p) * (1 - p)
    sigma = math.sqrt(want * (1 - want) / n)
    for name, x, y in (("seeds", a[:, 0], b[:, 0]), ("heads 0 / 4", a[:, 0], a[:, 4]),
                       ("heads 0 / 1", a[:, 0], a[:, 1])):
        agree = float((x == y).double().mean())
        print(f"p={p} {name}: agree {agree:.5f}, independent {want:.5f}, "
              f"{abs(agree - want) / sigma:.2f} sigma")
        assert abs(agree - want) <= 5 * sigma, name


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("heads", [1, 2, 4, 8])
def test_seed_conditions(heads, p):
    rowptr, _, rows = pattern()
    deg = rowptr[1:] - rowptr[:-1]
    keep = keep_mask(heads, p)
    kept = torch.zeros(R, heads, dtype=torch.long).index_add(0, rows, keep.long())
    one = kept[deg == 1]
    assert (one == 0).any() and (one == 1).any()      # a degree-1 row dropped, one kept
    hub = kept[deg == 301]
    assert ((hub > 0) & (hub < 301)).all()            # the hub: both, in every head
    if p == 0.5:
        assert (kept[deg >= 2] == 0).any()            # every edge of a longer row dropped


# ------------------------------------------------------------------------------ the contract
def dense_dropout_attention(rowptr, col, q, ka, va, heads, scale, keep, p):
    """``out [R, C]``: softmax matrix x keep mask / (1 - p) x v, dense over [R, E]
    (differentiable; the module docstring)."""
    nr, C = q.shape
    D = C // heads
    E = col.numel()
    rows = torch.repeat_interleave(torch.arange(nr), rowptr[1:] - rowptr[:-1])
    member = torch.zeros(nr, E, dtype=torch.bool)
    member[rows, torch.arange(E)] = True
    outs = []
    for h in range(heads):
        sl = slice(h * D, (h + 1) * D)
        score = (q[:, sl] @ ka[col][:, sl].T) * scale                       # [R, E]
        score = torch.where(member, score, torch.full_like(score, -float("inf")))
        alpha = torch.softmax(score, 1)
        alpha = torch.where(member, alpha, torch.zeros_like(alpha))         # (empty rows: nan)
        w = alpha * (member & keep[:, h][None, :]).to(alpha.dtype) / (1.0 - p)
        outs.append(w @ va[col][:, sl])
    return torch.cat(outs, 1)


def drop_contract(C, heads, s, p, dtype=torch.float64, seed=SEED, c=None):
    """What dot_attn_drop_fwd / _bwd_dst / _bwd_src compute on ``case(C, heads, s)``, per edge,
    in ``dtype``: the no-dropout ``alpha``, ``stat_m``, ``stat_l`` of ``dot_attn_contract``,
    then ``mm = keep / (1 - p)`` (in fp32: the fp32 quotient the kernels are handed)."""
    rowptr, col, rows = pattern()
    d = case(C, heads, s)
    base = dot_attn_contract(rowptr, col, d["q"], d["k"], d["v"], None, None, N, d["g"], heads,
                             d["scale"], 0.0, None, dtype=dtype)
    cv = lambda t: t.to(dtype)  # noqa: E731
    D, E = C // heads, col.numel()
    inv_keep = torch.tensor(1.0, dtype=dtype) / (torch.tensor(1.0, dtype=dtype) -
                                                 torch.tensor(p, dtype=dtype))
    mm = keep_mask(heads, p, seed).to(dtype) * inv_keep                     # [E, heads]
    alpha = base["alpha"]
    qe, ge = cv(d["q"])[rows].view(E, heads, D), cv(d["g"])[rows].view(E, heads, D)
    ke, ve = cv(d["k"])[col].view(E, heads, D), cv(d["v"])[col].view(E, heads, D)
    am = alpha * mm
    res = {"stat_m": base["stat_m"], "stat_l": base["stat_l"], "alpha": alpha, "mm": mm}
    res["out"] = torch.zeros(R, C, dtype=dtype).index_add(
        0, rows, (am.unsqueeze(-1) * ve).reshape(E, C))
    ga = (ge * ve).sum(-1)
    cc = torch.zeros(R, heads, dtype=dtype).index_add(0, rows, am * ga) if c is None else cv(c)
    de = alpha * (mm * ga - cc[rows])
    res["c"] = cc
    res["dq"] = d["scale"] * torch.zeros(R, C, dtype=dtype).index_add(
        0, rows, (de.unsqueeze(-1) * ke).reshape(E, C))
    res["dk"] = d["scale"] * torch.zeros(N, C, dtype=dtype).index_add(
        0, col, (de.unsqueeze(-1) * qe).reshape(E, C))
    res["dv"] = torch.zeros(N, C, dtype=dtype).index_add(
        0, col, (am.unsqueeze(-1) * ge).reshape(E, C))
    return res


@functools.lru_cache(maxsize=None)
def drop_oracle(C: int, heads: int, s: float, p: float):
    """(fp64, fp32) results of :func:`drop_contract`; computed once and shared."""
    return drop_contract(C, heads, s, p), drop_contract(C, heads, s, p, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def dense_reference(C: int, heads: int, s: float, p: float):
    """out and the gradients of the dense evaluation by ``torch.autograd`` at fp64."""
    rowptr, col, _ = pattern()
    d = case(C, heads, s)
    q, k, v = (d[n].double().requires_grad_() for n in ("q", "k", "v"))
    out = dense_dropout_attention(rowptr, col, q, k, v, heads, d["scale"], keep_mask(heads, p), p)
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), d["g"].double())
    return {"out": out.detach(), "dq": dq, "dk": dk, "dv": dv}


CASES = [(64, 1, 0.5), (64, 8, 40.0), (128, 4, 0.5), (256, 2, 0.5)]


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("C,heads,s", CASES)
def test_drop_contract_matches_dense_autograd(C, heads, s, p):
    """The per-edge contract the GPU tests compare the kernels with is the dense evaluation
    and its autograd; ``c`` is the delta of the dropped-out output; a row with every edge
    dropped gives out = 0, c = 0 and no gradient to q."""
    ref, want = drop_oracle(C, heads, s, p)[0], dense_reference(C, heads, s, p)
    for name in ("out", "dq", "dk", "dv"):
        torch.testing.assert_close(ref[name], want[name], **TOL)
    g = case(C, heads, s)["g"].double()
    torch.testing.assert_close(ref["c"], (g * ref["out"]).view(R, heads, -1).sum(-1), **TOL)
    rows = pattern()[2]
    kept = torch.zeros(R, heads).index_add(0, rows, (ref["mm"] > 0).float())
    dead = (kept == 0).repeat_interleave(C // heads, 1)
    assert (ref["out"][dead] == 0).all() and (ref["c"][kept == 0] == 0).all()
    assert (ref["dq"][dead] == 0).all()


@pytest.mark.parametrize("two_sources", [False, True])
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("C,heads,s", CASES)
def test_op_cpu_matches_dense(C, heads, s, p, two_sources):
    from dgraph_amd.ops import dot_attention
    from dgraph_amd.ops.gat import GatPattern

    rowptr, col, _ = pattern()
    d = case(C, heads, s)
    ns, nh = (LS, HS) if two_sources else (N, 0)
    pat = GatPattern(rowptr, col, ns, nh)
    mk = lambda t: t.double().clone().requires_grad_()  # noqa: E731
    q, k, v = mk(d["q"]), mk(d["k"][:ns]), mk(d["v"][:ns])
    kh, vh = (mk(d["k"][ns:]), mk(d["v"][ns:])) if two_sources else (None, None)
    seed = torch.tensor([SEED])
    out = dot_attention(q, k, v, pat, kh, vh, heads=heads, dropout_p=p, dropout_seed=seed)
    ins = [t for t in (q, k, v, kh, vh) if t is not None]
    grads = torch.autograd.grad(out, ins, d["g"].double())
    want = dense_reference(C, heads, s, p)
    torch.testing.assert_close(out.detach(), want["out"], **TOL)
    torch.testing.assert_close(grads[0], want["dq"], **TOL)
    if two_sources:  # dq, dk, dv, dkh, dvh
        torch.testing.assert_close(torch.cat([grads[1], grads[3]]), want["dk"], **TOL)
        torch.testing.assert_close(torch.cat([grads[2], grads[4]]), want["dv"], **TOL)
    else:
        torch.testing.assert_close(grads[1], want["dk"], **TOL)
        torch.testing.assert_close(grads[2], want["dv"], **TOL)
    assert dot_attention(d["q"], d["k"], d["v"], GatPattern(rowptr, col, N, 0), heads=heads,
                         dropout_p=p, dropout_seed=seed).dtype == torch.float32


def test_seeds_and_defaults():
    from dgraph_amd.ops import dot_attention
    from dgraph_amd.ops.gat import GatPattern

    rowptr, col, _ = pattern()
    d = case(64, 2, 0.5)
    pat = GatPattern(rowptr, col, N, 0)
    q, k, v = d["q"].double(), d["k"].double(), d["v"].double()
    run = lambda **kw: dot_attention(q, k, v, pat, heads=2, **kw)  # noqa: E731
    a = run(dropout_p=0.5, dropout_seed=torch.tensor([1]))
    b = run(dropout_p=0.5, dropout_seed=torch.tensor([2]))
    assert torch.equal(a, run(dropout_p=0.5, dropout_seed=torch.tensor([1])))
    assert not torch.equal(a, b)
    plain = run()
    assert torch.equal(run(dropout_p=0.0, dropout_seed=torch.tensor([1])), plain)
    assert torch.equal(run(dropout_p=0.0), plain)
    assert not torch.equal(a, plain)
    # no seed: drawn from the torch generator, reproducible under torch.manual_seed
    torch.manual_seed(11)
    c1, c2 = run(dropout_p=0.5), run(dropout_p=0.5)
    torch.manual_seed(11)
    assert torch.equal(run(dropout_p=0.5), c1) and not torch.equal(c1, c2)


def test_op_dropout_argument_checks():
    from dgraph_amd.ops import dot_attention
    from dgraph_amd.ops.gat import GatPattern

    rowptr, col, _ = pattern()
    d = case(64, 2, 0.5)
    pat = GatPattern(rowptr, col, N, 0)
    run = lambda **kw: dot_attention(d["q"], d["k"], d["v"], pat, heads=2, **kw)  # noqa: E731
    for p in (1.0, -0.25, 1.5):
        with pytest.raises(ValueError, match="dropout_p"):
            run(dropout_p=p)
    with pytest.raises(ValueError, match="edge"):
        run(dropout_p=0.5, edge=torch.zeros(col.numel(), 64))
    for seed in (torch.tensor([1, 2]), torch.tensor([1], dtype=torch.int32),
                 torch.tensor([1.0]), torch.tensor([1], device="meta"), 7):
        with pytest.raises(ValueError, match="dropout_seed"):
            run(dropout_p=0.5, dropout_seed=seed)
    run(dropout_p=0.0, dropout_seed="ignored")  # p = 0: the seed is not looked at


# --------------------------------------------------------------------------------- the layer
def _layer(heads, comm=None, **kw):
    from dgraph_amd.models.transformer_conv import CommAwareTransformerConv

    torch.manual_seed(0)
    layer = CommAwareTransformerConv(CIN, 8, comm=comm, heads=heads, hetero=True, **kw).double()
    with torch.no_grad():
        layer.bias.normal_()
    return layer


def layer_pieces_dense(layer, xd, xs, pat, seed: int, kh_rows=None):
    """The layer's own projections, the dense evaluation over its pattern with the mask of
    ``seed``, its skip and bias. ``kh_rows``: the received ``[k | v]`` halo rows."""
    from dgraph_amd.ops.philox import attn_keep_mask

    H, C = layer.heads, layer.out_channels
    q, kv = layer.lin_query(xd), layer.lin_kv(xs)
    if kh_rows is not None:
        kv = torch.cat([kv[:pat.nsplit], kh_rows])
    rowptr, col = pat.rowptr.cpu(), pat.col.long().cpu()
    keep = attn_keep_mask(seed, col.numel(), H, layer.dropout)
    out = dense_dropout_attention(rowptr, col, q, kv[:, :C], kv[:, C:], H,
                                  1.0 / math.sqrt(C // H), keep, layer.dropout)
    return out + layer.lin_skip(xd) + layer.bias


@pytest.mark.parametrize("heads", [1, 2])
def test_layer_training_matches_dense_and_eval_is_the_plain_layer(heads):
    from dgraph_amd.data.hetero import build_relation_graph, get_vertex_offsets

    edges = _edges()
    offs = {0: get_vertex_offsets(ND, 1), 1: get_vertex_offsets(NS, 1)}
    rel = build_relation_graph(edges, 1, 0, offs, 0, 1)
    layer, plain = _layer(heads, dropout=0.5), _layer(heads)
    assert list(layer.state_dict()) == list(plain.state_dict())
    for a, b in zip(layer.state_dict().values(), plain.state_dict().values()):
        assert torch.equal(a, b)
    torch.manual_seed(1)
    xd = torch.randn(ND, CIN, dtype=torch.float64, requires_grad=True)
    xs = torch.randn(NS, CIN, dtype=torch.float64, requires_grad=True)
    assert layer.training
    out = layer(xd, rel, x_j=xs, dropout_seed=torch.tensor([SEED]))
    ref = layer_pieces_dense(layer, xd, xs, layer._pattern(rel), SEED)
    torch.testing.assert_close(out, ref, **TOL)
    assert not torch.allclose(out, plain(xd, rel, x_j=xs))
    w = torch.randn_like(out)
    ins = [xd, xs] + list(layer.parameters())
    for a, b in zip(torch.autograd.grad((out * w).sum(), ins),
                    torch.autograd.grad((ref * w).sum(), ins)):
        torch.testing.assert_close(a, b, **TOL)
    # its own seed: from the torch generator
    torch.manual_seed(5)
    a = layer(xd, rel, x_j=xs)
    torch.manual_seed(5)
    assert torch.equal(layer(xd, rel, x_j=xs), a) and not torch.equal(layer(xd, rel, x_j=xs), a)
    # evaluation mode, and dropout = 0 in training: exactly the layer without dropout
    layer.eval()
    assert torch.equal(layer(xd, rel, x_j=xs), plain(xd, rel, x_j=xs))
    assert torch.equal(layer(xd, rel, x_j=xs, dropout_seed=torch.tensor([SEED])),
                       plain(xd, rel, x_j=xs))
    zero = _layer(heads, dropout=0.0).train()
    assert torch.equal(zero(xd, rel, x_j=xs), plain(xd, rel, x_j=xs))


def test_layer_dropout_argument_checks():
    from dgraph_amd.models.transformer_conv import CommAwareTransformerConv as Conv

    for kw in (dict(dropout=1.0), dict(dropout=-0.1), dict(dropout=0.5, overlap=True),
               dict(dropout=0.5, edge_dim=3)):
        with pytest.raises(ValueError):
            Conv(CIN, 8, heads=2, **kw)
    Conv(CIN, 8, heads=2, dropout=0.0, overlap=True, edge_dim=None)
    Conv(CIN, 8, heads=2, dropout=0.0, edge_dim=3)


RANK_MIX = 0x9E3779B97F4A7C15


def _layer_drop_dist(rank, world, heads):
    import torch.distributed as dist

    from dgraph_amd import Communicator
    from dgraph_amd.comm.alltoallv import CommStats
    from dgraph_amd.data.hetero import build_relation_graph, get_vertex_offsets
    from dgraph_amd.ops import dot_attention
    from dgraph_amd.parallel.halo import HaloExchange

    comm = Communicator.init_process_group("nccl")  # gloo underneath on the CPU
    try:
        edges = _edges()
        offs = {0: get_vertex_offsets(ND, world), 1: get_vertex_offsets(NS, world)}
        rel = build_relation_graph(edges, 1, 0, offs, rank, world)
        gen = torch.Generator().manual_seed(1)
        xd = torch.randn(ND, CIN, generator=gen, dtype=torch.float64)
        xs = torch.randn(NS, CIN, generator=gen, dtype=torch.float64)
        w = torch.randn(ND, 8, generator=gen, dtype=torch.float64)
        d0, d1 = int(offs[0][rank]), int(offs[0][rank + 1])
        s0, s1 = int(offs[1][rank]), int(offs[1][rank + 1])
        layer = _layer(heads, comm, dropout=0.5)
        assert list(layer.state_dict()) == list(_layer(heads, comm).state_dict())
        xdl = xd[d0:d1].clone().requires_grad_()
        xsl = xs[s0:s1].clone().requires_grad_()
        seed = torch.tensor([SEED])
        CommStats.reset()
        out = layer(xdl, rel, x_j=xsl, dropout_seed=seed)
        assert CommStats.calls == 1, CommStats.calls   # as without dropout: one exchange
        (out * w[d0:d1]).sum().backward()
        assert CommStats.calls == 2, CommStats.calls   # and its adjoint
        for t in [xdl, xsl] + list(layer.parameters()):
            assert t.grad is not None and torch.isfinite(t.grad).all()
        # the rank's seed: offset per rank, so equal torch seeds do not repeat the bits
        mine = layer._dropout_seed(torch.device("cpu"), seed)
        assert int(mine) == SEED + (rank * RANK_MIX) % 2 ** 62 and int(seed) == SEED
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        assert len({int(t) for t in every}) == world
        torch.manual_seed(3)  # the same torch seed on every rank: the drawn seeds still differ
        drawn = layer._dropout_seed(torch.device("cpu"))
        every = [torch.zeros_like(drawn) for _ in range(world)]
        dist.all_gather(every, drawn)
        assert len({int(t) for t in every}) == world
        # the output: the CPU op (and the dense evaluation) on the local pattern with that seed
        C, pat = layer.out_channels, layer._pattern(rel)
        with torch.no_grad():
            q, kv = layer.lin_query(xdl), layer.lin_kv(xsl)
            halo = HaloExchange(comm)(kv, rel.pattern)
            want = dot_attention(q, kv[:, :C], kv[:, C:], pat, halo[:, :C], halo[:, C:],
                                 heads=heads, dropout_p=0.5, dropout_seed=mine)
            want = want + layer.lin_skip(xdl) + layer.bias
            torch.testing.assert_close(out.detach(), want, **TOL)
            dense = layer_pieces_dense(layer, xdl, xsl, pat, int(mine), kh_rows=halo)
            torch.testing.assert_close(out.detach(), dense, **TOL)
    finally:
        comm.destroy()


@pytest.mark.parametrize("world,heads", [(2, 2), (3, 1)])
def test_layer_distributed_training_with_dropout(ranks, world, heads):
    ranks(_layer_drop_dist, world, heads)
