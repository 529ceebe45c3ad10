"""The fused softmax aggregation kernels (csrc/kernels/spmm_softmax.hip, through
``K.segment_softmax`` / ``K.segment_softmax_bwd``), ``softmax_aggregate``,
``dist_softmax_aggregate`` and ``CommAwareGENConv`` on the GPU against the fp64 evaluation of
their contract (tests/test_softmax_aggr.py: ``softmax_contract`` / ``softmax_bwd_contract``,
one row at a time).

Inputs: the skewed CSR (300 rows over 257 columns, Poisson(7) degrees, row 0 with 5,000
entries, row 150 empty, rows 1 / 2 of degree 1 / 2) with ``x = randn``, and ``100 + randn``
with ``t = +-2`` (``exp(200)`` is infinite in fp32: tells the running maximum from a plain
``exp``).

Accuracy rule: ``|kernel - fp64| <= test_gat_kernels.bound(ref64, ref32)`` with ``ref32`` the
same contract in fp32 on the CPU; nothing is taken from the kernel's own output. ``lse`` is
compared on the non-empty rows (the empty row must hold ``-inf``). The backward kernel is
given the forward kernel's ``(out, lse)``. Largest ``error / bound`` seen on an MI355X (a
record, not an input to the bound; every figure is printed before it is asserted):

    forward, t = 1        out 0.129 (F = 172: err 1.2e-5, bound 9.2e-5)   lse 0.049
                          out of the degree-1 row 0.000 (exact)
    100 + randn, t = +-2  out 0.013 (err 7.7e-5, bound 5.9e-3)   lse 0.002
    per-channel t         out 0.024   lse 0.007   dx 0.022   dt 0.005
    column blocks         out 0.029   lse 0.013   dx 0.006
    two sources           out 0.026   lse 0.019   the row pass 1 left empty 0.000
    backward              dx 0.009   dt 0.021 (F = 1)
    split patterns        dx 0.027   dt 0.006
    op, scalar t          out 0.034   dx 0.007   dt 0.031
    W = 2 op              out 0.013   dx 0.018   dt 0.003
    W = 2 layer           out 0.006   dx 0.009   every parameter gradient <= 0.013

The fp32 contract sums one entry at a time (test_pna._sum_rows), so the bounds are those of a
plain fp32 evaluation.
"""
from __future__ import annotations

import dataclasses
import functools

import pytest
import torch

from conftest import rank_device, run_ranks
from dgraph_amd.ops import kernels as K
from dgraph_amd.ops.aggregate import softmax_aggregate
from test_gat_kernels import bound
from test_pna import skewed_csr, values
from test_softmax_aggr import (SPLIT, softmax_bwd_contract, softmax_contract, split_csr,
                               two_pass)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.25e9  # what output buffers hold outside the blocks the kernel may write
NINF = float("-inf")
RATIOS: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(RATIOS):
        print(f"\n[softmax] largest error / bound, {k}: {RATIOS[k]:.3f}", end="")


def within(tag, name, got, ref64, ref32):
    """|got - fp64| against :func:`bound`; prints the figures, records the ratio."""
    got = got.detach().cpu().double()
    assert bool(torch.isfinite(got).all()), f"{tag} {name}: not finite"
    err = float((got - ref64.double()).abs().max()) if got.numel() else 0.0
    bd = bound(ref64, ref32)
    print(f"{tag} {name}: err {err:.3e} bound {bd:.3e} ratio {err / bd:.3f}")
    key = f"{tag.split('[')[0]} {name}"
    RATIOS[key] = max(RATIOS.get(key, 0.0), err / bd)
    assert err <= bd, f"{tag} {name}: error {err:.3e} above the bound {bd:.3e}"


def check_fwd(tag, out, lse, r64, r32, ne):
    """``out`` everywhere, ``lse`` on the non-empty rows ``ne``; the others: 0 and -inf."""
    within(tag, "out", out, r64[0], r32[0])
    within(tag, "lse", lse[ne.to(lse.device)], r64[1][ne], r32[1][ne])
    e = (~ne).to(out.device)
    assert torch.count_nonzero(out[e]) == 0 and bool((lse[e] == NINF).all())


def temperature(kind, F):
    if kind == "one":
        return torch.ones(F)
    t = torch.linspace(-3.0, 3.0, F)
    t[F // 3] = 0.0
    return t


@functools.lru_cache(maxsize=None)
def fwd_refs(F, tkind="one", xkind="plain", tscale=1.0):
    """(x, t, fp64 (out, lse), fp32 (out, lse)) of the skewed case, shared by the index
    widths and by the backward tests."""
    csr = skewed_csr()
    x = values("plain", 257, F, F)
    if xkind == "offset":
        x = 100.0 + x
    t = temperature(tkind, F) * tscale
    r64 = softmax_contract(csr.rowptr, csr.col, x, t)
    r32 = softmax_contract(csr.rowptr, csr.col, x, t, dtype=torch.float32)
    return x, t, r64, r32


def run_fwd(csr, x, t):
    R, F = csr.num_rows, x.shape[1]
    out = torch.full((R, F), SENT, device=x.device)
    lse = torch.full((R, F), SENT, device=x.device)
    return K.segment_softmax(csr.rowptr, csr.col, x, t, out, lse)


NE = skewed_csr().degree() > 0


@pytest.mark.parametrize("F", [1, 3, 4, 64, 172, 600])
@pytest.mark.parametrize("idx", [torch.int32, torch.int64])
def test_forward(F, idx):
    x, t, r64, r32 = fwd_refs(F)
    csr = skewed_csr(idx).to(DEV)
    out, lse = run_fwd(csr, x.to(DEV), t.to(DEV))
    check_fwd(f"fwd[F={F}]", out, lse, r64, r32, NE)
    assert not bool(NE[150])  # the empty row: checked by check_fwd (0 and -inf)
    src = x[skewed_csr().col[skewed_csr().rowptr[1]].long()]
    within(f"fwd[F={F}]", "out of the degree-1 row", out[1], src.double(), src)


@pytest.mark.parametrize("tscale", [2.0, -2.0])
def test_no_overflow_without_max_subtraction(tscale):
    """``x = 100 + randn`` at ``t = +-2``, F = 24: ``exp(+-200)`` overflows / underflows in
    fp32; the result and ``lse`` are finite and within the bound."""
    x, t, r64, r32 = fwd_refs(24, "one", "offset", tscale)
    csr = skewed_csr(torch.int32).to(DEV)
    out, lse = run_fwd(csr, x.to(DEV), t.to(DEV))
    check_fwd(f"offset[t={tscale:+.0f}]", out, lse, r64, r32, NE)


def bwd_case(csr, tcsr, x, t, r64, r32, seed):
    """(g, fp64 (dx, dt), fp32 (dx, dt)) over the transposed pattern ``tcsr`` (any subset of
    ``csr``'s entries), each dtype with its own forward."""
    g = values("plain", csr.num_rows, x.shape[1], seed)
    d64 = softmax_bwd_contract(tcsr.rowptr, tcsr.col, x, t, g, *r64)
    d32 = softmax_bwd_contract(tcsr.rowptr, tcsr.col, x, t, g, *r32, dtype=torch.float32)
    return g, d64, d32


@functools.lru_cache(maxsize=None)
def bwd_refs(F, tkind="one"):
    x, t, r64, r32 = fwd_refs(F, tkind)
    csr = skewed_csr()
    return bwd_case(csr, csr.transpose(), x, t, r64, r32, 1000 + F)


def check_bwd(tag, tcsr, x, t, g, out, lse, d64, d32):
    """The backward kernel on the device pattern ``tcsr`` with the forward KERNEL's
    ``(out, lse)``: dx, the summed dt partials, and ``want_dt=False``."""
    C, F = tcsr.num_rows, x.shape[1]
    dx, part = K.segment_softmax_bwd(tcsr.rowptr, tcsr.col, x, t, g, out, lse)
    P = K._native.ops().segment_softmax_dt_parts(C)
    assert part.shape == (P, F) and P >= 1
    within(tag, "dx", dx, d64[0], d32[0])
    within(tag, "dt", part.double().sum(0), d64[1], d32[1])
    sent = torch.full((P, F), SENT, device=x.device)
    dx2, none = K.segment_softmax_bwd(tcsr.rowptr, tcsr.col, x, t, g, out, lse,
                                      want_dt=False, dt_partials=sent)
    assert none is None and bool((sent == SENT).all()) and torch.equal(dx2, dx)
    return dx, part


@pytest.mark.parametrize("F", [1, 4, 172])
@pytest.mark.parametrize("idx", [torch.int32, torch.int64])
def test_backward(F, idx):
    x, t, _, _ = fwd_refs(F)
    g, d64, d32 = bwd_refs(F)
    csr = skewed_csr(idx)
    xd, td = x.to(DEV), t.to(DEV)
    out, lse = run_fwd(csr.to(DEV), xd, td)
    check_bwd(f"bwd[F={F}]", csr.transpose().to(DEV), xd, td, g.to(DEV), out, lse, d64, d32)


def test_per_channel_temperature():
    """F = 64, ``t = linspace(-3, 3)`` with one element exactly 0: forward and backward."""
    x, t, r64, r32 = fwd_refs(64, "channel")
    assert bool((t == 0).any()) and bool((t < 0).any()) and bool((t > 0).any())
    g, d64, d32 = bwd_refs(64, "channel")
    csr = skewed_csr(torch.int32)
    xd, td = x.to(DEV), t.to(DEV)
    out, lse = run_fwd(csr.to(DEV), xd, td)
    check_fwd("channel t[F=64]", out, lse, r64, r32, NE)
    check_bwd("channel t[F=64]", csr.transpose().to(DEV), xd, td, g.to(DEV), out, lse, d64, d32)


@pytest.mark.parametrize("F,pad", [(3, 1), (64, 4)])
def test_operands_as_column_blocks(F, pad):
    """``x``, ``out`` and ``lse`` as column blocks at offset ``pad`` of wider sentinel-filled
    buffers (F = 3: row strides 5 and 8, no multiple of 4; F = 64: 16-B aligned blocks):
    nothing outside the blocks is written."""
    x, t, r64, r32 = fwd_refs(F)
    csr = skewed_csr(torch.int32).to(DEV)
    xw = torch.full((257, F + 2 * pad), SENT, device=DEV)
    xw[:, pad:pad + F] = x.to(DEV)
    wide = torch.full((300, 2 * F + 2 * pad), SENT, device=DEV)
    out, lse = wide[:, pad:pad + F], wide[:, pad + F:pad + 2 * F]
    K.segment_softmax(csr.rowptr, csr.col, xw[:, pad:pad + F], t.to(DEV), out, lse)
    check_fwd(f"blocks[F={F}]", out, lse, r64, r32, NE)
    assert bool((wide[:, :pad] == SENT).all()) and bool((wide[:, pad + 2 * F:] == SENT).all())
    assert not bool((wide[:, pad:pad + 2 * F] == SENT).any())
    # the backward with every operand a column block
    g, d64, d32 = bwd_refs(F)
    tc = skewed_csr(torch.int32).transpose().to(DEV)
    gw = torch.full((300, F + 2 * pad), SENT, device=DEV)
    gw[:, pad:pad + F] = g.to(DEV)
    dw = torch.full((257, F + 2 * pad), SENT, device=DEV)
    dx, _ = K.segment_softmax_bwd(tc.rowptr, tc.col, xw[:, pad:pad + F], t.to(DEV),
                                  gw[:, pad:pad + F], out, lse, dw[:, pad:pad + F])
    within(f"blocks[F={F}]", "dx", dx, d64[0], d32[0])
    assert bool((dw[:, :pad] == SENT).all()) and bool((dw[:, pad + F:] == SENT).all())


@functools.lru_cache(maxsize=None)
def split_refs(F=40):
    full, a, b = split_csr()
    x = values("plain", 257, F, 31)
    t = temperature("channel", F)
    r64 = softmax_contract(full.rowptr, full.col, x, t)
    r32 = softmax_contract(full.rowptr, full.col, x, t, dtype=torch.float32)
    return x, t, r64, r32


@pytest.mark.parametrize("row_map", [False, True])
@pytest.mark.parametrize("idx", [torch.int32, torch.int64])
def test_two_sources_match_the_unsplit_csr(idx, row_map):
    """Pass 1 over columns < 130, pass 2 (carry mode) over the rest, over all rows or
    row-compacted: the fp64 contract on the unsplit CSR within the bound; rows without an
    entry in the second block are bitwise those of pass 1."""
    x, t, r64, r32 = split_refs()
    full, a, b = split_csr(idx)
    out, lse, o1, l1 = two_pass(a.to(DEV), b.to(DEV), x.to(DEV), t.to(DEV), row_map)
    ne = full.degree() > 0
    check_fwd("two sources", out, lse, r64, r32, ne)
    absent = (b.degree() == 0).to(DEV)
    assert int(absent.sum()) > 1 and bool(absent[2]) and bool(absent[150])
    assert torch.equal(out[absent], o1[absent]) and torch.equal(lse[absent], l1[absent])
    assert torch.count_nonzero(o1[1]) == 0 and bool((l1[1] == NINF).all())  # empty, then filled
    within("two sources", "out of the row pass 1 left empty", out[1], x[200].double(), x[200])


def test_backward_on_the_split_patterns():
    """The backward on the first block's and on the second block's transposed pattern with
    the final ``(out, lse)`` of the two-pass forward kernel: ``dx`` of the sources of each
    block and the two parts of ``dt`` match the contract restricted to each edge set."""
    x, t, r64, r32 = split_refs()
    full, a, b = split_csr(torch.int32)
    xd, td = x.to(DEV), t.to(DEV)
    out, lse, _, _ = two_pass(a.to(DEV), b.to(DEV), xd, td)
    for name, blk, xs in (("interior", a, x[:SPLIT]), ("halo", b, x[SPLIT:])):
        tc = blk.transpose()
        g, d64, d32 = bwd_case(full, tc, xs, t, r64, r32, 77)
        assert tc.num_rows == xs.shape[0]
        check_bwd(f"split bwd[{name}]", tc.to(DEV), xs.contiguous().to(DEV), td, g.to(DEV),
                  out, lse, d64, d32)


def test_bitwise_deterministic():
    csr = skewed_csr(torch.int32, seed=9).to(DEV)
    x = values("plain", 257, 172, 9).to(DEV)
    gy = values("plain", 300, 172, 10).to(DEV)
    res = []
    for _ in range(2):
        xi = x.clone().requires_grad_()
        ti = temperature("channel", 172).to(DEV).requires_grad_()
        out = softmax_aggregate(xi, csr, ti)
        out.backward(gy)
        res.append((out.detach(), xi.grad, ti.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_op_with_a_learnable_scalar_temperature():
    """``softmax_aggregate`` with a ``requires_grad`` scalar ``t`` (F = 64): out, dx and the
    scalar's gradient (the sum of the per-channel one)."""
    x, _, _, _ = fwd_refs(64)
    csr = skewed_csr(torch.int32)
    gy = values("plain", 300, 64, 5)
    refs = []
    for dt in (torch.float64, torch.float32):
        xr = x.to(dt).clone().requires_grad_()  # a copy: x is the cached case's tensor
        tr = torch.tensor([0.7], dtype=dt, requires_grad=True)
        o, _ = softmax_contract(csr.rowptr, csr.col, xr, tr, dtype=dt)
        refs.append((o.detach(),) + torch.autograd.grad((o * gy.to(dt)).sum(), (xr, tr)))
    xi = x.clone().to(DEV).requires_grad_()
    ti = torch.tensor([0.7], device=DEV, requires_grad=True)
    out = softmax_aggregate(xi, csr.to(DEV), ti)
    out.backward(gy.to(DEV))
    assert ti.grad.shape == (1,)
    for name, got, i in (("out", out, 0), ("dx", xi.grad, 1), ("dt", ti.grad, 2)):
        within("op, scalar t", name, got, refs[0][i], refs[1][i])


def test_contract_checks_raise():
    csr = skewed_csr(torch.int32).to(DEV)
    x = values("plain", 257, 8, 1).to(DEV)
    t = torch.ones(8, device=DEV)
    new = lambda F=8, dt=torch.float32: torch.empty(300, F, dtype=dt, device=DEV)  # noqa: E731
    call = lambda xx, tt, o, l, **kw: K.segment_softmax(  # noqa: E731
        csr.rowptr, csr.col, xx, tt, o, l, **kw)
    err = (RuntimeError, ValueError, TypeError)
    with pytest.raises(err):  # non-fp32 input on the GPU
        call(x.double(), t.double(), new(dt=torch.float64), new(dt=torch.float64))
    with pytest.raises(err):
        call(x.half(), t.half(), new(dt=torch.float16), new(dt=torch.float16))
    with pytest.raises(err):
        call(x, t, new(), new(dt=torch.float16))
    with pytest.raises(err):  # a t of the wrong length
        call(x, torch.ones(7, device=DEV), new(), new())
    with pytest.raises(err):
        K._native.ops().segment_softmax_fwd(csr.rowptr, csr.col, x, torch.ones(12, device=DEV),
                                            new(), new(), False, None)
    with pytest.raises(err):  # a misaligned VEC-4 block: row stride / base
        call(torch.empty(257, 10, device=DEV)[:, :8], t, new(), new())
    with pytest.raises(err):
        call(x, t, new(), torch.empty(300, 10, device=DEV)[:, 1:9])
    with pytest.raises(err):
        call(x, torch.ones(9, device=DEV)[1:], new(), new())
    with pytest.raises(err):  # a column stride
        call(x.t().contiguous().t(), t, new(), new())
    with pytest.raises(err):  # outputs with fewer rows than the CSR
        call(x, t, new()[:100], new()[:100])
    with pytest.raises(err):  # carry mode without an incumbent
        K.segment_softmax(csr.rowptr, csr.col, x, t, second=True)
    tc = skewed_csr(torch.int32).transpose().to(DEV)
    out, lse = call(x, t, new(), new())
    g = new()
    with pytest.raises(err):  # x narrower than the gradient
        K.segment_softmax_bwd(tc.rowptr, tc.col, x[:, :4].contiguous(), t[:4], g, out, lse)
    with pytest.raises(err):  # a partial buffer of the wrong row count
        K.segment_softmax_bwd(tc.rowptr, tc.col, x, t, g, out, lse,
                              dt_partials=torch.empty(1, 8, device=DEV))
    with pytest.raises(err):  # fewer lse rows than g rows
        K.segment_softmax_bwd(tc.rowptr, tc.col, x, t, g, out, lse[:100])
    # empty launches return without launching
    empty = skewed_csr(torch.int32).to(DEV)
    none_rp = torch.zeros(1, dtype=torch.long, device=DEV)
    none_col = torch.zeros(0, dtype=torch.int32, device=DEV)
    o, l = K.segment_softmax(none_rp, none_col, x, t)
    assert o.shape == (0, 8) and empty.num_rows == 300
    dx, part = K.segment_softmax_bwd(none_rp, none_col, x[:0], t, g, out, lse)
    assert dx.shape == (0, 8) and part.shape == (0, 8)
    rp0 = torch.zeros(258, dtype=torch.long, device=DEV)
    dx, part = K.segment_softmax_bwd(rp0, none_col, x, t, g[:0], out[:0], lse[:0])
    assert torch.count_nonzero(dx) == 0 and torch.count_nonzero(part) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ op and layer, W = 2
def _tiny_shape():
    from dgraph_amd.data.synthetic import SHAPES

    return dataclasses.replace(SHAPES["ogbn-arxiv"], name="tiny-64", num_nodes=64,
                               num_directed_edges=400)


def _cpu_single_rank(fn, shape, dev):
    """``fn(dtype, graph, slice, device)`` on the whole graph on the CPU in fp64 and in fp32.
    The graph is generated on ``dev`` like the ranks' parts (the synthetic generator draws
    from the device's random stream: a CPU-built graph is another graph) and moved over."""
    from dgraph_amd.data.synthetic import build_partition
    from dgraph_amd.parallel.dist_graph import DistGraph

    p = build_partition(shape, 0, 1, dev)
    g1 = DistGraph(p["csr"].to("cpu"), p["L"], 0)
    return [fn(dt, g1, slice(0, shape.num_nodes), "cpu") for dt in (torch.float64, torch.float32)]


def _rank_graph(shape, rank, world, dev):
    from dgraph_amd.data.synthetic import build_partition
    from dgraph_amd.parallel.dist_graph import DistGraph

    p = build_partition(shape, rank, world, dev)
    g = DistGraph(p["csr"], p["L"], p["H"], p["send_local_idx"], p["send_splits"],
                  p["recv_splits"])
    return g, slice(p["offsets"][rank], p["offsets"][rank + 1])


def _w2_op_body(rank, world):
    import torch.distributed as dist

    import test_softmax_aggr as D
    from dgraph_amd.parallel.dist_graph import dist_softmax_aggregate

    shape = _tiny_shape()

    def run(dt, graph, sl, dev):
        x, gy, t = D._global_inputs(dt, dev, shape)
        xl, t = x[sl].clone().requires_grad_(), t.requires_grad_()
        out = dist_softmax_aggregate(xl, graph, t)
        out.backward(gy[sl])
        return out.detach(), xl.grad, t.grad

    dev = rank_device()
    r64, r32 = _cpu_single_rank(run, shape, dev)
    graph, sl = _rank_graph(shape, rank, world, dev)
    out, dx, gt = run(torch.float32, graph, sl, dev)
    dist.all_reduce(gt)
    within("W=2 op", "out", out, r64[0][sl], r32[0][sl])
    within("W=2 op", "dx", dx, r64[1][sl], r32[1][sl])
    within("W=2 op", "dt", gt, r64[2], r32[2])


def _w2_layer_body(rank, world):
    import torch.distributed as dist

    import test_softmax_aggr as D

    shape = _tiny_shape()
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(shape.num_nodes, D.LF, generator=gen)
    gy = torch.randn(shape.num_nodes, D.LOUT, generator=gen)

    def run(dt, graph, sl, dev):
        layer = D.make_layer().to(device=dev, dtype=dt)
        xl = x[sl].to(device=dev, dtype=dt).requires_grad_()
        out = layer(xl, graph)
        (out * gy[sl].to(device=dev, dtype=dt)).sum().backward()
        return out.detach(), xl.grad, {n: q.grad for n, q in layer.named_parameters()}

    dev = rank_device()
    r64, r32 = _cpu_single_rank(run, shape, dev)
    graph, sl = _rank_graph(shape, rank, world, dev)
    out, dx, grads = run(torch.float32, graph, sl, dev)
    within("W=2 layer", "out", out, r64[0][sl], r32[0][sl])
    within("W=2 layer", "dx", dx, r64[1][sl], r32[1][sl])
    for n, gq in grads.items():
        dist.all_reduce(gq)
        within("W=2 layer", f"grad {n}", gq, r64[2][n], r32[2][n])
    assert float(grads["t"].abs().max()) > 0


def _w2_body(rank, world):
    from dgraph_amd.comm.rccl_exec import RCCLExecutor

    _w2_op_body(rank, world)
    _w2_layer_body(rank, world)
    torch.cuda.synchronize()
    RCCLExecutor.close_all()


def test_op_and_layer_two_ranks_rccl():
    """At W = 2 over real RCCL (both ranks on GPU 0, a 64-vertex graph, one process group for
    both): dist_softmax_aggregate forward, dx and the all-reduced dt against the CPU fp64
    result, then CommAwareGENConv against the same layer on the CPU in fp64, every parameter
    gradient (the temperature's included) after the all-reduce."""
    run_ranks(_w2_body, 2, backend="rccl-one-gpu")
