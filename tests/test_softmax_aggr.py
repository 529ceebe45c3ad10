"""Softmax neighbourhood aggregation and the GENConv layer on the CPU: the op against an fp64
contract written here row by row (it shares no code with ops/reference.py), its limits
(``t = 0``: mean, large ``|t|``: max / min, shift invariance), the carry mode against one
pass over the unsplit CSR, the distributed op and ``CommAwareGENConv`` at W = 2, 3 against
W = 1 / a dense evaluation."""
import copy
import functools

import pytest
import torch

from dgraph_amd.data.synthetic import SHAPES, build_partition
from dgraph_amd.ops import kernels as K
from dgraph_amd.ops.aggregate import aggregate, softmax_aggregate
from dgraph_amd.ops.csr import CSR
from dgraph_amd.parallel.dist_graph import (DistGraph, dist_aggregate,
                                            dist_softmax_aggregate)
from test_pna import _sum_rows, skewed_csr, small_csr, values


# ------------------------------------------------------------------ the contract, by rows
def softmax_contract(rowptr, col, x, t, dtype=torch.float64):
    """``(out, lse)`` of every CSR row, one row at a time, in ``dtype``: with ``s = t * v``
    over the row's gathered values ``v``, about the row maximum ``m``:
    ``out = sum exp(s - m) v / sum exp(s - m)``, ``lse = m + log sum exp(s - m)``; 0 and
    ``-inf`` for an empty row. The sums are :func:`test_pna._sum_rows` (fp32: one entry at a
    time). Differentiable in ``x`` and ``t`` in fp64."""
    x = x.to(dtype)
    F = x.shape[1]
    t = torch.as_tensor(t, dtype=dtype) if not isinstance(t, torch.Tensor) else t.to(dtype)
    t = t.reshape(-1).expand(F) if t.numel() == 1 else t
    rp = rowptr.tolist()
    outs, lses = [], []
    for r in range(len(rp) - 1):
        s, e = rp[r], rp[r + 1]
        if e == s:
            outs.append(torch.zeros(F, dtype=dtype))
            lses.append(torch.full((F,), float("-inf"), dtype=dtype))
            continue
        v = x[col[s:e].long()]
        sc = v * t
        m = sc.detach().max(0).values
        w = torch.exp(sc - m)
        l = _sum_rows(w)
        outs.append(_sum_rows(w * v) / l)
        lses.append(m + torch.log(l))
    if not outs:
        return torch.zeros(0, F, dtype=dtype), torch.zeros(0, F, dtype=dtype)
    return torch.stack(outs), torch.stack(lses)


def softmax_bwd_contract(t_rowptr, t_col, x, t, g, out_fwd, lse, dtype=torch.float64):
    """The backward formula of the kernel, one source row at a time, in ``dtype``: per entry
    ``w = exp(t x[c] - lse[r])``, ``d = x[c] - out_fwd[r]``; ``dx[c] = sum w g[r] (1 + t d)``
    and ``dt = sum_c sum w g[r] d^2``. Returns ``(dx, dt)``."""
    x, t, g = x.to(dtype), t.to(dtype), g.to(dtype)
    of, lse = out_fwd.to(dtype), lse.to(dtype)
    C, F = t_rowptr.numel() - 1, x.shape[1]
    rp = t_rowptr.tolist()
    dx = torch.zeros(C, F, dtype=dtype)
    dt = torch.zeros(F, dtype=dtype)
    for c in range(C):
        s, e = rp[c], rp[c + 1]
        if e == s:
            continue
        r = t_col[s:e].long()
        wg = torch.exp(t * x[c] - lse[r]) * g[r]
        d = x[c] - of[r]
        dx[c] = _sum_rows(wg * (1 + t * d))
        dt = dt + _sum_rows(wg * d * d)
    return dx, dt


T5 = torch.tensor([-2.0, -0.5, 0.0, 0.7, 3.0], dtype=torch.float64)  # mixed signs and a zero


@functools.lru_cache(maxsize=None)
def _small_case():
    csr = small_csr()
    x = values("plain", 30, 5, 7).double()
    gy = values("plain", 40, 5, 8).double()
    return csr, x, gy


@pytest.mark.parametrize("tkind", ["float", "scalar0d", "scalar1", "channel"])
def test_op_matches_contract_fp64(tkind):
    csr, x, gy = _small_case()
    t0 = {"float": 1.3, "scalar0d": torch.tensor(1.3, dtype=torch.float64),
          "scalar1": torch.tensor([-0.8], dtype=torch.float64), "channel": T5}[tkind]
    xr = x.clone().requires_grad_()
    tr = torch.as_tensor(t0, dtype=torch.float64).clone().requires_grad_()
    ref, _ = softmax_contract(csr.rowptr, csr.col, xr, tr)
    gxr, gtr = torch.autograd.grad((ref * gy).sum(), (xr, tr))
    xi = x.clone().requires_grad_()
    ti = t0 if tkind == "float" else t0.clone().requires_grad_()
    out = softmax_aggregate(xi, csr, ti)
    assert out.shape == (40, 5) and out.dtype == torch.float64
    torch.testing.assert_close(out.detach(), ref.detach(), atol=1e-10, rtol=1e-10)
    assert torch.count_nonzero(out[3]) == 0  # the empty row
    torch.testing.assert_close(out[4].detach(), x[csr.col[csr.rowptr[4]].long()],
                               atol=1e-12, rtol=1e-12)  # degree 1: its one source
    out.backward(gy)
    torch.testing.assert_close(xi.grad, gxr, atol=1e-10, rtol=1e-10)
    if tkind != "float":
        assert ti.grad.shape == ti.shape
        torch.testing.assert_close(ti.grad, gtr.reshape(ti.shape), atol=1e-10, rtol=1e-10)


def test_backward_formula_is_the_gradient():
    """The explicit backward contract (what the kernel evaluates) equals autograd of the
    forward contract in fp64, and the low-level wrappers return ``lse`` and the partials."""
    csr, x, gy = _small_case()
    xr, tr = x.clone().requires_grad_(), T5.clone().requires_grad_()
    ref, lse = softmax_contract(csr.rowptr, csr.col, xr, tr)
    gx, gt = torch.autograd.grad((ref * gy).sum(), (xr, tr))
    tp = csr.transpose()
    dx, dt = softmax_bwd_contract(tp.rowptr, tp.col, x, T5, gy, ref.detach(), lse.detach())
    torch.testing.assert_close(dx, gx, atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(dt, gt, atol=1e-12, rtol=1e-12)
    out, l2 = K.segment_softmax(csr.rowptr, csr.col, x, T5)
    torch.testing.assert_close(l2, lse.detach(), atol=1e-12, rtol=1e-12)
    assert bool((l2[3] == float("-inf")).all())
    kdx, part = K.segment_softmax_bwd(tp.rowptr, tp.col, x, T5, gy, out, l2)
    torch.testing.assert_close(kdx, gx, atol=1e-10, rtol=1e-10)
    torch.testing.assert_close(part.sum(0), gt, atol=1e-10, rtol=1e-10)
    assert K.segment_softmax_bwd(tp.rowptr, tp.col, x, T5, gy, out, l2, want_dt=False)[1] is None


def test_gradcheck_fp64():
    g = torch.Generator().manual_seed(0)
    csr = CSR.from_coo(torch.randint(0, 6, (20,), generator=g),
                       torch.randint(0, 9, (20,), generator=g), 6, 9)
    x = torch.randn(9, 3, dtype=torch.float64, generator=g).requires_grad_()
    t = torch.tensor([0.6, -1.1, 0.0], dtype=torch.float64, requires_grad=True)
    ts = torch.tensor(0.9, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda a, b: softmax_aggregate(a, csr, b), (x, t))
    assert torch.autograd.gradcheck(lambda a, b: softmax_aggregate(a, csr, b), (x, ts))


def _runner_up_gap(csr, x):
    """The smallest positive distance of any entry from its row's maximum or minimum."""
    rp = csr.rowptr.tolist()
    best = float("inf")
    for r in range(len(rp) - 1):
        if rp[r + 1] == rp[r]:
            continue
        v = x[csr.col[rp[r]:rp[r + 1]].long()]
        for d in (v.max(0).values - v, v - v.min(0).values):
            if bool((d > 0).any()):
                best = min(best, float(d[d > 0].min()))
    return best


def test_limits_mean_max_min_and_shift():
    csr, x, _ = _small_case()
    torch.testing.assert_close(softmax_aggregate(x, csr, 0.0), aggregate(x, csr, reduce="mean"),
                               atol=1e-6, rtol=1e-6)  # the SpMM's row scale 1/deg is fp32
    # |t| = 200 on randn. A runner-up delta below the extreme keeps the weight
    # exp(-200 delta) and moves the result by delta exp(-200 delta), up to 1 / (200 e) =
    # 1.8e-3 at delta = 0.005: the limit is reached to 1e-6 only where no entry lies within
    # (0, 0.1) of its row's extreme (then at most 8 * 0.1 * e^-20 = 2e-9; exact ties cost
    # nothing). The seed is chosen so that the INPUT has that property, asserted here.
    g = torch.Generator().manual_seed(0)
    c12 = CSR.from_coo(torch.randint(0, 12, (40,), generator=g),
                       torch.randint(0, 9, (40,), generator=g), 12, 9)
    xf = torch.randn(9, 3, generator=torch.Generator().manual_seed(21))
    assert _runner_up_gap(c12, xf) >= 0.1 and int(c12.degree().max()) <= 9
    torch.testing.assert_close(softmax_aggregate(xf.double(), c12, 200.0),
                               aggregate(xf, c12, reduce="max").double(), atol=1e-6, rtol=0)
    torch.testing.assert_close(softmax_aggregate(xf.double(), c12, -200.0),
                               aggregate(xf, c12, reduce="min").double(), atol=1e-6, rtol=0)
    # a constant added to x: the weights are unchanged and out moves by exactly that much
    # (k and x are multiples of 2^-10, so that x + k and t (x + k) - max are exact in fp64)
    xq = (x * 1024).round() / 1024
    k = 37.5
    tq = torch.tensor([-2.0, -0.5, 0.0, 0.75, 3.0], dtype=torch.float64)
    o0, l0 = K.segment_softmax(csr.rowptr, csr.col, xq, tq)
    o1, l1 = K.segment_softmax(csr.rowptr, csr.col, xq + k, tq)
    ne = csr.degree() > 0
    torch.testing.assert_close(o1[ne], o0[ne] + k, atol=1e-12, rtol=0)
    torch.testing.assert_close((l1 - l0)[ne], (tq * k).expand(40, 5)[ne], atol=1e-12, rtol=0)
    tp = csr.transpose()
    w0 = torch.exp(tq * xq[tp.row_ids()] - l0[tp.col.long()])
    w1 = torch.exp(tq * (xq + k)[tp.row_ids()] - l1[tp.col.long()])
    torch.testing.assert_close(w1, w0, atol=1e-12, rtol=1e-12)
    assert torch.count_nonzero(o1[~ne]) == 0


def test_reduce_softmax_and_validation():
    csr, x, _ = _small_case()
    assert torch.equal(aggregate(x, csr, reduce="softmax"), softmax_aggregate(x, csr, 1.0))
    with pytest.raises(ValueError):
        aggregate(x, csr, edge_weight=torch.ones(csr.nnz), reduce="softmax")
    with pytest.raises(ValueError):
        aggregate(x, csr, reduce="softmax", heads=2)
    with pytest.raises(ValueError):
        softmax_aggregate(x, csr, torch.ones(4, dtype=torch.float64))
    with pytest.raises(ValueError):
        K.segment_softmax(csr.rowptr, csr.col, x, torch.ones(3, dtype=torch.float64))
    # existing reductions keep their results
    xf = x.float()
    assert torch.equal(aggregate(xf, csr, reduce="sum"), K.spmm(csr.rowptr, csr.col, xf))


def test_empty_patterns_and_strided_input():
    csr, x, _ = _small_case()
    big = torch.zeros(30, 11, dtype=torch.float64)
    big[:, 3:8] = x
    bigr = big.clone().requires_grad_()
    out = softmax_aggregate(bigr[:, 3:8], csr, T5)  # row stride 11, column stride 1
    torch.testing.assert_close(out.detach(), softmax_aggregate(x, csr, T5), atol=0, rtol=0)
    out.sum().backward()
    assert torch.count_nonzero(bigr.grad[:, :3]) == 0 and torch.count_nonzero(bigr.grad[:, 8:]) == 0
    empty = CSR(torch.zeros(8, dtype=torch.long), torch.zeros(0, dtype=torch.int32), 30)
    o, l = K.segment_softmax(empty.rowptr, empty.col, x.float(), 1.0)
    assert torch.count_nonzero(o) == 0 and bool((l == float("-inf")).all())
    none = CSR(torch.zeros(1, dtype=torch.long), torch.zeros(0, dtype=torch.int32), 30)
    assert softmax_aggregate(x, none).shape == (0, 5)
    x0 = torch.zeros(0, 6, requires_grad=True)
    t0 = torch.ones(1, requires_grad=True)
    o = softmax_aggregate(x0, CSR(torch.zeros(4, dtype=torch.long),
                                  torch.zeros(0, dtype=torch.int32), 0), t0)
    o.sum().backward()
    assert o.shape == (3, 6) and x0.grad.shape == (0, 6) and float(t0.grad) == 0.0


# ------------------------------------------------------------------ two sources
SPLIT = 130


def split_csr(idx_dtype=torch.int64):
    """The skewed CSR (300 rows over 257 columns) with rows 1 and 2 forced: row 1 (degree 1)
    reads column 200 only (no entry in the first block), row 2 (degree 2) columns 5 and 6 (no
    entry in the second). Row 150 is empty in both. Returns ``(full, first, second)``, split
    at column 130."""
    c = skewed_csr()
    col = c.col.clone()
    col[int(c.rowptr[1])] = 200
    col[int(c.rowptr[2]):int(c.rowptr[3])] = torch.tensor([5, 6])
    full = CSR(c.rowptr, col.to(idx_dtype), 257)
    a, b = full.split_columns(SPLIT)
    da, db = a.degree(), b.degree()
    assert da[1] == 0 and db[1] == 1 and da[2] == 2 and db[2] == 0 and da[150] + db[150] == 0
    assert bool(((da > 0) & (db > 0)).any())
    return full, a, b


def two_pass(a, b, x, t, row_map=False):
    """Pass 1 over the first block, then pass 2 over the second with ``second=True`` (over
    all rows, or row-compacted with ``row_map``). Returns ``(out, lse, out of pass 1, lse of
    pass 1)``."""
    R, F = a.num_rows, x.shape[1]
    out = torch.empty(R, F, dtype=x.dtype, device=x.device)
    lse = torch.empty(R, F, dtype=x.dtype, device=x.device)
    K.segment_softmax(a.rowptr, a.col, x[:SPLIT], t, out, lse)
    o1, l1 = out.clone(), lse.clone()
    if row_map:
        bc = b.compact_rows()
        K.segment_softmax(bc.rowptr, bc.col, x[SPLIT:], t, out, lse, second=True,
                          row_map=bc.row_map)
    else:
        K.segment_softmax(b.rowptr, b.col, x[SPLIT:], t, out, lse, second=True)
    return out, lse, o1, l1


@pytest.mark.parametrize("row_map", [False, True])
def test_carry_mode_matches_unsplit(row_map):
    full, a, b = split_csr()
    x = values("plain", 257, 6, 21).double()
    t = torch.tensor([1.0, -1.5, 0.0, 2.5, 0.3, -0.2], dtype=torch.float64)
    out, lse, o1, l1 = two_pass(a, b, x, t, row_map)
    ref, rl = softmax_contract(full.rowptr, full.col, x, t)
    torch.testing.assert_close(out, ref, atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(lse, rl, atol=1e-12, rtol=1e-12)
    absent = b.degree() == 0
    assert bool(absent[2]) and torch.equal(out[absent], o1[absent])
    assert torch.equal(lse[absent], l1[absent])
    # row 1: empty after pass 1 (0, -inf), its one entry comes from the second block
    assert torch.count_nonzero(o1[1]) == 0 and bool((l1[1] == float("-inf")).all())
    torch.testing.assert_close(out[1], x[200], atol=1e-12, rtol=1e-12)
    assert torch.count_nonzero(out[150]) == 0 and bool((lse[150] == float("-inf")).all())


# ------------------------------------------------------------------ distributed
SHAPE = SHAPES["ogbn-arxiv"].scaled(0.01)
DF = 16


def _global_inputs(dtype, device="cpu", shape=SHAPE):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(shape.num_nodes, DF, generator=g)
    gy = torch.randn(shape.num_nodes, DF, generator=g)
    t = torch.linspace(-2.0, 2.0, DF)
    t[5] = 0.0
    return x.to(dtype).to(device), gy.to(dtype).to(device), t.to(dtype).to(device)


def _single_rank_reference(dtype, device, scalar, shape=SHAPE):
    p = build_partition(shape, 0, 1, device)
    x, gy, t = _global_inputs(dtype, device, shape)
    t = t[3:4].clone() if scalar else t
    x.requires_grad_()
    t.requires_grad_()
    g1 = DistGraph(p["csr"], p["L"], 0, symmetric=True)
    out = dist_softmax_aggregate(x, g1, t)
    out.backward(gy)
    return out.detach(), x.grad, t.grad


def dist_softmax_body(rank, world, device="cpu", dtype=torch.float64, check=None):
    """W ranks against W = 1 on the same device and dtype: forward, ``dx`` and the
    all-reduced ``dt``, with a per-channel and a scalar temperature. ``check(name, got,
    want)`` compares (default: 1e-9, the fp64 figure)."""
    import torch.distributed as dist

    if check is None:
        def check(name, got, want):
            torch.testing.assert_close(got, want, atol=1e-9, rtol=1e-9, msg=lambda m: name + m)
    p = build_partition(SHAPE, rank, world, device)
    g = DistGraph(p["csr"], p["L"], p["H"], p["send_local_idx"], p["send_splits"],
                  p["recv_splits"])
    lo, hi = p["offsets"][rank], p["offsets"][rank + 1]
    for scalar in (False, True):
        ref_out, ref_gx, ref_gt = _single_rank_reference(dtype, device, scalar)
        x, gy, t = _global_inputs(dtype, device)
        t = (t[3:4].clone() if scalar else t).requires_grad_()
        xl = x[lo:hi].clone().requires_grad_()
        e0 = g.edges_aggregated
        out = dist_softmax_aggregate(xl, g, t)
        out.backward(gy[lo:hi])
        assert g.edges_aggregated - e0 == 2 * g.nnz
        gt = t.grad.clone()
        assert gt.shape == t.shape
        dist.all_reduce(gt)
        check("out", out.detach(), ref_out[lo:hi])
        check("dx", xl.grad, ref_gx[lo:hi])
        check("dt", gt, ref_gt)
    x, _, _ = _global_inputs(dtype, device)
    assert torch.equal(dist_aggregate(x[lo:hi], g, reduce="softmax"),
                       dist_softmax_aggregate(x[lo:hi], g, 1.0))


@pytest.mark.parametrize("world", [2, 3])
def test_dist_softmax_matches_single_rank(ranks, world):
    ranks(dist_softmax_body, world)


def _sends_without_halo_body(rank, world):
    """Rank 0 owns vertices 0-2 and reads only those; rank 1 owns 3-4 and reads vertices 0
    and 2 of rank 0: rank 0 has sends and H == 0, and must still post both exchanges."""
    import torch.distributed as dist

    grow = torch.tensor([0, 0, 1, 2, 3, 3, 3, 4, 4])
    gcol = torch.tensor([1, 2, 0, 0, 0, 4, 2, 2, 3])
    gcsr = CSR.from_coo(grow, gcol, 5, 5)
    x = torch.tensor([[0.5, -1.0], [2.0, 0.25], [-3.0, 4.0], [1.5, -2.5], [0.75, 3.5]]).double()
    gy = torch.arange(1.0, 11.0, dtype=torch.float64).reshape(5, 2)
    t0 = torch.tensor([0.7, -1.2], dtype=torch.float64)
    xg, tg = x.clone().requires_grad_(), t0.clone().requires_grad_()
    ref = softmax_aggregate(xg, gcsr, tg)
    ref.backward(gy)
    if rank == 0:
        csr = CSR.from_coo(torch.tensor([0, 0, 1, 2]), torch.tensor([1, 2, 0, 0]), 3, 3)
        g = DistGraph(csr, 3, 0, torch.tensor([0, 2], dtype=torch.int32), [0, 2], [0, 0])
        assert g.halo is not None and g.H == 0
        sl = slice(0, 3)
    else:
        csr = CSR.from_coo(torch.tensor([0, 0, 0, 1, 1]), torch.tensor([2, 1, 3, 3, 0]), 2, 4)
        g = DistGraph(csr, 2, 2, torch.zeros(0, dtype=torch.int32), [0, 0], [2, 0])
        sl = slice(3, 5)
    xl, tl = x[sl].clone().requires_grad_(), t0.clone().requires_grad_()
    out = dist_softmax_aggregate(xl, g, tl)
    out.backward(gy[sl])
    gt = tl.grad.clone()
    dist.all_reduce(gt)
    torch.testing.assert_close(out.detach(), ref.detach()[sl], atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(xl.grad, xg.grad[sl], atol=1e-10, rtol=1e-10)
    torch.testing.assert_close(gt, tg.grad, atol=1e-10, rtol=1e-10)


def test_rank_with_sends_and_no_halo_rows(ranks):
    ranks(_sends_without_halo_body, 2)


# ------------------------------------------------------------------ the layer
LF, LOUT = 6, 5


def make_layer(seed=0):
    from dgraph_amd.models import CommAwareGENConv

    torch.manual_seed(seed)
    layer = CommAwareGENConv(LF, LOUT, t=0.8, learn_t=True, channelwise_t=True, bias=True)
    with torch.no_grad():
        layer.t.copy_(torch.tensor([0.8, -0.6, 1.7, 0.0, -1.1]))
    return layer.double()


def _dense_layer_reference(layer, x, gy, csr):
    """The module docstring's formula in fp64 with the row-by-row contract as the
    aggregator. Returns the output, ``dx`` and the parameter gradients by name."""
    ref = copy.deepcopy(layer).double()
    ref.zero_grad()
    xr = x.clone().requires_grad_()
    msg = torch.relu(ref.lin_src(xr)) + ref.eps
    agg, _ = softmax_contract(csr.rowptr, csr.col, msg, ref.t)
    out = ref.mlp(agg + ref.lin_dst(xr))
    (out * gy).sum().backward()
    return out.detach(), xr.grad, {n: q.grad for n, q in ref.named_parameters()}


def layer_body(rank, world, device="cpu", dtype=torch.float64, check=None):
    import torch.distributed as dist

    if check is None:
        def check(name, got, want):
            torch.testing.assert_close(got, want, atol=1e-9, rtol=1e-9, msg=lambda m: name + m)
    p1 = build_partition(SHAPE, 0, 1, "cpu")
    g = torch.Generator().manual_seed(12)
    x = torch.randn(SHAPE.num_nodes, LF, generator=g).double()
    gy = torch.randn(SHAPE.num_nodes, LOUT, generator=g).double()
    layer = make_layer()
    ro, rdx, rgrads = _dense_layer_reference(layer, x, gy, p1["csr"])
    p = build_partition(SHAPE, rank, world, device)
    graph = DistGraph(p["csr"], p["L"], p["H"], p["send_local_idx"], p["send_splits"],
                      p["recv_splits"]) if world > 1 else DistGraph(p["csr"], p["L"], 0)
    lo, hi = p["offsets"][rank], p["offsets"][rank + 1]
    layer = layer.to(device=device, dtype=dtype)
    xl = x[lo:hi].to(device=device, dtype=dtype).requires_grad_()
    out = layer(xl, graph)
    (out * gy[lo:hi].to(device=device, dtype=dtype)).sum().backward()
    check("out", out.detach().cpu().double(), ro[lo:hi])
    check("dx", xl.grad.cpu().double(), rdx[lo:hi])
    for name, q in layer.named_parameters():
        grad = q.grad
        if world > 1:
            dist.all_reduce(grad)
        check(name, grad.cpu().double(), rgrads[name])


def test_layer_matches_dense_single_rank():
    layer_body(0, 1)


@pytest.mark.parametrize("world", [2, 3])
def test_layer_matches_dense_ranks(ranks, world):
    ranks(layer_body, world)


def test_layer_options():
    from dgraph_amd.models.genconv import CommAwareGENConv

    p = build_partition(SHAPE, 0, 1, "cpu")
    graph = DistGraph(p["csr"], p["L"], 0)
    x = torch.randn(SHAPE.num_nodes, LF)
    for kw, shape in ((dict(learn_t=True), (1,)),
                      (dict(learn_t=True, channelwise_t=True), (LF,))):
        layer = CommAwareGENConv(LF, LF, t=0.5, **kw)
        assert isinstance(layer.t, torch.nn.Parameter) and layer.t.shape == shape
        assert layer.lin_src is None and layer.lin_dst is None
        out = layer(x, graph)
        assert out.shape == (SHAPE.num_nodes, LF)
        out.square().mean().backward()
        assert layer.t.grad.shape == shape and float(layer.t.grad.abs().max()) > 0
    fixed = CommAwareGENConv(LF, LOUT, t=2.0, norm=False, expansion=3)
    assert fixed.t == 2.0 and not any(n == "t" for n, _ in fixed.named_parameters())
    assert fixed.mlp[0].weight.shape == (3 * LOUT, LOUT) and fixed.mlp[0].bias is None
    assert not any(isinstance(m, torch.nn.LayerNorm) for m in fixed.mlp)
    assert fixed(x, graph).shape == (SHAPE.num_nodes, LOUT)
