"""The gated aggregation kernels with bf16 storage (csrc/kernels/spmm_gated_bf16.hip) through
``K.segment_gated`` / ``K.segment_gated_bwd_src`` on bf16 rows, ``gated_aggregate``,
``DistGraph.aggregate_gated`` at W = 2 and a bf16 ``CommAwareResGatedGraphConv``. Inputs,
reference and bounds: tests/test_gated_aggr_bf16.py; nothing comes from the kernels' own output
and every figure is printed before it is asserted. An array rounded to bf16 once may be off by
``b + 2^-8 (|ref64| + b)``, an fp32 output by ``b``; ``dk = rne(g * rne(ds))`` is rounded twice
and may be off by ``(1 + 2^-8)^2 - 1`` of its value (``TWICE``). Largest error / bound seen on
an MI355X (a record, not an input to the bounds; one rounding errs by up to 2^-8 of the value),
as out / ds / dq / dv: kernels 0.951 / 0.942 / 0.975 / 0.975 (fp32 outputs 0.129 / 0.145 / 0.026 /
0.027; k = +-100: 0.766 / 0 / 0 / 0.971); two sources 0.058 / 0.077 in fp32, 0.841 / 0.862 cast;
op out 0.863, dk 0.655, dq 0.958, dv 0.973; W = 2 out 0.969, dk 0.816, d[q | v] 0.714; layer out
0.960 (bf16 layer and autocast alike).
"""
import pytest
import torch

from conftest import rank_device, run_ranks
from dgraph_amd.ops import kernels as K
from dgraph_amd.ops.aggregate import gated_aggregate
from test_gat_bf16 import EPS
from test_gated_aggr import dense_gated, gated_contract, two_pass_gated
from test_gated_aggr_bf16 import COLS, ROWS, bounds, inputs, reference, rounded
from test_pna import skewed_csr
from test_softmax_aggr import SPLIT, split_csr

pytestmark = pytest.mark.gpu
DEV, BF = "cuda", torch.bfloat16
SENT = -7.25e9  # what output buffers hold where the kernels may not write
TWICE = 2 * EPS + EPS * EPS


def within(tag, got, r64, r32, eps=None, extra=0.0):
    # |got - fp64| <= bound + extra elementwise; eps: 2^-8 for a bf16 array, else 0
    eps = (EPS if got.dtype == BF else 0.0) if eps is None else eps
    got, r64 = got.detach().double().cpu(), r64.double()
    assert got.shape == r64.shape and bool(torch.isfinite(got).all()), tag
    b, bd = bounds(r64, r32, eps)
    ratio = float(((got - r64).abs() / (bd + extra)).max())
    print(f"{tag}: b {b:.3e} largest err / bound {ratio:.3f}")
    assert ratio <= 1.0, (tag, ratio)


def run_kernels(F, idx, odt=BF, shift=0.0):
    """k, q, v: column views of ONE [ROWS, 3F] bf16 buffer; out | ds, dq | dv: halves of two."""
    k, q, v, g = inputs(F, shift)
    kqv = torch.full((ROWS, 3 * F), float("nan"), dtype=BF, device=DEV)
    kqv[:, :F], kqv[:COLS, F:2 * F], kqv[:COLS, 2 * F:] = k.to(DEV), q.to(DEV), v.to(DEV)
    kd, qd, vd = kqv[:, :F], kqv[:COLS, F:2 * F], kqv[:COLS, 2 * F:]
    csr = skewed_csr(idx)
    cd, tc = csr.to(DEV), csr.transpose().to(DEV)
    o, o2 = (torch.full((ROWS, 2 * F), SENT, dtype=odt, device=DEV) for _ in range(2))
    d = torch.full((COLS + 3, 2 * F), SENT, dtype=odt, device=DEV)
    K.segment_gated(cd.rowptr, cd.col, kd, qd, vd, o[:, :F], o[:, F:])
    K.segment_gated(cd.rowptr, cd.col, kd, qd, vd, o2[:, :F])
    K.segment_gated_bwd_src(tc.rowptr, tc.col, kd, qd, vd, g.to(DEV, BF), d[:, :F], d[:, F:])
    assert bool((o2[:, F:] == SENT).all()) and bool((d[COLS:] == SENT).all())
    assert torch.equal(o[:, :F], o2[:, :F])
    return dict(out=o[:, :F], ds=o[:, F:], dq=d[:COLS, :F], dv=d[:COLS, F:])


@pytest.mark.parametrize("F,shift", [(8, 0.0), (64, 0.0), (72, 0.0), (256, 0.0), (520, 0.0),
                                     (64, 100.0), (64, -100.0)])
def test_kernels_against_fp64(F, shift):
    """One lane, a full LPR 8 group, LPR 16 with idle lanes, LPR 32, two passes of LPR 64 with a
    tail; index widths and a repeat: equal bits. k +- 100: the derivative (at -100: the gate) 0."""
    r64, r32 = (reference(F, shift, t) for t in (torch.float64, torch.float32))
    res = [run_kernels(F, idx, odt, shift) for idx, odt in (
        (torch.int32, BF), (torch.int64, BF), (torch.int32, BF), (torch.int64, torch.float32))]
    for got in (res[0], res[3]):
        for n, t in got.items():
            within(f"F={F} {shift:+.0f} {t.dtype} {n}", t, r64[n], r32[n])
        assert not bool(got["out"][150].any()) and not bool(got["ds"][150].any())  # empty row
    assert all(torch.equal(res[0][n], other[n]) for other in res[1:3] for n in res[0])
    small = ("ds", "dq") * bool(shift) + ("out", "dv") * (shift < 0)
    assert all(float(res[0][n].abs().max()) < 1e-30 for n in small)


def test_two_sources_into_fp32_sums():
    """Columns < SPLIT, then the rest with accumulate, into fp32 sums: the unsplit contract,
    also after the one cast; a row the second block misses keeps its bits; bf16 is refused."""
    F = 72
    full, a, b = (c.to(DEV) for c in split_csr(torch.int32))
    k, q, v = rounded(ROWS, F, 30), rounded(COLS, F, 31), rounded(COLS, F, 32)
    r64, r32 = (gated_contract(full.rowptr.cpu(), full.col.cpu(), k, q, v, dtype=t)
                for t in (torch.float64, torch.float32))
    kd, qd, vd = (t.to(DEV, BF) for t in (k, q, v))
    with pytest.raises(ValueError, match="accumulate"):
        two_pass_gated(a, b, kd, qd, vd)
    out, ds = (torch.full((ROWS, F), SENT, device=DEV) for _ in range(2))
    K.segment_gated(a.rowptr, a.col, kd, qd[:SPLIT], vd[:SPLIT], out, ds)
    o1, d1 = out.clone(), ds.clone()
    K.segment_gated(b.rowptr, b.col, kd, qd[SPLIT:], vd[SPLIT:], out, ds, accumulate=True)
    for n, t, i in (("out", out, 0), ("ds", ds, 1)):
        within(f"two sources {n} fp32", t, r64[i], r32[i])
        within(f"two sources {n} cast once", t.to(BF), r64[i], r32[i])
    absent = b.degree() == 0
    assert bool(absent[2]) and bool(absent[150])
    assert torch.equal(out[absent], o1[absent]) and torch.equal(ds[absent], d1[absent])
    assert not bool(o1[1].any()) and bool(out[1].any())  # empty in pass 1, then filled


def test_op_against_fp64_autograd():
    k, q, v, g = inputs(64)
    csr, refs = skewed_csr(torch.int32), []
    for dt in (torch.float64, torch.float32):
        ins = [t.to(dt).clone().requires_grad_() for t in (k, q, v)]
        o, _ = gated_contract(csr.rowptr, csr.col, *ins, dtype=dt)
        refs.append((o.detach(),) + torch.autograd.grad((o * g.to(dt)).sum(), ins))
    ins = [t.to(DEV, BF).requires_grad_() for t in (k, q, v)]
    out = gated_aggregate(*ins, csr.to(DEV))
    out.backward(g.to(DEV, BF))
    for n, t, a, b in zip(("out", "dk", "dq", "dv"), [out] + [t.grad for t in ins], *refs):
        assert t.dtype == BF
        within(f"op {n}", t, a, b, TWICE if n == "dk" else EPS)


def test_refusals():
    csr = skewed_csr(torch.int32).to(DEV)
    new = lambda n, F=8, dt=BF, w=0, c0=0: torch.zeros(  # noqa: E731
        n, w or F, dtype=dt, device=DEV)[:, c0:c0 + F]
    k, q, v, o = new(ROWS), new(COLS), new(COLS), new(ROWS)
    cases = {"multiple of 8": (new(ROWS, 12), new(COLS, 12), new(COLS, 12)),
             "k must have .* stride divisible by 8": (new(ROWS, w=12), q, v),  # stride 12
             "q must have .* 16-B alignment": (k, new(COLS, w=16, c0=4), v),   # base 8 B off
             "float32 or bfloat16": (k.half(), q.half(), v.half()),
             "accumulate": (k, q, v, o, None, True),                           # into bf16
             "q must be torch.bfloat16": (k, q.float(), v),
             "ds must be torch.bfloat16": (k, q, v, o, new(ROWS, dt=torch.float32))}
    for msg, args in cases.items():
        with pytest.raises((RuntimeError, ValueError), match=msg):
            K.segment_gated(csr.rowptr, csr.col, *args[:5], accumulate=len(args) > 5)


def _w2_body(rank, world):
    import test_gated_aggr as D
    import test_gated_aggr_gpu as G
    from dgraph_amd.comm.rccl_exec import RCCLExecutor

    shape, dev = G._tiny_shape(), rank_device()

    def run(dt, graph, sl, d, absg=False):
        k, qv, gy = (t.to(d, dt) for t in D._global_inputs(BF, "cpu", shape))
        kl, ql = k[sl].clone().requires_grad_(), qv[sl].clone().requires_grad_()
        out = D.dist_gated_aggregate(kl, ql, graph)
        out.backward(gy[sl].abs() if absg else gy[sl])
        return out.detach(), kl.grad, ql.grad

    r64, r32 = G._cpu_single_rank(run, shape, dev)
    mag = G._cpu_single_rank(lambda *a: run(*a, absg=True), shape, dev)[0][2].abs()
    graph, sl = G._rank_graph(shape, rank, world, dev)
    assert graph.halo is not None
    got = run(BF, graph, sl, dev)
    for n, t, a, b in zip(("out", "dk", "dqv"), got, r64, r32):
        assert t.dtype == BF
        within(f"W=2 {n}", t, a[sl], b[sl], TWICE if n == "dk" else EPS,
               EPS * mag[sl] if n == "dqv" else 0.0)
    k, qv, _ = (t.to(dev) for t in D._global_inputs(BF, "cpu", shape))
    o1, saved = graph.aggregate_gated(k[sl], qv[sl])
    o2, s2 = graph.aggregate_gated(k[sl], qv[sl], halo_rows=saved["halo"])  # no exchange
    assert o1.dtype == BF and saved["ds"].dtype == BF and torch.equal(o1, got[0])
    assert torch.equal(o2, o1) and torch.equal(s2["ds"], saved["ds"])
    torch.cuda.synchronize()
    RCCLExecutor.close_all()


def test_dist_two_ranks_rccl():
    """``dist_gated_aggregate`` and ``aggregate_gated(halo_rows=)`` on bf16 rows at W = 2 against
    the CPU fp64 result. ``d[q | v]`` adds the peer's rows, each rounded by its sender, before
    its own rounding: 2^-8 of the sum of the terms' magnitudes (the pass over ``|g|``) more."""
    run_ranks(_w2_body, 2, backend="rccl-one-gpu")


@pytest.mark.parametrize("autocast", [False, True], ids=["bf16_layer", "autocast"])
def test_layer_bf16_against_dense_fp64(autocast):
    """Without skip term and bias the output is the aggregation of ``[k | q | v]``, the bf16
    result of the one projection GEMM, which the test forms with the same torch call: dense fp64
    on those rows, the single-rounding bound. The default layer returns bf16 too."""
    import test_gated_aggr_gpu as G
    from dgraph_amd.data.synthetic import build_partition
    from dgraph_amd.models import CommAwareResGatedGraphConv as Conv
    from dgraph_amd.parallel.dist_graph import DistGraph

    p = build_partition(G._tiny_shape(), 0, 1, DEV)
    graph, csr = DistGraph(p["csr"], p["L"], 0), p["csr"].to("cpu")
    torch.manual_seed(0)
    layer, full = Conv(6, 16, root_weight=False, bias=False).to(DEV), Conv(6, 16).to(DEV)
    x = torch.randn(p["L"], 6, device=DEV)
    if not autocast:
        layer, full, x = layer.bfloat16(), full.bfloat16(), x.bfloat16()
    x.requires_grad_()
    lins = (layer.lin_key, layer.lin_query, layer.lin_value)
    with torch.autocast("cuda", BF, enabled=autocast):
        out = layer(x, graph)
        h = torch.nn.functional.linear(x, torch.cat([m.weight for m in lins]),
                                       torch.cat([m.bias for m in lins])).detach().cpu()
        assert full(x, graph).dtype == BF
    assert out.dtype == BF and h.dtype == BF
    r64, r32 = (dense_gated(csr, h[:, :16].to(t), h[:, 16:32].to(t), h[:, 32:].to(t))
                for t in (torch.float64, torch.float32))
    within(f"layer autocast={autocast}", out, r64, r32)
    out.backward(torch.ones_like(out))
    assert all(bool(torch.isfinite(w.grad).all()) for w in list(layer.parameters()) + [x])
