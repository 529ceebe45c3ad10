"""The fused PNA statistics kernels (csrc/kernels/spmm_pna.hip, through ``K.segment_pna`` /
``K.segment_pna_bwd``), ``aggregate_multi``, ``DistGraph.aggregate_multi`` and
``CommAwarePNAConv`` on the GPU against the fp64 evaluation of their contract
(tests/test_pna.py: ``pna_contract`` / ``pna_bwd_contract``, one row at a time).

Inputs: the skewed CSR (300 rows over 257 columns, Poisson(7) degrees, row 0 with 5,000
entries, row 150 empty, rows 1 / 2 of degree 1 / 2) with ``x = randn`` ("plain"),
``1000 + 0.1 randn`` ("offset": tells the pivoted variance from ``E[x^2] - E[x]^2``) or one
column constant at 3.7.

``vmax`` / ``vmin`` / ``amax`` / ``amin`` must EQUAL the contract's. ``mean``, ``sdev`` and
gradients: ``|kernel - fp64| <= test_gat_kernels.bound(ref64, ref32)`` with ``ref32`` the
same two-pass contract in fp32 on the CPU; nothing is taken from the kernel's own output.
The backward kernel is given the forward kernel's ``mean`` / ``sdev``. Largest
``error / bound`` seen on an MI355X (a record, not an input to the bound; every figure is
printed before it is asserted):

    forward, plain     mean 0.008   sdev 0.042   sdev of the degree-1 row 0.000
    column blocks      mean 0.008   sdev 0.009
    optional outputs   mean 0.006   sdev 0.009
    offset (F = 24)    mean 0.001 (err 3.1e-5, bound 2.4e-2)   sdev 0.000 (4.3e-8, 3.9e-4)
    constant column    mean 0.002   sdev 0.004   the constant column's sdev 0.000
    backward           dx 0.126 (F = 172, g_std alone)   dx with beta = 1 0.086
    ties               mean 0.005   sdev 0.004
    two sources        mean 0.005   sdev 0.008   dx 0.007   dx of the halo rows 0.007

The fp32 contract sums one entry at a time (test_pna._sum_rows), so the bounds are those of a
plain fp32 evaluation: 4.6e-5 for the plain sdev. A first version of the kernel that kept
ONE pivot per lane group for a whole row missed it at F = 172 (one lane group, the
5,000-entry row: 6.8e-5 against 5.6e-5); the kernel now re-centres the pivot every four
entries.
"""
from __future__ import annotations

import functools
import math

import pytest
import torch

from conftest import rank_device, run_ranks
from dgraph_amd.ops import kernels as K
from dgraph_amd.ops.aggregate import aggregate_multi
from dgraph_amd.ops.csr import CSR
from test_gat_kernels import bound
from test_pna import ALL, EPS, pna_bwd_contract, pna_contract, skewed_csr, values

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.25e9  # what output buffers hold outside the blocks the kernel may write
RATIOS: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(RATIOS):
        print(f"\n[pna] largest error / bound, {k}: {RATIOS[k]:.3f}", end="")


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


@functools.lru_cache(maxsize=None)
def fwd_refs(kind, F):
    """(fp64, fp32) contract of the skewed case (shared by the index widths)."""
    csr = skewed_csr()
    x = values(kind, 257, F, F)
    r64 = pna_contract(csr.rowptr, csr.col, x)
    r32 = pna_contract(csr.rowptr, csr.col, x, dtype=torch.float32)
    return x, r64, r32


def run_fwd(csr, x, which=ALL, eps=EPS):
    """K.segment_pna into fresh buffers; ``which`` out of moments / max / min."""
    R, F = csr.num_rows, x.shape[1]
    f = lambda dt: torch.full((R, F), SENT if dt == torch.float32 else -77, dtype=dt,  # noqa
                              device=x.device)
    o = {}
    if "mean" in which or "std" in which:
        o.update(mean=f(torch.float32), sdev=f(torch.float32))
    if "max" in which:
        o.update(vmax=f(torch.float32), amax=f(torch.int32))
    if "min" in which:
        o.update(vmin=f(torch.float32), amin=f(torch.int32))
    K.segment_pna(csr.rowptr, csr.col, x, eps=eps, **o)
    return o


def check_fwd(tag, o, r64, r32):
    if "vmax" in o:
        assert torch.equal(o["vmax"].cpu().double(), r64["max"])
        assert torch.equal(o["amax"].cpu(), r64["amax"])
    if "vmin" in o:
        assert torch.equal(o["vmin"].cpu().double(), r64["min"])
        assert torch.equal(o["amin"].cpu(), r64["amin"])
    if "mean" in o:
        within(tag, "mean", o["mean"], r64["mean"], r32["mean"])
        within(tag, "sdev", o["sdev"], r64["std"], r32["std"])


@pytest.mark.parametrize("F", [1, 3, 4, 64, 172, 600])
@pytest.mark.parametrize("idx", [torch.int32, torch.int64])
def test_forward(F, idx):
    x, r64, r32 = fwd_refs("plain", F)
    csr = skewed_csr(idx).to(DEV)
    o = run_fwd(csr, x.to(DEV))
    check_fwd(f"fwd[F={F}]", o, r64, r32)
    assert torch.count_nonzero(o["mean"][150]) == 0 and torch.count_nonzero(o["vmax"][150]) == 0
    assert torch.count_nonzero(o["vmin"][150]) == 0
    assert bool((o["amax"][150] == -1).all()) and bool((o["amin"][150] == -1).all())
    assert torch.equal(o["sdev"][150].cpu(), torch.full((F,), EPS).sqrt())  # both fp32 sqrt
    root = torch.full((F,), math.sqrt(EPS), dtype=torch.float64)
    within(f"fwd[F={F}]", "sdev of the degree-1 row", o["sdev"][1], root, r32["std"][1])


@pytest.mark.parametrize("F,pad", [(3, 1), (64, 4)])
def test_outputs_as_column_blocks(F, pad):
    """The four value arrays as the column blocks of one [R, 4F] buffer inside a wider one
    (F = 3: row stride 14, no multiple of 4; F = 64: 16-B aligned blocks), the args as the
    blocks of an int buffer: nothing outside the blocks is written."""
    x, r64, r32 = fwd_refs("plain", F)
    csr = skewed_csr(torch.int32).to(DEV)
    wide = torch.full((300, 4 * F + 2 * pad), SENT, device=DEV)
    iwide = torch.full((300, 2 * F + 2 * pad), -77, dtype=torch.int32, device=DEV)
    buf, ibuf = wide[:, pad:pad + 4 * F], iwide[:, pad:pad + 2 * F]
    o = dict(mean=buf[:, :F], vmax=buf[:, F:2 * F], vmin=buf[:, 2 * F:3 * F],
             sdev=buf[:, 3 * F:], amax=ibuf[:, :F], amin=ibuf[:, F:])
    K.segment_pna(csr.rowptr, csr.col, x.to(DEV), **o)
    check_fwd(f"blocks[F={F}]", o, r64, r32)
    assert bool((wide[:, :pad] == SENT).all()) and bool((wide[:, pad + 4 * F:] == SENT).all())
    assert bool((iwide[:, :pad] == -77).all()) and bool((iwide[:, pad + 2 * F:] == -77).all())
    assert not bool((buf == SENT).any()) and not bool((ibuf == -77).any())


@pytest.mark.parametrize("which", [("mean", "std"), ("max", "min"), ("min",), ("max",)])
def test_optional_outputs(which):
    x, r64, r32 = fwd_refs("plain", 64)
    csr = skewed_csr(torch.int64).to(DEV)
    o = run_fwd(csr, x.to(DEV), which)
    assert set(o) == {k for w in which for k in
                      {"mean": ("mean", "sdev"), "std": ("mean", "sdev"), "max": ("vmax", "amax"),
                       "min": ("vmin", "amin")}[w]}
    check_fwd(f"optional[{'+'.join(which)}]", o, r64, r32)


@pytest.mark.parametrize("kind", ["offset", "constant"])
def test_offset_and_constant_values(kind):
    """Forward only, F = 24. Offset: ``x = 1000 + 0.1 randn`` (E[x^2] - E[x]^2 errs 2.5 here,
    far above the bound). Constant: one column at 3.7, whose sdev is sqrt(eps)."""
    x, r64, r32 = fwd_refs(kind, 24)
    csr = skewed_csr(torch.int32).to(DEV)
    o = run_fwd(csr, x.to(DEV))
    check_fwd(f"{kind}[F=24]", o, r64, r32)
    if kind == "constant":
        within("constant[F=24]", "sdev of the constant column", o["sdev"][:, 12],
               r64["std"][:, 12], r32["std"][:, 12])


@functools.lru_cache(maxsize=None)
def bwd_refs(F, which):
    """(g by name, fp64 gradient, fp32 gradient) of the skewed plain case by the explicit
    backward contract, each with its own dtype's forward."""
    x, r64, r32 = fwd_refs("plain", F)
    csr = skewed_csr()
    g = {a: values("plain", 300, F, 1000 + F + i) for i, a in enumerate(ALL) if a in which}
    t, rel = csr.transpose_rel()
    deg = csr.degree().clamp(min=1)
    d64 = pna_bwd_contract(t.rowptr, t.col, rel, x, 1.0 / deg.double(), r64, g)
    d32 = pna_bwd_contract(t.rowptr, t.col, rel, x, 1.0 / deg.float(), r32, g,
                           dtype=torch.float32)
    return g, d64, d32


@pytest.mark.parametrize("F", [3, 64, 172, 600])
@pytest.mark.parametrize("idx", [torch.int32, torch.int64])
@pytest.mark.parametrize("which", [("std",), ALL], ids=["std", "all"])
def test_backward(F, idx, which):
    x, r64, r32 = fwd_refs("plain", F)
    g, d64, d32 = bwd_refs(F, which)
    csr = skewed_csr(idx)
    dcsr = csr.to(DEV)
    xd = x.to(DEV)
    o = run_fwd(dcsr, xd)
    t, rel = csr.transpose_rel()
    t, rel = t.to(DEV), rel.to(DEV)
    gd = {a: v.to(DEV) for a, v in g.items()}
    kw = dict(g_mean=gd.get("mean"), g_std=gd.get("std"), mean=o["mean"], sdev=o["sdev"],
              g_max=gd.get("max"), amax=o["amax"], g_min=gd.get("min"), amin=o["amin"])
    inv = dcsr.inv_degree()
    out = K.segment_pna_bwd(t.rowptr, t.col, rel, xd, inv, **kw)  # beta = 0
    within(f"bwd[F={F},{'+'.join(which)}]", "dx", out, d64, d32)
    o0 = values("plain", 257, F, 77)
    acc = o0.to(DEV)
    K.segment_pna_bwd(t.rowptr, t.col, rel, xd, inv, acc, beta=1.0, **kw)
    within(f"bwd[F={F},{'+'.join(which)}]", "dx (beta = 1)", acc, d64 + o0.double(),
           d32 + o0)


@pytest.mark.parametrize("shift", [0.0, -3.0, 3.0])
def test_ties_multi_edges_and_signs(shift):
    """64 rows over 5 columns (every row repeats columns), small-integer values (ties
    everywhere; all negative / all positive with a shift): args and the extreme part of the
    gradient exact, moments within the bound."""
    g = torch.Generator().manual_seed(11)
    deg = torch.randint(0, 41, (64,), generator=g)
    rowptr = torch.zeros(65, dtype=torch.long)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, 5, (int(rowptr[-1]),), generator=g, dtype=torch.int32)
    csr = CSR(rowptr, col, 5)
    x = torch.randint(-2, 3, (5, 40), generator=g).float() + shift
    gy = torch.randint(-3, 4, (64, 80), generator=g).float()  # integers: exact sums
    r64 = pna_contract(rowptr, col, x)
    r32 = pna_contract(rowptr, col, x, dtype=torch.float32)
    dcsr = csr.to(DEV)
    check_fwd(f"ties[{shift:+.0f}]", run_fwd(dcsr, x.to(DEV)), r64, r32)
    t, rel = csr.transpose_rel()
    want = pna_bwd_contract(t.rowptr, t.col, rel, x, csr.inv_degree(), r64,
                            {"max": gy[:, :40], "min": gy[:, 40:]})
    xd = x.to(DEV).requires_grad_()
    aggregate_multi(xd, dcsr, ("max", "min")).backward(gy.to(DEV))
    assert torch.equal(xd.grad.cpu().double(), want)


def _rank0_of_two(device):
    from dgraph_amd.data.synthetic import SHAPES, build_partition
    from dgraph_amd.parallel.dist_graph import DistGraph

    shape = SHAPES["ogbn-papers100M"].scaled(5e-5)
    part = build_partition(shape, 0, 2, device, global_frac=0.05, window=256, rehearse=True)
    g = DistGraph(part["csr"], part["L"], part["H"], part["send_local_idx"],
                  part["send_splits"], part["recv_splits"], None)
    return part, g


def test_two_sources_match_the_unsplit_csr():
    """Interior pass + halo pass (second source, all L rows) against the contract over the
    unsplit CSR with [x_local; halo_rows]; then aggregate_multi_T with halo_out."""
    part, g = _rank0_of_two(DEV)
    L, H, F = part["L"], part["H"], 72
    assert 1000 < L < 10000 and H > 0
    full = part["csr"].to("cpu")
    x = values("plain", L + H, F, 2)
    gy = values("plain", L, 4 * F, 3)
    r64 = pna_contract(full.rowptr, full.col, x)
    r32 = pna_contract(full.rowptr, full.col, x, dtype=torch.float32)
    xa = x.to(DEV)
    e0 = g.edges_aggregated
    out, saved = g.aggregate_multi(xa[:L].contiguous(), ALL, halo_rows=xa[L:].contiguous())
    o = out.cpu().double()
    assert torch.equal(o[:, F:2 * F], r64["max"]) and torch.equal(o[:, 2 * F:3 * F], r64["min"])
    assert bool((saved["amax"] >= 0).any()) and bool((saved["amax"] <= -2).any())
    within("two sources", "mean", out[:, :F], r64["mean"], r32["mean"])
    within("two sources", "sdev", out[:, 3 * F:], r64["std"], r32["std"])
    halo_out = torch.empty(H, F, device=DEV)
    gx = g.aggregate_multi_T(gy.to(DEV), xa[:L].contiguous(), saved, ALL, halo_out=halo_out)
    assert g.edges_aggregated - e0 == 2 * g.nnz
    # reference: the backward contract over the unsplit CSR (random values: no ties between
    # distinct sources, so the slot order inside a row does not matter)
    t, rel = full.transpose_rel()
    gb = {a: gy[:, i * F:(i + 1) * F] for i, a in enumerate(ALL)}
    deg = full.degree().clamp(min=1)
    d64 = pna_bwd_contract(t.rowptr, t.col, rel, x, 1.0 / deg.double(), r64, gb)
    d32 = pna_bwd_contract(t.rowptr, t.col, rel, x, 1.0 / deg.float(), r32, gb,
                           dtype=torch.float32)
    within("two sources", "dx", gx, d64[:L], d32[:L])
    within("two sources", "dx of the halo rows", halo_out, d64[L:], d32[L:])


def test_second_source_crafted():
    from dgraph_amd.parallel.dist_graph import DistGraph

    # 3 local rows, 2 halo rows (columns 3, 4). Row 0: interior and halo entries; row 1: halo
    # entries only; row 2: interior only.
    rows = torch.tensor([0, 0, 0, 1, 1, 2, 2])
    cols = torch.tensor([3, 1, 2, 4, 3, 0, 1])
    csr = CSR.from_coo(rows, cols, 3, 5).to(DEV)
    g = DistGraph(csr, 3, 2, torch.tensor([0, 1], dtype=torch.int32, device=DEV), [0, 2],
                  [0, 2], None)
    x = torch.tensor([[1.0, -4.0], [5.0, -1.0], [2.0, -3.0]], device=DEV)
    halo = torch.tensor([[5.0, -1.0], [7.0, -9.0]], device=DEV)
    out, saved = g.aggregate_multi(x, ALL, halo_rows=halo)
    out = out.cpu()
    # row 0 reads {5, 5, 2} / {-1, -1, -3}; row 1 {7, 5} / {-9, -1}; row 2 {1, 5} / {-4, -1}
    mean = torch.tensor([[4.0, -5.0 / 3.0], [6.0, -5.0], [3.0, -2.5]])
    var = torch.tensor([[2.0, 8.0 / 9.0], [1.0, 16.0], [4.0, 2.25]])  # population variance
    torch.testing.assert_close(out[:, 0:2], mean, atol=1e-6, rtol=1e-6)
    torch.testing.assert_close(out[:, 6:8], (var + EPS).sqrt(), atol=1e-6, rtol=1e-6)
    assert torch.equal(out[:, 2:4], torch.tensor([[5.0, -1.0], [7.0, -1.0], [5.0, -1.0]]))
    assert torch.equal(out[:, 4:6], torch.tensor([[2.0, -3.0], [5.0, -9.0], [1.0, -4.0]]))
    # the interior keeps ties (row 0: its slot 0 = column 1); halo winners are -2 - slot
    assert saved["amax"].cpu().tolist() == [[0, 0], [-2, -3], [1, 1]]
    assert saved["amin"].cpu().tolist() == [[1, 1], [-3, -2], [0, 0]]
    gy = torch.zeros(3, 8, device=DEV)
    gy[:, 2:4] = torch.tensor([[1.0, 2.0], [4.0, 8.0], [16.0, 32.0]], device=DEV)
    halo_out = torch.empty(2, 2, device=DEV)
    gx = g.aggregate_multi_T(gy, x, saved, ALL, halo_out=halo_out)
    assert torch.equal(gx.cpu(), torch.tensor([[0.0, 0.0], [17.0, 34.0], [0.0, 0.0]]))
    assert torch.equal(halo_out.cpu(), torch.tensor([[0.0, 8.0], [4.0, 0.0]]))


def test_bitwise_deterministic():
    csr = skewed_csr(torch.int32, seed=9).to(DEV)
    x = values("plain", 257, 172, 9).to(DEV)
    gy = values("plain", 300, 4 * 172, 10).to(DEV)
    res = []
    for _ in range(2):
        xi = x.clone().requires_grad_()
        out = aggregate_multi(xi, csr)
        out.backward(gy)
        res.append((out.detach(), xi.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_contract_checks_raise():
    csr = skewed_csr(torch.int32).to(DEV)
    x = values("plain", 257, 8, 1).to(DEV)
    new = lambda F=8, dt=torch.float32: torch.empty(300, F, dtype=dt, device=DEV)  # noqa: E731
    call = lambda xx, **o: K.segment_pna(csr.rowptr, csr.col, xx, **o)  # noqa: E731
    err = (RuntimeError, ValueError)
    with pytest.raises(err):  # wrong dtype
        call(x.double(), mean=new(dt=torch.float64), sdev=new(dt=torch.float64))
    with pytest.raises(err):
        call(x, mean=new(), sdev=new(dt=torch.float16))
    with pytest.raises(err):  # a column stride
        call(x.t().contiguous().t(), mean=new(), sdev=new())
    with pytest.raises(err):
        call(x, mean=new(), sdev=torch.empty(8, 300, device=DEV).t())
    with pytest.raises(err):  # a misaligned row stride / base (F a multiple of 4)
        call(torch.empty(257, 10, device=DEV)[:, :8], mean=new(), sdev=new())
    with pytest.raises(err):
        call(x, mean=new(), sdev=torch.empty(300, 10, device=DEV)[:, 1:9])
    with pytest.raises(err):  # mismatched F
        call(x, mean=new(), sdev=new(12))
    with pytest.raises(err):  # amax without vmax
        call(x, amax=new(dt=torch.int32))
    with pytest.raises(err):  # int64 args
        call(x, vmax=new(), amax=new(dt=torch.int64))
    with pytest.raises(err):  # a second pass over moments without the first row pointer
        call(x, mean=new(), sdev=new(), second=True)
    with pytest.raises(err):  # outputs with fewer rows than the CSR
        call(x, mean=new()[:100], sdev=new()[:100])
    t, rel = skewed_csr(torch.int32).transpose_rel()
    t, rel = t.to(DEV), rel.to(DEV)
    with pytest.raises(err):  # g_std without mean / sdev
        K.segment_pna_bwd(t.rowptr, t.col, rel, x, csr.inv_degree(), g_std=new())
    with pytest.raises(err):  # x narrower than the gradient
        K.segment_pna_bwd(t.rowptr, t.col, rel, x[:, :4].contiguous(), csr.inv_degree(),
                          torch.empty(257, 8, device=DEV), g_mean=new())


def test_layer_matches_cpu():
    """CommAwarePNAConv on the GPU against the same layer on the CPU, at the tolerances of
    tests/test_segment_max_gpu.py::test_graphsage_max_matches_cpu."""
    from dgraph_amd.data.synthetic import SHAPES, build_partition, node_data
    from dgraph_amd.models import CommAwarePNAConv
    from dgraph_amd.parallel.dist_graph import DistGraph

    shape = SHAPES["ogbn-arxiv"].scaled(0.01)
    p = build_partition(shape, 0, 1, "cpu")
    x, _, _ = node_data(shape, 0, p["offsets"], "cpu", dtype=torch.float32)
    torch.manual_seed(0)
    m = CommAwarePNAConv(shape.num_features, 32)
    res = {}
    for dev in ("cpu", DEV):
        md = m.to(dev)
        md.zero_grad()
        g = DistGraph(p["csr"].to(dev), p["L"], 0, symmetric=True)
        xi = x.clone().to(dev).requires_grad_()
        out = md(xi, g)
        out.square().mean().backward()
        res[dev] = (out.detach().cpu(), [xi.grad.cpu()] +
                    [q.grad.detach().cpu().clone() for q in md.parameters()])
    torch.testing.assert_close(res[DEV][0], res["cpu"][0], atol=1e-5, rtol=1e-4)
    for a, b in zip(res[DEV][1], res["cpu"][1]):
        torch.testing.assert_close(a, b, atol=1e-6, rtol=1e-4)


def _fp32_check(name, got, want):
    """Two fp32 evaluations that differ in summation order (the partition's): each is
    within the fp32 SpMM figure 2e-5 max(1, max|value|) of the exact result
    (``test_gat_kernels.bound``'s floor), so they differ by at most twice that."""
    scale = max(1.0, float(want.abs().max()))
    err = float((got - want).abs().max())
    print(f"[pna W=2] {name}: diff {err:.3e} allowed {4e-5 * scale:.3e}")
    assert err <= 4e-5 * scale, (name, err)


def _w2_body(rank, world):
    import test_pna as D

    from dgraph_amd.comm.rccl_exec import RCCLExecutor

    D.dist_multi_body(rank, world, rank_device(), torch.float32, _fp32_check)
    torch.cuda.synchronize()
    RCCLExecutor.close_all()


def test_dist_multi_two_ranks_rccl():
    """dist_aggregate_multi forward and backward at W = 2 over real RCCL (both ranks on
    GPU 0) against the W = 1 result on the GPU."""
    run_ranks(_w2_body, 2, backend="rccl-one-gpu")
