"""The DropEdge kernels (csrc/kernels/spmm_drop.hip) called directly through ``_native.ops()``
on the pattern of ``test_gat_kernels.pattern()`` (37 rows over 60 sources; degrees 0, 1, every
lane-group boundary +-1, 130 and a 301-entry hub; 694 of the 1293 entries repeat an earlier
pair), then the op, ``SAGEConv(drop_edge=)`` and a captured step on the GPU.

``out`` is compared with the fp64 contract (``test_drop_edge.drop_contract``, a dense masked
matrix product) under ``test_gat_kernels.bound(ref64, ref32)``: the project's 2e-5 floor for the
fp32 SpMM, or 8 times the error of the same formula evaluated in fp32 on the CPU. Nothing is
taken from the kernels' own output. ``kept_degree`` must equal the CPU count exactly. Every
comparison prints error / bound.

Largest error / bound seen on an MI355X (the module prints it per width at its end): the
kernels 0.070 (F = 256; 0.006 at F = 1, 0.030 at F = 64 and 128, 0.055 at F = 520), the op
0.010 (``dx``), the layer 0.052 (``dw_self``; 0.007 for its output).
"""
from __future__ import annotations

import functools
import itertools

import pytest
import torch

from test_drop_edge import BIG, SEED, drop_contract, keep_of, mean_scale
from test_gat_kernels import N, R, bound, pattern, transpose

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.25e9  # what output buffers hold outside the slices the kernels may write
RATIOS: dict = {}
# the issue's widths, then two that reach what they leave out: 301 (element path, two passes
# of four 64-column chunks) and 520 (16-byte path with three of four chunks of accumulators)
WIDTHS = [1, 3, 4, 60, 64, 100, 128, 256, 301, 520]
PS = [0.0, 0.5, 0.9]
IDS = ["base 0", "base 2^32+", "arrays"]
# (row_scale / col_scale, beta, row_map, wide buffers)
DRESSINGS = [(False, 0.0, False, False), (True, 1.0, True, True), (True, 0.0, False, True),
             (False, 1.0, True, False)]


@pytest.fixture(scope="module", autouse=True)
def _native_and_record():
    from dgraph_amd import _native

    assert _native.load(), "native library missing"
    yield
    for k in sorted(RATIOS, key=str):
        print(f"\n[drop-edge] largest error / bound, {k}: {RATIOS[k]:.3f}", end="")
    print()


def _ops():
    from dgraph_amd import _native

    return _native.ops()


def _seed(value=SEED):
    return torch.tensor([value], dtype=torch.int64, device=DEV)


def _compare(tag, key, got, ref64, ref32):
    got = got.detach().double().cpu()
    assert got.shape == ref64.shape, (tag, got.shape, ref64.shape)
    assert torch.isfinite(got).all(), tag
    bd = bound(ref64, ref32)
    err = float((got - ref64).abs().max()) if got.numel() else 0.0
    RATIOS[key] = max(RATIOS.get(key, 0.0), err / bd)
    print(f"{tag}: err {err:.3e} bound {bd:.3e} ratio {err / bd:.3f}")
    assert err <= bd, (tag, err, bd)


@functools.lru_cache(maxsize=None)
def _patterns(transposed: bool, compact: bool):
    """(rowptr, col, row_map or None, output rows, source rows) on the CPU: the pattern or its
    transpose, optionally over the non-empty rows only."""
    rowptr, col, _ = pattern()
    n_out, n_src = R, N
    if transposed:
        rowptr, col = transpose(rowptr, col, N)
        n_out, n_src = N, R
    row_map = None
    if compact:
        row_map = torch.nonzero(rowptr[1:] > rowptr[:-1]).reshape(-1)
        assert 0 < row_map.numel() < n_out
        rowptr = torch.cat([rowptr[row_map], rowptr[-1:]])
    return rowptr, col, row_map, n_out, n_src


@functools.lru_cache(maxsize=None)
def _values(F: int):
    gen = torch.Generator().manual_seed(100 + F)
    rn = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    return dict(x=rn(N, F), out0=rn(N, F), rs=torch.rand(N, generator=gen) + 0.5,
                cs=torch.rand(N, generator=gen) + 0.5,
                row_ids=torch.randperm(N, generator=gen) + BIG,
                col_ids=torch.randperm(N, generator=gen) * 3 + 1)


def _id_args(mode: str, n_out: int, n_src: int, F: int):
    v = _values(F)
    if mode == "base 0":
        return {}
    if mode == "base 2^32+":
        return dict(row_base=BIG, col_base=BIG + 17)
    return dict(row_ids=v["row_ids"][:n_out], col_ids=v["col_ids"][:n_src])


def _slice(rows, cols, fill, wide, misaligned=False):
    """A [rows, cols] view: the whole of a fresh buffer, or (``wide``) the upper column half
    of a [rows, 2 cols] buffer (one column: column 2 of [rows, 4]), or (``misaligned``) the
    columns 1 .. cols + 1 of a [rows, cols + 3] buffer, off every 16-byte boundary."""
    if misaligned:
        buf = torch.full((rows, cols + 3), fill, device=DEV)
        return buf[:, 1:cols + 1], buf, slice(1, cols + 1)
    if not wide:
        return torch.full((rows, cols), fill, device=DEV), None, None
    if cols == 1:
        buf, sl = torch.full((rows, 4), fill, device=DEV), slice(2, 3)
    else:
        buf, sl = torch.full((rows, 2 * cols), fill, device=DEV), slice(cols, 2 * cols)
    return buf[:, sl], buf, sl


def _run_config(F, transposed, undirected, p, idmode, scales, beta, compact, wide,
                misaligned=False):
    """One configuration at both index widths, twice each: against the contract, bitwise
    equal among the four runs, nothing written outside the output slice; kept_degree (plain
    and accumulating) against the CPU count."""
    ops = _ops()
    rowptr, col, row_map, n_out, n_src = _patterns(transposed, compact)
    v = _values(F)
    ids = _id_args(idmode, n_out, n_src, F)
    x, out0 = v["x"][:n_src], v["out0"][:n_out]
    rs, cs = (v["rs"][:n_out], v["cs"][:n_src]) if scales else (None, None)
    refs = [drop_contract(rowptr, col, x, SEED, p, undirected=undirected, transposed=transposed,
                          col_scale=cs, row_scale=rs, beta=beta, out=out0, row_map=row_map,
                          dtype=dt, **ids) for dt in (torch.float64, torch.float32)]
    (ref64, kept64), (ref32, _) = refs
    out_rows = torch.arange(n_out) if row_map is None else row_map
    tag = (f"F={F} {'T' if transposed else 'N'} {'und' if undirected else 'dir'} p={p} "
           f"{idmode} scales={scales} beta={beta} row_map={compact} wide={wide}"
           f"{' misaligned' if misaligned else ''}")
    dv = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    xin, _, _ = _slice(n_src, F, float("nan"), wide, misaligned)
    xin.copy_(x)
    seed = _seed()
    args = (seed, p, undirected, transposed)
    tail = (dv(row_map), dv(ids.get("row_ids")), dv(ids.get("col_ids")))
    bases = (ids.get("row_base", 0), ids.get("col_base", 0))
    runs = []
    for idx in (torch.int32, torch.int64, torch.int32, torch.int64):
        rp, cl = rowptr.to(DEV), col.to(idx).to(DEV)
        out, buf, sl = _slice(n_out, F, SENT, wide, misaligned)
        out.copy_(out0)
        if beta == 0.0:  # the rows the pass writes hold NaN on entry
            out[out_rows.to(DEV)] = float("nan")
        ops.spmm_drop_f32(rp, cl, xin, out, *args, dv(cs), dv(rs), beta, *tail, *bases)
        torch.cuda.synchronize()
        if buf is not None:
            outside = torch.ones(buf.shape[1], dtype=torch.bool, device=DEV)
            outside[sl] = False
            rest = buf[:, outside]
            assert torch.equal(rest, torch.full_like(rest, SENT)), tag
        runs.append(out.clone())
        kept = torch.full((n_out,), -3, dtype=torch.int32, device=DEV)
        ops.kept_degree(rp, cl, kept, *args, False, *tail, n_src, *bases)
        want = torch.full((n_out,), -3, dtype=torch.int64)
        want[out_rows] = kept64[out_rows]
        assert torch.equal(kept.cpu().long(), want), tag
        ops.kept_degree(rp, cl, kept, *args, True, *tail, n_src, *bases)
        want[out_rows] += kept64[out_rows]
        assert torch.equal(kept.cpu().long(), want), tag
    _compare(tag, F, runs[0], ref64, ref32)
    for other in runs[1:]:  # two runs, and int32 == int64 columns, bit for bit
        assert torch.equal(other.view(torch.int32), runs[0].view(torch.int32)), tag


def test_inputs_are_not_vacuous():
    """Seed 83, base 0, p = 0.5: a non-empty row that loses every entry, one that keeps every
    entry, a partially kept hub; p = 0.9: sources all of whose entries are dropped."""
    rowptr, col, rows = pattern()
    deg = rowptr[1:] - rowptr[:-1]
    for und, lost, full, hub, dead in ((False, 1, 1, 127, 21), (True, 2, 1, 167, 19)):
        _, _, keep = keep_of(rowptr, col, SEED, 0.5, und)
        kept = torch.bincount(rows[keep], minlength=R)
        assert int(((kept == 0) & (deg > 0)).sum()) == lost >= 1
        assert int(((kept == deg) & (deg > 0)).sum()) == full >= 1
        assert int(kept[deg == 301]) == hub and 0 < hub < 301
        _, _, keep9 = keep_of(rowptr, col, SEED, 0.9, und)
        gone = (torch.bincount(col[keep9], minlength=N) == 0) & (torch.bincount(col, minlength=N) > 0)
        assert int(gone.sum()) == dead >= 1


@pytest.mark.parametrize("F", WIDTHS)
def test_spmm_drop_and_kept_degree_vs_fp64(F):
    for (t, und, p, idmode), (scales, beta, compact, wide) in itertools.product(
            itertools.product((False, True), (False, True), PS, IDS), DRESSINGS):
        _run_config(F, t, und, p, idmode, scales, beta, compact, wide)


@pytest.mark.parametrize("F", [4, 64, 256])
def test_misaligned_rows_take_the_element_path(F):
    """A width that is a multiple of 4 in rows off the 16-byte grid: the element path, at
    256 columns with four chunks of accumulators."""
    for t, und in itertools.product((False, True), (False, True)):
        _run_config(F, t, und, 0.5, "arrays", True, 1.0, True, False, misaligned=True)


@pytest.mark.parametrize("undirected", [False, True], ids=["directed", "undirected"])
@pytest.mark.parametrize("F", [3, 64, 256])
def test_dropped_rows_are_never_read(F, undirected):
    """p = 0.9: every source all of whose entries are dropped holds NaN; the output equals the
    clean run bitwise (a load of such a row, even with weight zero, would show)."""
    ops = _ops()
    rowptr, col, _ = pattern()
    _, _, keep = keep_of(rowptr, col, SEED, 0.9, undirected)
    gone = (torch.bincount(col[keep], minlength=N) == 0) & (torch.bincount(col, minlength=N) > 0)
    assert int(gone.sum()) == (19 if undirected else 21)
    x = _values(F)["x"].to(DEV)
    dirty = x.clone()
    dirty[gone.to(DEV)] = float("nan")
    for idx in (torch.int32, torch.int64):
        outs = []
        for src in (x, dirty):
            out = torch.full((R, F), float("nan"), device=DEV)
            ops.spmm_drop_f32(rowptr.to(DEV), col.to(idx).to(DEV), src, out, _seed(), 0.9,
                              undirected, False, None, None, 0.0, None, None, None, 0, 0)
            outs.append(out)
        torch.cuda.synchronize()
        assert torch.isfinite(outs[0]).all()
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


def test_empty_patterns_return_without_a_launch():
    ops = _ops()
    x = torch.randn(4, 8, device=DEV)
    rp = torch.zeros(6, dtype=torch.long, device=DEV)
    col = torch.zeros(0, dtype=torch.int32, device=DEV)
    out = torch.full((5, 8), 2.0, device=DEV)
    ops.spmm_drop_f32(rp, col, x, out, _seed(), 0.5, False, False, None, None, 0.5, None, None,
                      None, 0, 0)
    assert torch.equal(out, torch.full_like(out, 1.0))
    kept = torch.full((5,), 9, dtype=torch.int32, device=DEV)
    ops.kept_degree(rp, col, kept, _seed(), 0.5, False, False, True, None, None, None, 4, 0, 0)
    assert (kept == 9).all()
    ops.kept_degree(rp, col, kept, _seed(), 0.5, False, False, False, None, None, None, 4, 0, 0)
    assert (kept == 0).all()
    ops.spmm_drop_f32(rp[:1], col, x, out[:0], _seed(), 0.5, False, False, None, None, 0.0,
                      None, None, None, 0, 0)
    with pytest.raises(RuntimeError):
        ops.spmm_drop_f32(rp, col, x.bfloat16(), out, _seed(), 0.5, False, False, None, None,
                          0.0, None, None, None, 0, 0)
    with pytest.raises(RuntimeError):
        ops.spmm_drop_f32(rp, col, x, out, _seed(), 1.0, False, False, None, None, 0.0, None,
                          None, None, 0, 0)
    with pytest.raises(RuntimeError):
        ops.spmm_drop_f32(rp, col, x, out, _seed().cpu(), 0.5, False, False, None, None, 0.0,
                          None, None, None, 0, 0)


# ------------------------------------------------------------------ the op and the layer
@pytest.mark.parametrize("undirected", [False, True], ids=["directed", "undirected"])
@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_aggregate_drop_gpu_vs_cpu(reduce, undirected):
    """``aggregate(..., drop=)`` forward and backward on the GPU against its CPU evaluation in
    fp64 (and fp32, for the bound) with the same seed."""
    from dgraph_amd.ops.aggregate import EdgeDrop, aggregate
    from dgraph_amd.ops.csr import CSR

    F = 64
    rowptr, col, _ = pattern()
    v = _values(F)
    ids = (v["row_ids"][:R], v["col_ids"][:N])

    def run(dev, dtype):
        csr = CSR(rowptr.to(dev), col.to(dev), N)
        x = v["x"].clone().to(device=dev, dtype=dtype).requires_grad_()  # (v is shared)
        drop = EdgeDrop(0.5, torch.tensor([SEED], device=dev), undirected)
        out = aggregate(x, csr, reduce=reduce, drop=drop, row_ids=ids[0].to(dev),
                        col_ids=ids[1].to(dev))
        out.backward(v["out0"][:R].to(device=dev, dtype=dtype))
        return out.detach().cpu(), x.grad.cpu()

    got, r64, r32 = run(DEV, torch.float32), run("cpu", torch.float64), run("cpu", torch.float32)
    for name, g, a, b in zip(("out", "dx"), got, r64, r32):
        _compare(f"aggregate {reduce} {'und' if undirected else 'dir'} {name}", f"op:{name}",
                 g, a, b)


def _layer_graph(dev):
    from dgraph_amd.data.synthetic import SHAPES, build_partition
    from dgraph_amd.parallel.dist_graph import DistGraph

    # built on the CPU and moved: the generator draws another graph on another device
    p = build_partition(SHAPES["ogbn-arxiv"].scaled(0.01), 0, 1, "cpu")
    return DistGraph(p["csr"].to(dev), p["L"], 0), p["L"]


def test_sage_conv_drop_edge_gpu_vs_cpu():
    from dgraph_amd.models.sage import SAGEConv

    def run(dev, dtype):
        graph, n = _layer_graph(dev)
        gen = torch.Generator().manual_seed(21)
        x = torch.randn(n, 32, generator=gen).to(device=dev, dtype=dtype).requires_grad_()
        gy = torch.randn(n, 64, generator=gen).to(device=dev, dtype=dtype)
        torch.manual_seed(0)
        layer = SAGEConv(32, 64, drop_edge=0.5).to(device=dev, dtype=dtype)
        out = layer(x, graph, drop_seed=SEED)
        out.backward(gy)
        return [t.detach().cpu() for t in (out, x.grad, layer.w_self.grad, layer.w_neigh.grad)]

    got, r64, r32 = run(DEV, torch.float32), run("cpu", torch.float64), run("cpu", torch.float32)
    for name, g, a, b in zip(("out", "dx", "dw_self", "dw_neigh"), got, r64, r32):
        _compare(f"SAGEConv(drop_edge=0.5) {name}", f"layer:{name}", g, a, b)


def test_captured_step_draws_a_new_subgraph_per_replay():
    """The layer's forward and backward captured once (``GraphedStep``): the step counter
    advances inside the capture, so two replays keep different edges, each the CPU count for
    its seed."""
    from dgraph_amd.models.sage import SAGEConv
    from dgraph_amd.ops import kernels as K
    from dgraph_amd.ops.aggregate import EdgeDrop
    from dgraph_amd.utils.graphed import GraphedStep

    graph, n = _layer_graph(DEV)
    cpu_graph, _ = _layer_graph("cpu")
    gen = torch.Generator().manual_seed(22)
    x = torch.randn(n, 32, generator=gen).to(DEV).requires_grad_()
    gy = torch.randn(n, 64, generator=gen).to(DEV)
    layer = SAGEConv(32, 64, drop_edge=0.5).to(DEV)
    stride = SAGEConv.DROP_SEED_STRIDE

    def step():
        out = layer(x, graph)
        torch.autograd.grad(out, (x, layer.w_neigh), gy)
        seed = layer.drop_base_seed + (layer.drop_step - 1) * stride  # this call's seed
        _, kept = graph.aggregate_drop(x.detach(), EdgeDrop(0.5, seed), True)
        return kept

    run = GraphedStep(step, warmup=1)
    run()  # warm-up, eager
    run()  # capture and first replay
    assert run.captured
    seen = []
    for _ in range(2):
        kept = run().clone()
        torch.cuda.synchronize()
        s = int(layer.drop_base_seed) + (int(layer.drop_step) - 1) * stride
        s = (s + 2 ** 63) % 2 ** 64 - 2 ** 63  # int64 wrap-around, as the device computes it
        it = cpu_graph.interior
        want = K.kept_degree(it.rowptr, it.col, seed=s, p=0.5, num_cols=n)
        assert torch.equal(kept.cpu(), want)
        seen.append(kept)
    assert not torch.equal(seen[0], seen[1])
    assert int(layer.drop_step) == 4
