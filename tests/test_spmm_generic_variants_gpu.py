"""Every compiled instantiation of csrc/kernels/spmm.hip -- the generic CSR SpMM in its two
data flows (variants 1 and 2), the bf16 row-group kernel (variant 4) and the two hub-split
kernels -- against the fp64 formula of test_spmm_generic_cases.py, which holds the inputs,
the oracles, the case table (``TABLE``: which instantiation each case reaches, by the
launchers' rules restated) and the CPU tests showing that the comparisons bite.

* ``test_exact[group]``: the table, a group at a time; bitwise (``assert_exact``). The
  ``many-*`` groups run the 36,867-row pattern: ``beta = 0`` into a sentinel-filled output
  (a skipped row keeps it, an empty visited row must be 0), then ``beta != 0`` (a row
  visited twice accumulates twice).
* the hub kernels through the raw ops with hand-made segments, then the whole split path
  ``K.spmm(split=...)``; empty shapes; one full-mantissa pass per kernel family and element
  type; ``edge_softmax_fwd`` / ``edge_softmax_bwd`` (the ``[E, heads]`` weights of the
  multi-head SpMM) at every lanes-per-edge width against fp64.

Every ``set_spmm_config`` / ``set_spmm_f32_config`` is restored in a ``finally``.
"""
from __future__ import annotations

import contextlib
import functools

import pytest
import torch

import test_spmm_generic_cases as G
from dgraph_amd.ops import kernels as K
from dgraph_amd.ops import reference as R
from test_gat_kernels import bound
from test_segment_cases import ladder_csr, with_idx

pytestmark = pytest.mark.gpu
DEV = "cuda"
TDT = {"f32": torch.float32, "bf16": torch.bfloat16}
IDT = {"i32": torch.int32, "i64": torch.int64}


def _ops():
    from dgraph_amd import _native

    return _native.ops()


@contextlib.contextmanager
def config(variant=4, xcd=0, pc=128, rg32=False):
    """The SpMM configuration of a run; the defaults restored on the way out."""
    ops = _ops()
    try:
        ops.set_spmm_config(-1, -1)
        ops.set_spmm_config(variant, xcd, pc)
        ops.set_spmm_f32_config(1 if rg32 else 0)
        yield ops
    finally:
        ops.set_spmm_config(-1, -1)
        ops.set_spmm_f32_config(1)


def placed(t: torch.Tensor, dtype, view):
    """``t`` on the device in ``dtype``: contiguous, or (``view = (offset, stride)``) a
    column slice of a sentinel-filled ``[rows, stride]`` buffer. (buffer or None, tensor)."""
    if view is None:
        return None, t.to(dtype).to(DEV).contiguous()
    off, ld = view
    assert off + t.shape[1] <= ld
    buf = torch.full((t.shape[0], ld), G.SENT, dtype=dtype, device=DEV)
    v = buf[:, off:off + t.shape[1]]
    v.copy_(t)
    return buf, v


def untouched(buf, view, F) -> bool:
    if buf is None:
        return True
    b = buf.float().cpu()
    return bool((b[:, :view[0]] == G.SENT).all() and (b[:, view[0] + F:] == G.SENT).all())


@functools.lru_cache(maxsize=None)
def _pattern_dev(pat, idx):
    csr = G.csr_of(pat)
    return (csr.rowptr.to(DEV), csr.col.to(IDT[idx]).to(DEV),
            None if csr.row_map is None else csr.row_map.to(DEV))


def run_gpu(c, spec: G.CallSpec, run: G.RunSpec) -> torch.Tensor:
    """The call through the raw op under the run's configuration; the output buffer (CPU).
    The columns around a column-slice operand must keep the sentinel."""
    rowptr, col, row_map = _pattern_dev(spec.pat, run.idx)
    dev = lambda k: None if c.get(k) is None else c[k].to(DEV).contiguous()  # noqa: E731
    xbuf, x = placed(c["x"], TDT[run.dt], run.view)
    obuf, out = placed(c["out0"], TDT[run.dt], run.view)
    F = spec.F
    with config(run.variant, run.xcd, run.pc, run.rg32) as ops:
        ops.spmm(rowptr, col, dev("edge_weight"), dev("col_scale"), dev("row_scale"), x, out,
                 spec.heads, F // spec.heads, float(c["beta"]), int(spec.cap), row_map)
        torch.cuda.synchronize()
    assert untouched(xbuf, run.view, F) and untouched(obuf, run.view, F), (spec, run)
    return out.cpu()


@pytest.mark.parametrize("group", list(G.TABLE))
def test_exact(group):
    for spec, runs in G.TABLE[group]:
        if spec.pat == "many":
            c = G.make_call(spec)
            ref = G.formula(c)
            G.exact_ok(c, ref)
        else:
            c, ref = G.ladder_case(spec)
        for run in runs:
            try:
                G.assert_exact(run_gpu(c, spec, run), c, run.dt, ref, checked=True)
            except AssertionError as e:
                raise AssertionError(f"{spec} {run}: {e}") from e


# ------------------------------------------------------------------------------ hub kernels
@pytest.mark.parametrize("dt,F,view", list(G.HUB_CASES), ids=str)
def test_hub_partials(dt, F, view):
    """``spmm_hub_partials`` on the hand-made segments (lengths 1 .. 1,027), every weighting,
    both index types; the partials are fp32 and compared as fp32, bitwise."""
    ops = _ops()
    for fam in G.FAMS:
        c = G.make_hub_call(F, fam)
        ref = G.hub_oracle(c)
        G.hub_exact_ok(c, ref)
        dev = lambda k: None if c.get(k) is None else c[k].to(DEV)  # noqa: E731
        for idx in G.IDX:
            xbuf, x = placed(c["x"], TDT[dt], view)
            part = torch.full((len(G.SEG_LENS) + 1, F), G.SENT, device=DEV)
            ops.spmm_hub_partials(dev("beg"), dev("end"), c["col"].to(IDT[idx]).to(DEV),
                                  dev("ew"), dev("cs"), x, part)
            torch.cuda.synchronize()
            G.assert_same(part[:-1], ref)
            assert bool((part[-1] == G.SENT).all()) and untouched(xbuf, view, F), (fam, idx)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("F", [6, 47, 130])
def test_hub_reduce(F, dt):
    """``spmm_hub_reduce``: hubs of 1, 3 and 5 segments, with and without ``row_scale``,
    contiguous and strided output; the rows of no hub and the columns around the slice keep
    their contents."""
    ops = _ops()
    for scaled in (False, True):
        c = G.make_reduce_call(F, scaled)
        want = G.expect(G.reduce_formula(c), dt)
        for view in (None, (3, F + 5)):
            obuf, out = placed(c["out0"], TDT[dt], view)
            ops.spmm_hub_reduce(c["part"].to(DEV), c["seg_ptr"].to(DEV), c["rows"].to(DEV),
                                None if not scaled else c["rs"].to(DEV), out)
            torch.cuda.synchronize()
            G.assert_same(out, want)
            assert untouched(obuf, view, F)


def _split_run(c, dt, idx, cap, compact, rg32):
    csr = with_idx(ladder_csr(), IDT[idx]).to(DEV)
    if compact:
        csr = csr.compact_rows()
    split = csr.hub_split(cap)
    assert split is not None and split.cap == cap
    dev = lambda k: None if c.get(k) is None else c[k].to(DEV)  # noqa: E731
    out = c["out0"].to(TDT[dt]).to(DEV)
    with config(rg32=rg32):
        K.spmm(csr.rowptr, csr.col, c["x"].to(TDT[dt]).to(DEV), out,
               edge_weight=dev("edge_weight"), col_scale=dev("col_scale"),
               row_scale=dev("row_scale"), beta=c["beta"], split=split, row_map=csr.row_map)
        torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("cap", G.SPLIT_CAPS)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_split_path(dt, cap):
    """``K.spmm(split=...)`` on the ladder, plain and compacted: the capped main pass, the
    segment partials and the reduce together. bf16 rounds at the main pass's store and at
    the reduce's (``split_expect``). fp32 runs on the generic kernels and, left to the
    defaults, on the fp32 row-group kernel."""
    for F in G.SPLIT_F[dt]:
        for spec in G.split_specs(F):
            c, _ = G.ladder_case(spec)
            want = G.split_expect(c, cap, dt)
            for idx in G.IDX:
                for rg32 in ((False, True) if dt == "f32" else (False,)):
                    got = _split_run(c, dt, idx, cap, spec.pat == "ladderc", rg32)
                    G.assert_same(got, want)


# ------------------------------------------------------------------------------ empty shapes
@pytest.mark.parametrize("variant", [1, 2, 4])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_empty_shapes(dt, variant):
    F, n = 24, 9
    g = G.gen("empty", dt, variant)
    out0 = G.ints((n, F), g)
    rs = G.pick(G.ALPHABETS["scale"], (n,), g).to(DEV)
    x = G.ints((5, F), g).to(TDT[dt]).to(DEV)
    for idx in G.IDX:
        col = torch.zeros(0, dtype=IDT[idx], device=DEV)
        with config(variant, 0, 128) as ops:
            # zero rows: nothing is written
            out = out0.to(TDT[dt]).to(DEV)
            ops.spmm(torch.zeros(1, dtype=torch.long, device=DEV), col, None, None, rs, x, out,
                     1, F, 0.5, 0, None)
            assert torch.equal(out.float().cpu(), out0)
            # zero entries: exactly beta * out0 (and 0 with beta = 0), also from a source
            # of zero rows
            rowptr = torch.zeros(n + 1, dtype=torch.long, device=DEV)
            for src in (x, x[:0]):
                for beta in (0.0, 0.5, -2.0):
                    out = out0.to(TDT[dt]).to(DEV)
                    ops.spmm(rowptr, col, None, None, rs, src, out, 1, F, beta, 0, None)
                    torch.cuda.synchronize()
                    G.assert_same(out, G.expect(beta * out0.double(), dt))


# ------------------------------------------------------------------------------ full mantissa
@pytest.mark.parametrize("dt,variant", [("f32", 1), ("f32", 2), ("bf16", 1), ("bf16", 2),
                                        ("bf16", 4)])
def test_unit_normal(dt, variant):
    """Unit-normal values, one pass per kernel family and element type: fp32 within
    ``bound``; bf16 (inputs rounded to bf16 first) within ``bound`` plus ``2^-8 |ref|`` for
    its one rounding. Variant 4 is the bf16 row-group kernel where the width allows it."""
    for spec in G.NORMAL_SPECS:
        c, ref64, ref32 = G.normal_case(spec, dt)
        for idx in G.IDX:
            run = G.RunSpec(dt, idx, variant, 0, 512)
            G.assert_bound(run_gpu(c, spec, run), ref64, ref32, dt,
                           label=f"{G.reach(spec, run)[0][0]} F={spec.F} {idx}")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_unit_normal_hub(dt):
    """... the fp32 partials under ``bound``, and the split path (bf16: two roundings, the
    first at the main pass's value)."""
    ops = _ops()
    for F in (47, 130):
        c = G.make_hub_call(F, "w3", normal=True)
        if dt == "bf16":
            c = dict(c, x=c["x"].bfloat16().float())
        part = torch.empty(len(G.SEG_LENS), F, device=DEV)
        ops.spmm_hub_partials(c["beg"].to(DEV), c["end"].to(DEV), c["col"].to(DEV),
                              c["ew"].to(DEV), c["cs"].to(DEV), c["x"].to(TDT[dt]).to(DEV), part)
        G.assert_bound(part, G.hub_oracle(c), G.hub_oracle(c, torch.float32), "f32",
                       label=f"hub_partials<{dt}> F={F}")
    for spec in G.NORMAL_SPECS:
        if spec.heads > 1:
            continue
        for cap in G.SPLIT_CAPS:
            c, ref64, ref32, main = G.split_normal_case(spec, dt, cap)
            got = _split_run(c, dt, "i32", cap, False, False)
            G.assert_bound(got, ref64, ref32, dt, (main,), f"split cap={cap} F={spec.F}")


# ------------------------------------------------------------------------------ edge softmax
@pytest.mark.parametrize("H", G.EDGE_SOFTMAX_H)
def test_edge_softmax_ladder(H):
    """``edge_softmax_fwd`` / ``_bwd`` at every lanes-per-edge width (1 .. 64, and head
    counts that leave lanes of an edge idle) on the ladder, against the fp64 softmax and
    its adjoint under ``bound`` (whose factor covers ``__expf``). Row 0 is empty; every
    entry belongs to a row, so every weight is written and none is NaN."""
    csr = ladder_csr()
    g = G.gen("edge_softmax", H)
    s = torch.randn(csr.nnz, H, generator=g) * 5
    s[:3] += 80.0  # large scores: the max subtraction must keep this finite
    gr = torch.randn(csr.nnz, H, generator=g)
    a64, a32 = R.edge_softmax_fwd(csr.rowptr, s.double()), R.edge_softmax_fwd(csr.rowptr, s)
    rowptr = csr.rowptr.to(DEV)
    a = K.edge_softmax_fwd(rowptr, s.to(DEV)).cpu()
    assert a.shape == s.shape and bool(torch.isfinite(a).all())
    err, lim = float((a.double() - a64).abs().max()), bound(a64, a32)
    print(f"edge_softmax_fwd H={H} err {err:.3e} bound {lim:.3e}")
    assert err <= lim, (err, lim)
    sums = torch.zeros(csr.num_rows, H, dtype=torch.float64).index_add_(0, csr.row_ids(),
                                                                         a.double())
    ne = csr.degree() > 0
    torch.testing.assert_close(sums[ne], torch.ones_like(sums[ne]), atol=1e-5, rtol=0)
    # the adjoint on the same fp32 weights
    al = a64.float()
    d64 = R.edge_softmax_bwd(csr.rowptr, al.double(), gr.double())
    d32 = R.edge_softmax_bwd(csr.rowptr, al, gr)
    d = K.edge_softmax_bwd(rowptr, al.to(DEV), gr.to(DEV)).cpu()
    assert bool(torch.isfinite(d).all())
    err, lim = float((d.double() - d64).abs().max()), bound(d64, d32)
    print(f"edge_softmax_bwd H={H} err {err:.3e} bound {lim:.3e}")
    assert err <= lim, (err, lim)
