"""The softmax aggregation kernels with edge features (csrc/kernels/spmm_softmax_edge.hip,
through ``K.segment_softmax_edge`` / ``K.segment_softmax_edge_bwd``),
``softmax_aggregate_edge``, ``dist_softmax_aggregate_edge`` and ``CommAwareGENConv(edge_dim=)``
on the GPU against the fp64 evaluation of their contract (tests/test_softmax_aggr_edge.py:
``edge_contract`` / ``edge_bwd_contract``, one slot at a time).

Inputs: the skewed CSR (300 rows over 257 columns, Poisson(7) degrees, row 0 with 5,000
entries, row 150 empty, rows 1 / 2 of degree 1 / 2) with ``x = randn`` and ``e = randn``; the
36,867-row pattern whose rows past 32,768 are a wave's SECOND row; ``100 + randn`` with
``t = +-2`` (``exp(200)`` is infinite in fp32).

Accuracy rule: ``|kernel - fp64| <= test_gat_kernels.bound(ref64, ref32)`` with ``ref32`` the
same contract in fp32 on the CPU; nothing is taken from the kernel's own output. ``lse`` is
compared on the non-empty rows (the empty row must hold ``-inf``). The backward kernel is given
the forward kernel's ``(out, lse)``; ``dx`` is the slot-transposed row sum of the kernel's
``de``. Largest ``error / bound`` seen on an MI355X (a record, not an input to the bound; every
figure is printed before it is asserted):

    forward, t = 1        out 0.145 (F = 600: err 8.9e-5, bound 6.2e-4)   lse 0.134
                          out of the degree-1 row 0.004
    backward, t = 1       de 0.061   dx 0.052   dt 0.126 (F = 600)
    a second row per wave out 0.007   lse 0.005   de 0.042 (second sweep 0.040)   dx 0.038
                          dt 0.007
    100 + randn, t = +-2  out 0.027   lse 0.004   de 0.088   dx 0.093   dt 0.144
    relu / eps flags      out 0.010   lse 0.006   de 0.020   dx 0.018   dt 0.016
    z == 0 and z < 0      out 0.064   lse 0.072   de 0.014   dx 0.012   dt 0.070; the masked
                          de rows are exact zeros
    per-channel t         out 0.093   lse 0.068   de 0.094   dx 0.094   dt 0.029
    column blocks         out 0.016   lse 0.017   de 0.026  dx 0.019   dt 0.023
    two sources           out 0.027   lse 0.029   per block: de 0.034   dx 0.042   dt 0.064
    op, hub source        out 0.011   dx 0.049   de 0.014   dt 0.326 (scalar t: err 2.1e-5,
                          bound 6.3e-5)
    W = 2 op              out 0.010   dx 0.022   de 0.027 (interior) / 0.024 (halo)   dt 0.007
    W = 2 layer           out 0.007   dx 0.012   every parameter gradient <= 0.019

The fp32 contract sums one slot at a time (test_softmax_aggr_edge.seg_sum), so the bounds are
those of a plain fp32 evaluation.
"""
from __future__ import annotations

import dataclasses
import functools

import pytest
import torch

import test_softmax_aggr_edge as E
from conftest import rank_device, run_ranks
from dgraph_amd.ops import kernels as K
from dgraph_amd.ops.aggregate import _slot_transpose, softmax_aggregate_edge
from dgraph_amd.ops.csr import CSR
from test_gat_kernels import bound
from test_pna import skewed_csr, values
from test_segment_cases import many_rows_csr
from test_softmax_aggr import SPLIT, split_csr

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.25e9  # what output buffers hold outside the blocks the kernel may write
NINF = float("-inf")
RATIOS: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(RATIOS):
        print(f"\n[softmax edge] largest error / bound, {k}: {RATIOS[k]:.3f}", end="")


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


@dataclasses.dataclass
class Case:
    """One input with the fp64 / fp32 contract of the forward and of the backward."""
    csr: CSR
    x: torch.Tensor
    e: torch.Tensor
    t: torch.Tensor
    g: torch.Tensor
    relu: bool
    eps: float
    f64: tuple  # (out, lse)
    f32: tuple
    b64: tuple  # (de, dx, dt)
    b32: tuple


def make_case(csr, x, e, t, g, relu=True, eps=1e-7, state=None):
    """``state``: the fp64 / fp32 ``(out, lse)`` to run the backward contract with (a block
    of a larger pattern is given the final state of the whole); default: this pattern's."""
    a = (csr.rowptr, csr.col.long(), x, e, t)
    f64 = E.edge_contract(*a, relu=relu, eps=eps)
    f32 = E.edge_contract(*a, relu=relu, eps=eps, dtype=torch.float32)
    s64, s32 = state if state is not None else (f64, f32)
    b64 = E.edge_bwd_contract(*a, g, *s64, relu=relu, eps=eps)
    b32 = E.edge_bwd_contract(*a, g, *s32, relu=relu, eps=eps, dtype=torch.float32)
    return Case(csr, x, e, t, g, relu, eps, f64, f32, b64, b32)


@functools.lru_cache(maxsize=None)
def skewed_case(F, tkind="one", xkind="plain", tscale=1.0, relu=True, eps=1e-7, kink=False):
    """The skewed case, shared by the index widths. ``kink``: slot 7 of row 0 has ``e = -x[col]``
    exactly (``z == 0``) and slots 100..139 of row 0 have ``z < 0`` in every channel."""
    csr = skewed_csr()
    x = values("plain", 257, F, F)
    if xkind == "offset":
        x = 100.0 + x
    e = values("plain", csr.nnz, F, 2000 + F)
    if kink:
        xs = x[csr.col.long()]
        e[7] = -xs[7]
        e[100:140] = -xs[100:140] - 1.0 - e[100:140].abs()
        assert bool((xs[7] + e[7] == 0).all()) and bool((xs[100:140] + e[100:140] < 0).all())
    t = temperature(tkind, F) * tscale
    g = values("plain", 300, F, 1000 + F)
    return make_case(csr, x, e, t, g, relu, eps)


def run_fwd(csr, c: Case, **kw):
    R, F = csr.num_rows, c.x.shape[1]
    out = torch.full((R, F), SENT, device=DEV)
    lse = torch.full((R, F), SENT, device=DEV)
    return K.segment_softmax_edge(csr.rowptr, csr.col, c.x.to(DEV), c.e.to(DEV), c.t.to(DEV),
                                  out, lse, relu=c.relu, eps=c.eps, **kw)


def check_bwd(tag, csr, c: Case, out, lse, num_sources=None):
    """The backward kernel on the device pattern ``csr`` with the forward KERNEL's ``(out,
    lse)``: every ``de`` row written into a sentinel buffer, ``dx`` as the slot-transposed
    row sum of it, the summed ``dt`` partials, and ``want_dt=False``."""
    F = c.x.shape[1]
    a = (csr.rowptr, csr.col, c.x.to(DEV), c.e.to(DEV), c.t.to(DEV), c.g.to(DEV), out, lse)
    kw = dict(relu=c.relu, eps=c.eps)
    de = torch.full((csr.nnz, F), SENT, device=DEV)
    de, part = K.segment_softmax_edge_bwd(*a, de, **kw)
    P = K.segment_softmax_edge_dt_parts(csr.num_rows)
    assert part.shape == (P, F) and P >= 1
    assert not bool((de == SENT).any())
    within(tag, "de", de, c.b64[0], c.b32[0])
    tt = _slot_transpose(CSR(csr.rowptr, csr.col, num_sources or c.x.shape[0]))
    within(tag, "dx", K.spmm(tt.rowptr, tt.perm, de), c.b64[1], c.b32[1])
    within(tag, "dt", part.double().sum(0), c.b64[2], c.b32[2])
    sent = torch.full((P, F), SENT, device=DEV)
    de2, none = K.segment_softmax_edge_bwd(*a, **kw, want_dt=False, dt_partials=sent)
    assert none is None and bool((sent == SENT).all()) and torch.equal(de2, de)
    return de, part


NE = skewed_csr().degree() > 0

# F -> (VEC, LPR, column passes) the launcher picks
VARIANTS = {1: (1, 8, 1), 3: (1, 8, 1), 13: (1, 16, 1), 30: (1, 32, 1), 70: (1, 64, 2),
            4: (4, 8, 1), 64: (4, 16, 1), 100: (4, 32, 1), 172: (4, 64, 1), 600: (4, 64, 3)}


def test_variant_table_restates_the_launcher():
    for F, (vec, lpr, passes) in VARIANTS.items():
        v = 4 if F % 4 == 0 else 1
        lanes = -(-F // v)
        l = 8 if lanes <= 8 else 16 if lanes <= 16 else 32 if lanes <= 32 else 64
        assert (v, l, -(-F // (l * v))) == (vec, lpr, passes)
    assert {(v, l) for v, l, _ in VARIANTS.values()} == {(v, l) for v in (1, 4)
                                                         for l in (8, 16, 32, 64)}


@pytest.mark.parametrize("F", sorted(VARIANTS))
@pytest.mark.parametrize("idx", [torch.int32, torch.int64])
def test_forward_and_backward(F, idx):
    c = skewed_case(F)
    csr = skewed_csr(idx).to(DEV)
    out, lse = run_fwd(csr, c)
    tag = f"fwd[F={F}]"
    check_fwd(tag, out, lse, c.f64, c.f32, NE)
    assert not bool(NE[150])  # the empty row: checked by check_fwd (0 and -inf)
    k = int(c.csr.rowptr[1])  # the degree-1 row: its one message
    m64 = E.messages(c.csr.col[k:k + 1], c.x.double(), c.e[k:k + 1].double(), True, c.eps)[1]
    m32 = E.messages(c.csr.col[k:k + 1], c.x, c.e[k:k + 1], True, c.eps)[1]
    within(tag, "out of the degree-1 row", out[1], m64[0], m32[0])
    check_bwd(f"bwd[F={F}]", csr, c, out, lse)


@functools.lru_cache(maxsize=None)
def many_case(F):
    csr = many_rows_csr()
    x = values("plain", csr.num_cols, F, 40 + F)
    e = values("plain", csr.nnz, F, 41 + F)
    g = values("plain", csr.num_rows, F, 42 + F)
    return make_case(csr, x, e, temperature("channel", F), g)


@pytest.mark.parametrize("F", [12, 70])
def test_a_second_row_per_wave(F):
    """36,867 rows, more than the 32,768 waves of the capped grid: rows past the cap are a
    wave's second row. ``de`` must be right there and the ``dt`` partials must accumulate
    across the rows of a wave (F = 70: also across two column passes)."""
    c = many_case(F)
    csr = many_rows_csr().to(DEV)
    assert csr.num_rows > 256 * 32 * 4 and K.segment_softmax_edge_dt_parts(csr.num_rows) == 8192
    out, lse = run_fwd(csr, c)
    ne = c.csr.degree() > 0
    check_fwd(f"many rows[F={F}]", out, lse, c.f64, c.f32, ne)
    de, _ = check_bwd(f"many rows[F={F}]", csr, c, out, lse)
    second = int(c.csr.rowptr[256 * 32 * 4])  # the first slot of the second sweep
    assert second < csr.nnz
    within(f"many rows[F={F}]", "de of the second sweep", de[second:], c.b64[0][second:],
           c.b32[0][second:])


@pytest.mark.parametrize("tscale", [2.0, -2.0])
def test_no_overflow_without_max_subtraction(tscale):
    """``x = 100 + randn`` at ``t = +-2``, F = 24: ``exp(+-200)`` overflows / underflows in
    fp32; everything is finite and within the bound."""
    c = skewed_case(24, "one", "offset", tscale)
    csr = skewed_csr(torch.int32).to(DEV)
    out, lse = run_fwd(csr, c)
    check_fwd(f"offset[t={tscale:+.0f}]", out, lse, c.f64, c.f32, NE)
    check_bwd(f"offset[t={tscale:+.0f}]", csr, c, out, lse)


@pytest.mark.parametrize("relu,eps", [(False, 1e-7), (True, 0.5), (False, 0.5)])
def test_message_flags(relu, eps):
    c = skewed_case(24, relu=relu, eps=eps)
    plain = skewed_case(24)
    assert float((c.f64[0] - plain.f64[0]).abs().max()) > 0.1  # the flag is visible
    csr = skewed_csr(torch.int32).to(DEV)
    out, lse = run_fwd(csr, c)
    check_fwd(f"flags[relu={relu}, eps={eps}]", out, lse, c.f64, c.f32, NE)
    check_bwd(f"flags[relu={relu}, eps={eps}]", csr, c, out, lse)


@pytest.mark.parametrize("F", [24, 30])
def test_relu_mask_is_exact(F):
    """One slot with ``e = -x[col]`` exactly (``z == 0``) and forty with ``z < 0`` under
    ``relu=True``: their ``de`` rows are exact zeros (VEC 4 and VEC 1); the bound holds
    everywhere else; without relu the same slots have a gradient."""
    c = skewed_case(F, kink=True)
    csr = skewed_csr(torch.int32).to(DEV)
    out, lse = run_fwd(csr, c)
    check_fwd(f"kink[F={F}]", out, lse, c.f64, c.f32, NE)
    de, _ = check_bwd(f"kink[F={F}]", csr, c, out, lse)
    assert torch.count_nonzero(de[7]) == 0 and torch.count_nonzero(de[100:140]) == 0
    assert torch.count_nonzero(c.b64[0][7]) == 0 and torch.count_nonzero(c.b64[0][100:140]) == 0
    pos = (c.x[c.csr.col.long()] + c.e > 0).to(DEV)
    assert float((de != 0)[pos].float().mean()) > 0.99 and not bool((de != 0)[~pos].any())
    n = skewed_case(F, relu=False, kink=True)
    o2, l2 = run_fwd(csr, n)
    de2, _ = check_bwd(f"kink, no relu[F={F}]", csr, n, o2, l2)
    assert torch.count_nonzero(de2[7]) == F


def test_per_channel_temperature():
    """F = 64, ``t = linspace(-3, 3)`` with one element exactly 0: forward and backward."""
    c = skewed_case(64, "channel")
    assert bool((c.t == 0).any()) and bool((c.t < 0).any()) and bool((c.t > 0).any())
    csr = skewed_csr(torch.int32).to(DEV)
    out, lse = run_fwd(csr, c)
    check_fwd("channel t[F=64]", out, lse, c.f64, c.f32, NE)
    check_bwd("channel t[F=64]", csr, c, out, lse)


@pytest.mark.parametrize("F,pad", [(3, 1), (64, 4)])
def test_operands_as_column_blocks(F, pad):
    """``x``, ``e``, ``out``, ``lse``, ``g`` and ``de`` as column blocks at offset ``pad`` of
    wider sentinel-filled buffers (F = 3: row strides 5 and 8, no multiple of 4: VEC 1;
    F = 64: 16-B aligned blocks: VEC 4): nothing outside the blocks is written."""
    c = skewed_case(F)
    csr = skewed_csr(torch.int32).to(DEV)
    nnz = csr.nnz

    def wide(v, rows):
        w = torch.full((rows, F + 2 * pad), SENT, device=DEV)
        if v is not None:
            w[:, pad:pad + F] = v.to(DEV)
        return w, w[:, pad:pad + F]

    _, xb = wide(c.x, 257)
    _, eb = wide(c.e, nnz)
    _, gb = wide(c.g, 300)
    ow = torch.full((300, 2 * F + 2 * pad), SENT, device=DEV)
    out, lse = ow[:, pad:pad + F], ow[:, pad + F:pad + 2 * F]
    td = c.t.to(DEV)
    K.segment_softmax_edge(csr.rowptr, csr.col, xb, eb, td, out, lse)
    check_fwd(f"blocks[F={F}]", out, lse, c.f64, c.f32, NE)
    assert bool((ow[:, :pad] == SENT).all()) and bool((ow[:, pad + 2 * F:] == SENT).all())
    assert not bool((ow[:, pad:pad + 2 * F] == SENT).any())
    dw, db = wide(None, nnz)
    de, part = K.segment_softmax_edge_bwd(csr.rowptr, csr.col, xb, eb, td, gb, out, lse, db)
    within(f"blocks[F={F}]", "de", de, c.b64[0], c.b32[0])
    within(f"blocks[F={F}]", "dt", part.double().sum(0), c.b64[2], c.b32[2])
    assert bool((dw[:, :pad] == SENT).all()) and bool((dw[:, pad + F:] == SENT).all())
    assert not bool((db == SENT).any())
    tt = _slot_transpose(CSR(csr.rowptr, csr.col, 257))
    within(f"blocks[F={F}]", "dx", K.spmm(tt.rowptr, tt.perm, db), c.b64[1], c.b32[1])


def test_a_misaligned_edge_block_raises():
    """A width that is a multiple of 4 whose ``e`` (or ``de``) has a row stride or base off
    the 16-B grid raises, as ``segment_softmax`` does for ``x``: no silent VEC 1 run."""
    c = skewed_case(64)
    csr = skewed_csr(torch.int32).to(DEV)
    x, t, g = c.x.to(DEV), c.t.to(DEV), c.g.to(DEV)
    out, lse = run_fwd(csr, c)
    err = (RuntimeError, ValueError)
    for lo, w in ((0, 66), (1, 68)):  # the row stride; the base
        e = torch.zeros(csr.nnz, w, device=DEV)[:, lo:lo + 64]
        e.copy_(c.e)
        with pytest.raises(err):
            K.segment_softmax_edge(csr.rowptr, csr.col, x, e, t)
        with pytest.raises(err):
            K.segment_softmax_edge_bwd(csr.rowptr, csr.col, x, e, t, g, out, lse)
        with pytest.raises(err):
            K.segment_softmax_edge_bwd(csr.rowptr, csr.col, x, c.e.to(DEV), t, g, out, lse,
                                       torch.empty(csr.nnz, w, device=DEV)[:, lo:lo + 64])
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def split_cases(F=40):
    """The unsplit case and each block's, the blocks' backward contracts with the FINAL
    state of the unsplit pattern."""
    full, a, b = split_csr()
    x = values("plain", 257, F, 31)
    e = values("plain", full.nnz, F, 32)
    g = values("plain", 300, F, 77)
    t = temperature("channel", F)
    whole = make_case(full, x, e, t, g)
    ea, eb = full.split_edge_values(SPLIT, e)
    state = (whole.f64, whole.f32)
    ca = make_case(a, x[:SPLIT].contiguous(), ea.contiguous(), t, g, state=state)
    cb = make_case(b, x[SPLIT:].contiguous(), eb.contiguous(), t, g, state=state)
    return whole, ca, cb


@pytest.mark.parametrize("row_map", [False, True])
@pytest.mark.parametrize("idx", [torch.int32, torch.int64])
def test_two_sources_match_the_unsplit_csr(idx, row_map):
    """Pass 1 over columns < 130, pass 2 (carry mode) over the rest, over all rows or
    row-compacted: the fp64 contract on the unsplit CSR within the bound; rows without an
    entry in the second block are bitwise those of pass 1. Then the backward on each block
    with the final ``(out, lse)``: ``de``, ``dx`` of its sources through the slot-transposed
    SpMM, and its part of ``dt``, against the contract restricted to that edge set."""
    whole, ca, cb = split_cases()
    full, a, b = split_csr(idx)
    out, lse, o1, l1 = E.two_pass_edge(a.to(DEV), b.to(DEV), whole.x.to(DEV), ca.e.to(DEV),
                                       cb.e.to(DEV), whole.t.to(DEV), row_map)
    ne = full.degree() > 0
    check_fwd("two sources", out, lse, whole.f64, whole.f32, ne)
    absent = (b.degree() == 0).to(DEV)
    assert int(absent.sum()) > 1 and bool(absent[2]) and bool(absent[150])
    assert torch.equal(out[absent], o1[absent]) and torch.equal(lse[absent], l1[absent])
    assert torch.count_nonzero(o1[1]) == 0 and bool((l1[1] == NINF).all())  # empty, then filled
    for name, blk, c in (("interior", a, ca), ("halo", b, cb)):
        check_bwd(f"split bwd[{name}]", blk.to(DEV), c, out, lse)
    dt = ca.b64[2] + cb.b64[2]
    torch.testing.assert_close(dt, whole.b64[2], atol=1e-10, rtol=1e-10)


def test_op_on_a_pattern_with_a_hub_source():
    """``softmax_aggregate_edge`` on the transposed skewed pattern (257 rows; source 0 has
    5,000 entries, so the ``dx`` row sum takes the hub split) with a learnable scalar ``t``
    (F = 8): out, dx, de and the scalar's gradient."""
    tp = skewed_csr().transpose()
    csr = CSR(tp.rowptr, tp.col.to(torch.int32), 300)
    tt = _slot_transpose(csr)
    assert tt.hub_split(2048) is not None
    x, e = values("plain", 300, 8, 61), values("plain", csr.nnz, 8, 62)
    gy = values("plain", 257, 8, 63)
    refs = []
    for dt in (torch.float64, torch.float32):
        o, l = E.edge_contract(csr.rowptr, csr.col.long(), x, e, 0.7, dtype=dt)
        de, dx, dtp = E.edge_bwd_contract(csr.rowptr, csr.col.long(), x, e, 0.7, gy, o, l,
                                          dtype=dt)
        refs.append((o, dx, de, dtp.sum().reshape(1)))
    xi, ei = x.to(DEV).requires_grad_(), e.to(DEV).requires_grad_()
    ti = torch.tensor([0.7], device=DEV, requires_grad=True)
    out = softmax_aggregate_edge(xi, ei, csr.to(DEV), ti)
    out.backward(gy.to(DEV))
    assert ti.grad.shape == (1,)
    for name, got, i in (("out", out, 0), ("dx", xi.grad, 1), ("de", ei.grad, 2),
                         ("dt", ti.grad, 3)):
        within("op, hub source", name, got, refs[0][i], refs[1][i])


def test_bitwise_deterministic():
    csr = skewed_csr(torch.int32, seed=9).to(DEV)
    x = values("plain", 257, 172, 9).to(DEV)
    e = values("plain", csr.nnz, 172, 11).to(DEV)
    gy = values("plain", 300, 172, 10).to(DEV)
    res = []
    for _ in range(2):
        xi, ei = x.clone().requires_grad_(), e.clone().requires_grad_()
        ti = temperature("channel", 172).to(DEV).requires_grad_()
        out = softmax_aggregate_edge(xi, ei, csr, ti)
        out.backward(gy)
        res.append((out.detach(), xi.grad, ei.grad, ti.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_contract_checks_raise():
    csr = skewed_csr(torch.int32).to(DEV)
    nnz = csr.nnz
    x = values("plain", 257, 8, 1).to(DEV)
    e = values("plain", nnz, 8, 2).to(DEV)
    t = torch.ones(8, device=DEV)
    new = lambda F=8, dt=torch.float32: torch.empty(300, F, dtype=dt, device=DEV)  # noqa: E731
    call = lambda xx, ee, tt, o, l, **kw: K.segment_softmax_edge(  # noqa: E731
        csr.rowptr, csr.col, xx, ee, tt, o, l, **kw)
    err = (RuntimeError, ValueError, TypeError)
    with pytest.raises(err):  # e with the wrong row count
        call(x, e[:-1], t, new(), new())
    with pytest.raises(err):  # e with the wrong width
        call(x, e[:, :4].contiguous(), t, new(), new())
    with pytest.raises(err):
        K._native.ops().segment_softmax_edge_fwd(csr.rowptr, csr.col, x, e[:-1], t, new(), new(),
                                                 True, 1e-7, False, None)
    with pytest.raises(err):  # non-fp32 on the GPU
        call(x.double(), e.double(), t.double(), new(dt=torch.float64), new(dt=torch.float64))
    with pytest.raises(err):
        call(x, e.half(), t, new(), new())
    with pytest.raises(err):
        K._native.ops().segment_softmax_edge_fwd(csr.rowptr, csr.col, x, e.half(), t, new(),
                                                 new(), True, 1e-7, False, None)
    with pytest.raises(err):  # a column stride
        call(x, e.t().contiguous().t(), t, new(), new())
    with pytest.raises(err):
        call(x.t().contiguous().t(), e, t, new(), new())
    with pytest.raises(err):  # a t of the wrong length
        call(x, e, torch.ones(7, device=DEV), new(), new())
    with pytest.raises(err):  # outputs with fewer rows than the CSR
        call(x, e, t, new()[:100], new()[:100])
    with pytest.raises(err):  # carry mode without an incumbent
        K.segment_softmax_edge(csr.rowptr, csr.col, x, e, t, second=True)
    out, lse = call(x, e, t, new(), new())
    g = new()
    bwd = lambda *a, **kw: K.segment_softmax_edge_bwd(csr.rowptr, csr.col, *a, **kw)  # noqa: E731
    with pytest.raises(err):  # too few de rows
        bwd(x, e, t, g, out, lse, torch.empty(nnz - 1, 8, device=DEV))
    with pytest.raises(err):
        K._native.ops().segment_softmax_edge_bwd(csr.rowptr, csr.col, x, e, t, g, out, lse,
                                                 torch.empty(nnz - 1, 8, device=DEV), True, 1e-7,
                                                 None)
    with pytest.raises(err):  # a partial buffer of the wrong row count
        bwd(x, e, t, g, out, lse, dt_partials=torch.empty(1, 8, device=DEV))
    with pytest.raises(err):
        K._native.ops().segment_softmax_edge_bwd(csr.rowptr, csr.col, x, e, t, g, out, lse,
                                                 torch.empty(nnz, 8, device=DEV), True, 1e-7,
                                                 torch.empty(1, 8, device=DEV))
    with pytest.raises(err):  # fewer lse rows than CSR rows
        bwd(x, e, t, g, out, lse[:100])
    with pytest.raises(err):  # e narrower than x
        bwd(x, e[:, :4].contiguous(), t, g, out, lse)
    # empty launches return without launching
    none_rp = torch.zeros(1, dtype=torch.long, device=DEV)
    none_col = torch.zeros(0, dtype=torch.int32, device=DEV)
    o, l = K.segment_softmax_edge(none_rp, none_col, x, e[:0], t)
    assert o.shape == (0, 8) and K.segment_softmax_edge_dt_parts(0) == 0
    de, part = K.segment_softmax_edge_bwd(none_rp, none_col, x, e[:0], t, g[:0], out[:0], lse[:0])
    assert de.shape == (0, 8) and part.shape == (0, 8)
    rp0 = torch.zeros(301, dtype=torch.long, device=DEV)
    o, l = K.segment_softmax_edge(rp0, none_col, x, e[:0], t)  # rows without entries
    assert torch.count_nonzero(o) == 0 and bool((l == NINF).all())
    keep_o, keep_l = out.clone(), lse.clone()
    K.segment_softmax_edge(rp0, none_col, x, e[:0], t, out, lse, second=True)
    assert torch.equal(out, keep_o) and torch.equal(lse, keep_l)
    de, part = K.segment_softmax_edge_bwd(rp0, none_col, x, e[:0], t, g, out, lse)
    assert de.shape == (0, 8) and torch.count_nonzero(part) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ op and layer, W = 2
def _tiny_shape():
    from dgraph_amd.data.synthetic import SHAPES

    return dataclasses.replace(SHAPES["ogbn-arxiv"], name="tiny-64", num_nodes=64,
                               num_directed_edges=400)


def _to_cpu(p):
    return dict(p, csr=p["csr"].to("cpu"), halo_gids=p["halo_gids"].cpu())


def _cpu_single_rank(fn, shape, dev):
    """``fn(dtype, graph, partition, rank, device)`` on the whole graph on the CPU in fp64
    and in fp32. The graph is generated on ``dev`` like the ranks' parts (the synthetic
    generator draws from the device's random stream) and moved over."""
    from dgraph_amd.data.synthetic import build_partition
    from dgraph_amd.parallel.dist_graph import DistGraph

    p = _to_cpu(build_partition(shape, 0, 1, dev))
    res = []
    for dt in (torch.float64, torch.float32):
        res.append(fn(dt, DistGraph(p["csr"], p["L"], 0), p, 0, "cpu"))
    return res


def _rank_graph(shape, rank, world, dev):
    from dgraph_amd.data.synthetic import build_partition
    from dgraph_amd.parallel.dist_graph import DistGraph

    p = build_partition(shape, rank, world, dev)
    g = DistGraph(p["csr"], p["L"], p["H"], p["send_local_idx"], p["send_splits"],
                  p["recv_splits"])
    return g, p


def _de_table(p, de_int, N):
    """W = 1: the edge gradient by ``gdst * N + gsrc`` (parallel edges share it)."""
    gdst, gsrc = E.global_slot_ids(p, 0)
    key, order = torch.sort(gdst * N + gsrc)
    return key, de_int.cpu()[order]


def _w2_op_body(rank, world):
    import torch.distributed as dist

    from dgraph_amd.data.synthetic import build_partition
    from dgraph_amd.parallel.dist_graph import dist_softmax_aggregate_edge

    shape = _tiny_shape()
    N = shape.num_nodes

    def run(dt, graph, p, r, dev):
        sl = slice(p["offsets"][r], p["offsets"][r + 1])
        x, gy, t = E._global_inputs(dt, dev, shape)
        e_int, e_halo, i_int, i_halo = E.partition_edges(p, r, E.DF, dt, dev)
        xl, t = x[sl].clone().requires_grad_(), t.requires_grad_()
        e_int, e_halo = e_int.requires_grad_(), e_halo.requires_grad_()
        out = dist_softmax_aggregate_edge(xl, e_int, e_halo, graph, t)
        out.backward(gy[sl])
        de_halo = e_halo.grad if e_halo.grad is not None else torch.zeros_like(e_halo)
        return out.detach(), xl.grad, t.grad, e_int.grad, de_halo, i_int, i_halo, sl

    dev = rank_device()
    p1 = _to_cpu(build_partition(shape, 0, 1, dev))
    r64, r32 = _cpu_single_rank(run, shape, dev)
    graph, p = _rank_graph(shape, rank, world, dev)
    assert graph.halo is not None and graph.halo.nnz > 0
    out, dx, gt, de_int, de_halo, i_int, i_halo, sl = run(torch.float32, graph, p, rank, dev)
    dist.all_reduce(gt)
    within("W=2 op", "out", out, r64[0][sl], r32[0][sl])
    within("W=2 op", "dx", dx, r64[1][sl], r32[1][sl])
    within("W=2 op", "dt", gt, r64[2], r32[2])
    t64, t32 = _de_table(p1, r64[3], N), _de_table(p1, r32[3], N)
    within("W=2 op", "de interior", de_int, E.lookup(t64, i_int, N), E.lookup(t32, i_int, N))
    within("W=2 op", "de halo", de_halo, E.lookup(t64, i_halo, N), E.lookup(t32, i_halo, N))


def _w2_layer_body(rank, world):
    import torch.distributed as dist

    shape = _tiny_shape()
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(shape.num_nodes, E.LF, generator=gen)
    gy = torch.randn(shape.num_nodes, E.LOUT, generator=gen)

    def run(dt, graph, p, r, dev):
        sl = slice(p["offsets"][r], p["offsets"][r + 1])
        layer = E.make_layer(3).to(device=dev, dtype=dt)
        a_int, a_halo, _, _ = E.partition_edges(p, r, 3, dt, dev)
        xl = x[sl].to(device=dev, dtype=dt).requires_grad_()
        out = layer(xl, graph, (a_int, a_halo))
        (out * gy[sl].to(device=dev, dtype=dt)).sum().backward()
        return out.detach(), xl.grad, {n: q.grad for n, q in layer.named_parameters()}, sl

    dev = rank_device()
    r64, r32 = _cpu_single_rank(run, shape, dev)
    graph, p = _rank_graph(shape, rank, world, dev)
    out, dx, grads, sl = run(torch.float32, graph, p, rank, dev)
    within("W=2 layer", "out", out, r64[0][sl], r32[0][sl])
    within("W=2 layer", "dx", dx, r64[1][sl], r32[1][sl])
    assert "lin_edge.weight" in grads and "t" in grads
    for n, gq in grads.items():
        dist.all_reduce(gq)
        within("W=2 layer", f"grad {n}", gq, r64[2][n], r32[2][n])
    assert float(grads["t"].abs().max()) > 0 and float(grads["lin_edge.weight"].abs().max()) > 0


def _w2_body(rank, world):
    from dgraph_amd.comm.rccl_exec import RCCLExecutor

    _w2_op_body(rank, world)
    _w2_layer_body(rank, world)
    torch.cuda.synchronize()
    RCCLExecutor.close_all()


def test_op_and_layer_two_ranks_rccl():
    """At W = 2 over real RCCL (both ranks on GPU 0, a 64-vertex graph, one process group for
    both): dist_softmax_aggregate_edge forward, dx, both de blocks and the all-reduced dt
    against the CPU fp64 result, then CommAwareGENConv(edge_dim=3) against the same layer on
    the CPU in fp64, every parameter gradient (the temperature's and lin_edge's included)
    after the all-reduce."""
    run_ranks(_w2_body, 2, backend="rccl-one-gpu")
