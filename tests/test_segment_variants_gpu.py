"""Every (VEC, LPR) instantiation of the three wave-per-row gather families on the GPU --
``segment_softmax_fwd / bwd`` (csrc/kernels/spmm_softmax.hip), ``segment_pna_fwd / bwd``
(spmm_pna.hip), ``segment_extreme_fwd / bwd`` (spmm_max.hip) -- against the fp64 contracts
of tests/test_softmax_aggr.py and tests/test_pna.py. Inputs, references and the table of
widths come from tests/test_segment_cases.py, which pins them down on the CPU.

(a) the ladder (degrees 0..136, a 1,027-entry row, four rows that repeat one source) at every
    width of ``VARIANTS``, int32 and int64 column ids (of the transposed pattern too);
(b) two sources on the ladder split at column 130, F = 128 (VEC 4 LPR 32) and 29 (VEC 1
    LPR 32);
(c) 36,867 rows, so that 4,099 waves take a second row, F = 12 and 70;
(d) bitwise repeatability of (a) at F = 128, 150 and of (c) at F = 70.

Accuracy rule, the project's: ``|kernel - fp64| <= test_gat_kernels.bound(ref64, ref32)`` with
``ref32`` the same contract in fp32 on the CPU; ``vmax`` / ``vmin`` / ``amax`` / ``amin`` and
the segment-extreme outputs must EQUAL the contract's; ``lse`` is compared on the non-empty
rows (the empty ones must hold 0 and ``-inf``); the bf16 max / min backward by
``test_segment_max_gpu._tol``. The backward kernels are given the forward kernel's own
outputs. Output buffers are pre-filled with a sentinel that must not survive. Largest
``error / bound`` seen on an MI355X (a record, not an input to the bound; every figure is
printed before it is asserted):

    (a) softmax        out 0.127   lse 0.011   dx 0.147   dt 0.029
                       out of the single-source rows 0.039
        100 + randn    out 0.063   lse 0.002   dx 0.161 (F = 29, t = +2)   dt 0.130
        PNA            mean 0.006   sdev 0.017   sdev of the single-source rows 0.000
                       dx 0.003   g_std alone 0.001   beta = 1 0.003
        1000 + 0.1 randn   mean 0.002   sdev 0.000
        max / min      fp32 dx 0.011
    (b) two sources    softmax out 0.049   lse 0.029   PNA mean 0.003   sdev 0.008
    (c) many rows      softmax out 0.007   lse 0.004   dx 0.023   dt 0.005
                       PNA mean 0.004   sdev 0.008   dx 0.126   max / min dx 0.004
        second source  softmax out 0.010   lse 0.005   PNA mean 0.004   sdev 0.010

The whole file takes 12 s there. Shown to bite on two arithmetic-only mutants of the kernels:
resetting the softmax backward's per-lane ``dt`` sum for every source row fails (c)'s ``dt``
alone (error 20 and 55 against bounds of 5e-3 and 7e-3) while tests/test_softmax_aggr_gpu.py
passes; skipping the PNA forward's single-entry tail loop at VEC 4 LPR 32 fails every
F = 128 case of (a) and (b) and nothing else here.
"""
from __future__ import annotations

import math

import pytest
import torch

from dgraph_amd.ops import kernels as K
from dgraph_amd.ops.csr import CSR
from test_gat_kernels import bound
from test_pna import ALL, EPS, values
from test_segment_cases import (BF16_F, FP32_F, MANY, MANY_F, NSRC, SINGLE_ROWS, SPLIT, WAVES,
                                extreme_bwd_case, extreme_case, ladder_csr, many_case,
                                many_rows_csr, many_union_case, pna_bwd_case, pna_case,
                                second_pattern, softmax_case, split_slots, transposed,
                                with_idx)
from test_segment_max_gpu import _tol

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.25e9  # what float output buffers hold before a call
ISENT = -(2 ** 30)  # no slot of these rows, nor -2 - slot
NINF = float("-inf")
IDX = [torch.int32, torch.int64]
RATIOS: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(RATIOS):
        print(f"\n[segment variants] largest error / bound, {k}: {RATIOS[k]:.3f}", end="")


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


def full(shape, dtype=torch.float32):
    return torch.full(shape, ISENT if dtype == torch.int32 else SENT, dtype=dtype, device=DEV)


def written(*arrays):
    for a in arrays:
        assert not bool((a == (ISENT if a.dtype == torch.int32 else SENT)).any())


def in_range(csr: CSR, nsrc: int):
    """The column ids are the caller's contract: checked here before anything is launched."""
    assert csr.nnz == int(csr.rowptr[-1]) and bool((csr.degree() >= 0).all())
    assert csr.nnz == 0 or (0 <= int(csr.col.min()) and int(csr.col.max()) < nsrc)
    return csr.to(DEV)


# ------------------------------------------------------------------------------ runners
def run_softmax(csr, tc, x, t, g):
    """Forward into sentinel-filled buffers, then the backward on the forward's own
    ``(out, lse)`` with sentinel-filled ``dx`` and partials. Everything on the GPU."""
    R, C, F = csr.num_rows, tc.num_rows, x.shape[1]
    out, lse = K.segment_softmax(csr.rowptr, csr.col, x, t, full((R, F)), full((R, F)))
    P = K._native.ops().segment_softmax_dt_parts(C)
    dx, part = K.segment_softmax_bwd(tc.rowptr, tc.col, x, t, g, out, lse, full((C, F)),
                                     dt_partials=full((P, F)))
    assert part.shape == (P, F) and P >= 1
    written(out, lse, dx, part)  # every row of the partials too
    return dict(out=out, lse=lse, dx=dx, part=part)


def check_softmax(tag, o, r64, r32, d64, d32, ne):
    within(tag, "out", o["out"], r64[0], r32[0])
    within(tag, "lse", o["lse"][ne.to(DEV)], r64[1][ne], r32[1][ne])
    e = (~ne).to(DEV)
    assert torch.count_nonzero(o["out"][e]) == 0 and bool((o["lse"][e] == NINF).all())
    within(tag, "dx", o["dx"], d64[0], d32[0])
    within(tag, "dt", o["part"].double().sum(0), d64[1], d32[1])


def pna_buffers(R, F):
    return dict(mean=full((R, F)), sdev=full((R, F)), vmax=full((R, F)),
                amax=full((R, F), torch.int32), vmin=full((R, F)),
                amin=full((R, F), torch.int32))


def run_pna(csr, tc, rel, x, g, which=ALL, acc=None):
    """Forward (all four pairs) into sentinel-filled buffers, then the backward for the
    aggregators ``which`` on the forward's own outputs (``acc``: with ``beta = 1`` into
    it)."""
    R, C, F = csr.num_rows, tc.num_rows, x.shape[1]
    o = pna_buffers(R, F)
    K.segment_pna(csr.rowptr, csr.col, x, **o)
    written(*o.values())
    kw = dict(g_mean=g.get("mean") if "mean" in which else None,
              g_std=g.get("std") if "std" in which else None, mean=o["mean"], sdev=o["sdev"],
              g_max=g.get("max") if "max" in which else None, amax=o["amax"],
              g_min=g.get("min") if "min" in which else None, amin=o["amin"])
    inv = csr.inv_degree()
    if acc is None:
        o["dx"] = K.segment_pna_bwd(tc.rowptr, tc.col, rel, x, inv, full((C, F)), **kw)
    else:
        o["dx"] = K.segment_pna_bwd(tc.rowptr, tc.col, rel, x, inv, acc, beta=1.0, **kw)
    written(o["dx"])
    return o


def check_pna_fwd(tag, o, r64, r32):
    for a in ("max", "min"):
        assert torch.equal(o["v" + a].cpu().double(), r64[a]), f"{tag} v{a}"
        assert torch.equal(o["a" + a].cpu(), r64["a" + a]), f"{tag} a{a}"
    within(tag, "mean", o["mean"], r64["mean"], r32["mean"])
    within(tag, "sdev", o["sdev"], r64["std"], r32["std"])


def run_extreme(csr, tc, rel, x, g, minimum):
    R, C, F = csr.num_rows, tc.num_rows, x.shape[1]
    out, arg = K.segment_extreme(csr.rowptr, csr.col, x, full((R, F), x.dtype),
                                 full((R, F), torch.int32), minimum=minimum)
    dx = K.segment_extreme_bwd(tc.rowptr, tc.col, rel, g, arg, full((C, F), g.dtype))
    written(out, arg, dx)
    return dict(out=out, arg=arg, dx=dx)


def ladder_on_device(idx):
    csr = ladder_csr(idx)
    tc, rel = transposed(csr, idx)
    assert tc.col.dtype == idx and csr.col.dtype == idx
    return in_range(csr, NSRC), in_range(tc, csr.num_rows), rel.to(DEV)


LADDER_NE = ladder_csr().degree() > 0
SINGLE = list(SINGLE_ROWS)


def dev(d):
    return {k: v.to(DEV) for k, v in d.items()}


# ------------------------------------------------------------------- (a) the ladder
def ladder_softmax(F, idx, xkind="plain", tscale=None):
    c = softmax_case(F, xkind, tscale)
    csr, tc, _ = ladder_on_device(idx)
    return c, run_softmax(csr, tc, c["x"].to(DEV), c["t"].to(DEV), c["g"].to(DEV))


@pytest.mark.parametrize("F", FP32_F)
@pytest.mark.parametrize("idx", IDX)
def test_ladder_softmax(F, idx):
    c, o = ladder_softmax(F, idx)
    t = c["t"]
    assert bool((t == 0).any()) and bool((t < 0).any()) and bool((t > 0).any())
    check_softmax(f"softmax[F={F}]", o, c["r64"], c["r32"], c["d64"], c["d32"], LADDER_NE)
    col = ladder_csr().col
    src = c["x"][col[ladder_csr().rowptr[SINGLE]]]  # the one source each of these rows repeats
    within(f"softmax[F={F}]", "out of the single-source rows", o["out"][SINGLE], src.double(),
           c["r32"][0][SINGLE])


@pytest.mark.parametrize("F", [128, 29])
@pytest.mark.parametrize("tscale", [2.0, -2.0])
def test_ladder_softmax_offset(F, tscale):
    """``x = 100 + randn`` at ``t = +-2``: ``exp(+-200)`` is out of fp32's range."""
    c, o = ladder_softmax(F, torch.int32, "offset", tscale)
    check_softmax(f"softmax offset[F={F},t={tscale:+.0f}]", o, c["r64"], c["r32"], c["d64"],
                  c["d32"], LADDER_NE)


def ladder_pna(F, idx, which=ALL, beta1=False):
    c = pna_case(F)
    csr, tc, rel = ladder_on_device(idx)
    acc = values("plain", NSRC, F, 77).to(DEV) if beta1 else None  # dx's old contents
    return c, run_pna(csr, tc, rel, c["x"].to(DEV), dev(c["g"]), which, acc)


@pytest.mark.parametrize("F", FP32_F)
@pytest.mark.parametrize("idx", IDX)
def test_ladder_pna(F, idx):
    c, o = ladder_pna(F, idx)
    tag = f"pna[F={F}]"
    check_pna_fwd(tag, o, c["r64"], c["r32"])
    assert bool((o["amax"][SINGLE] == 0).all()) and bool((o["amin"][SINGLE] == 0).all())
    root = torch.full((len(SINGLE), F), math.sqrt(EPS), dtype=torch.float64)
    within(tag, "sdev of the single-source rows", o["sdev"][SINGLE], root, c["r32"]["std"][SINGLE])
    assert torch.equal(o["sdev"][0].cpu(), torch.full((F,), EPS).sqrt())  # the empty row
    assert bool((o["amax"][0] == -1).all()) and bool((o["amin"][0] == -1).all())
    d64, d32 = pna_bwd_case(F)
    within(tag, "dx", o["dx"], d64, d32)


@pytest.mark.parametrize("F", [8, 128, 150])
@pytest.mark.parametrize("idx", IDX)
def test_ladder_pna_backward_std_alone(F, idx):
    c, o = ladder_pna(F, idx, ("std",))
    d64, d32 = pna_bwd_case(F, ("std",))
    within(f"pna std alone[F={F}]", "dx", o["dx"], d64, d32)


@pytest.mark.parametrize("F", [128, 150])
@pytest.mark.parametrize("idx", IDX)
def test_ladder_pna_backward_beta_one(F, idx):
    c, o = ladder_pna(F, idx, beta1=True)
    d64, d32 = pna_bwd_case(F)
    old = values("plain", NSRC, F, 77)
    within(f"pna beta = 1[F={F}]", "dx", o["dx"], d64 + old.double(), d32 + old)


@pytest.mark.parametrize("F", [128, 29])
def test_ladder_pna_offset(F):
    """``x = 1000 + 0.1 randn`` (forward): the pivot and its re-centring carry the variance."""
    c = pna_case(F, "offset")
    csr, _, _ = ladder_on_device(torch.int32)
    o = pna_buffers(csr.num_rows, F)
    K.segment_pna(csr.rowptr, csr.col, c["x"].to(DEV), **o)
    written(*o.values())
    check_pna_fwd(f"pna offset[F={F}]", o, c["r64"], c["r32"])


def ladder_extreme(F, dtype, idx, minimum):
    c = extreme_case(F, dtype)
    csr, tc, rel = ladder_on_device(idx)
    return c, run_extreme(csr, tc, rel, c["x"].to(DEV), c["g"].to(DEV), minimum)


def check_extreme(tag, F, dtype, minimum, c, o):
    name = "min" if minimum else "max"
    assert o["out"].dtype == dtype and o["arg"].dtype == torch.int32
    assert torch.equal(o["arg"].cpu(), c["ref"]["a" + name]), tag
    assert torch.equal(o["out"].cpu().double(), c["ref"][name]), tag  # bf16: exact widening
    assert bool((o["arg"][SINGLE] == 0).all()) and bool((o["arg"][0] == -1).all())
    d64, d32 = extreme_bwd_case(F, dtype, minimum)
    if dtype == torch.float32:
        within(tag, "dx", o["dx"], d64, d32)
    else:
        assert o["dx"].dtype == dtype
        torch.testing.assert_close(o["dx"].cpu().double(), d64, **_tol(dtype))


@pytest.mark.parametrize("F", FP32_F)
@pytest.mark.parametrize("idx", IDX)
@pytest.mark.parametrize("minimum", [False, True])
def test_ladder_extreme_fp32(F, idx, minimum):
    c, o = ladder_extreme(F, torch.float32, idx, minimum)
    check_extreme(f"extreme fp32[F={F}]", F, torch.float32, minimum, c, o)


@pytest.mark.parametrize("F", BF16_F)
@pytest.mark.parametrize("idx", IDX)
@pytest.mark.parametrize("minimum", [False, True])
def test_ladder_extreme_bf16(F, idx, minimum):
    c, o = ladder_extreme(F, torch.bfloat16, idx, minimum)
    check_extreme(f"extreme bf16[F={F}]", F, torch.bfloat16, minimum, c, o)


# ------------------------------------------------------------------- (b) two sources
@pytest.mark.parametrize("F", [128, 29])
@pytest.mark.parametrize("idx", IDX)
def test_two_sources_on_the_ladder(F, idx):
    """Pass 1 over the sources below 130 (PNA: ``final=False``), pass 2 with ``second=True``
    over ALL rows: the contract on the unsplit ladder; rows without an entry in the second
    block are bitwise what pass 1 left (PNA's ``sdev``: what pass 1 leaves when it
    finalises)."""
    ladder = ladder_csr()
    a, b = ladder.split_columns(SPLIT)
    absent = b.degree() == 0
    assert int(absent.sum()) > 1 and bool((~absent).any()) and bool((a.degree() == 0)[1:].any())
    a, b = in_range(with_idx(a, idx), SPLIT), in_range(with_idx(b, idx), NSRC - SPLIT)
    absent = absent.to(DEV)
    R = ladder.num_rows
    tag = f"two sources[F={F}]"

    s = softmax_case(F)
    x, t = s["x"].to(DEV), s["t"].to(DEV)
    xa, xb = x[:SPLIT].contiguous(), x[SPLIT:].contiguous()
    out, lse = K.segment_softmax(a.rowptr, a.col, xa, t, full((R, F)), full((R, F)))
    o1, l1 = out.clone(), lse.clone()
    K.segment_softmax(b.rowptr, b.col, xb, t, out, lse, second=True)
    within(tag, "softmax out", out, s["r64"][0], s["r32"][0])
    ne = LADDER_NE
    within(tag, "softmax lse", lse[ne.to(DEV)], s["r64"][1][ne], s["r32"][1][ne])
    assert torch.count_nonzero(out[0]) == 0 and bool((lse[0] == NINF).all())
    assert torch.equal(out[absent], o1[absent]) and torch.equal(lse[absent], l1[absent])

    p = pna_case(F)
    assert torch.equal(p["x"], s["x"])
    want = {k: split_slots(ladder, p["r64"][k]) for k in ("amax", "amin")}
    o = pna_buffers(R, F)
    K.segment_pna(a.rowptr, a.col, xa, final=False, **o)
    first = {k: v.clone() for k, v in o.items()}
    K.segment_pna(b.rowptr, b.col, xb, second=True, final=True, prev_rowptr=a.rowptr, **o)
    written(*o.values())
    alone = pna_buffers(R, F)  # the first block by itself, finalised
    K.segment_pna(a.rowptr, a.col, xa, **alone)
    within(tag, "pna mean", o["mean"], p["r64"]["mean"], p["r32"]["mean"])
    within(tag, "pna sdev", o["sdev"], p["r64"]["std"], p["r32"]["std"])
    for name in ("max", "min"):
        assert torch.equal(o["v" + name].cpu().double(), p["r64"][name])
        assert torch.equal(o["a" + name].cpu(), want["a" + name])
    for k in ("mean", "vmax", "amax", "vmin", "amin"):
        assert torch.equal(o[k][absent], first[k][absent]), k
    assert torch.equal(o["sdev"][absent], alone["sdev"][absent])
    assert bool((o["amax"] >= 0).any()) and bool((o["amax"] <= -2).any())

    for minimum, name in ((False, "max"), (True, "min")):
        out, arg = K.segment_extreme(a.rowptr, a.col, xa, full((R, F)),
                                     full((R, F), torch.int32), minimum=minimum)
        o1, a1 = out.clone(), arg.clone()
        K.segment_extreme(b.rowptr, b.col, xb, out, arg, minimum=minimum, second=True)
        assert torch.equal(out.cpu().double(), p["r64"][name])
        assert torch.equal(arg.cpu(), want["a" + name])
        assert torch.equal(out[absent], o1[absent]) and torch.equal(arg[absent], a1[absent])


# ------------------------------------------------------------------- (c) two rows per wave
def many_on_device():
    csr = many_rows_csr(torch.int32)
    tc, rel = transposed(csr, torch.int32)
    parts = K._native.ops().segment_softmax_dt_parts(MANY)
    # the grid cap is what makes a wave take a second row: if it moves, this case must too
    assert parts == WAVES // 4 == 8192 < -(-MANY // 4)
    return in_range(csr, MANY), in_range(tc, MANY), rel.to(DEV)


def run_many(F):
    c = many_case(F)
    csr, tc, rel = many_on_device()
    x, t, g = c["x"].to(DEV), c["t"].to(DEV), dev(c["g"])
    res = dict(s=run_softmax(csr, tc, x, t, g["mean"]), p=run_pna(csr, tc, rel, x, g))
    for minimum, name in ((False, "max"), (True, "min")):
        res[name] = run_extreme(csr, tc, rel, x, g[name], minimum)
    return c, res


@pytest.mark.parametrize("F", MANY_F)
def test_second_row_of_a_wave(F):
    """36,867 rows and as many sources: forward and backward of the three families. The
    softmax ``dt`` partials (one row per workgroup, 8,192 of them, each lane's sum running
    over BOTH source rows of its wave) are the point."""
    c, res = run_many(F)
    tag = lambda fam: f"many rows {fam}[F={F}]"  # noqa: E731
    ne = many_rows_csr().degree() > 0
    s = res["s"]
    assert s["part"].shape == (8192, F)
    check_softmax(tag("softmax"), s, c["s64"], c["s32"], c["sd64"], c["sd32"], ne)
    check_pna_fwd(tag("pna"), res["p"], c["p64"], c["p32"])
    within(tag("pna"), "dx", res["p"]["dx"], c["pd64"], c["pd32"])
    for name in ("max", "min"):
        e = res[name]
        assert torch.equal(e["out"].cpu().double(), c["p64"][name])
        assert torch.equal(e["arg"].cpu(), c["p64"]["a" + name])
        within(tag("extreme"), "dx", e["dx"], c[name + "d64"], c[name + "d32"])


@pytest.mark.parametrize("F", MANY_F)
def test_second_source_over_many_rows(F):
    """A second-source pass over all 36,867 rows whose pattern is empty on every odd row:
    those stay bitwise, the even ones match the contract over both blocks' entries."""
    c, u = many_case(F), many_union_case(F)
    csr, _, _ = many_on_device()
    p2 = in_range(second_pattern(), MANY)
    x, t = c["x"].to(DEV), c["t"].to(DEV)
    tag = f"many rows second source[F={F}]"
    odd = slice(1, None, 2)
    ne = (many_rows_csr().degree() + second_pattern().degree()) > 0

    out, lse = K.segment_softmax(csr.rowptr, csr.col, x, t, full((MANY, F)), full((MANY, F)))
    o1, l1 = out.clone(), lse.clone()
    K.segment_softmax(p2.rowptr, p2.col, x, t, out, lse, second=True)
    assert torch.equal(out[odd], o1[odd]) and torch.equal(lse[odd], l1[odd])
    within(tag, "softmax out", out, u["s64"][0], u["s32"][0])
    within(tag, "softmax lse", lse[ne.to(DEV)], u["s64"][1][ne], u["s32"][1][ne])

    o = pna_buffers(MANY, F)
    K.segment_pna(csr.rowptr, csr.col, x, final=False, **o)
    first = {k: v.clone() for k, v in o.items()}
    K.segment_pna(p2.rowptr, p2.col, x, second=True, final=True, prev_rowptr=csr.rowptr, **o)
    alone = pna_buffers(MANY, F)
    K.segment_pna(csr.rowptr, csr.col, x, **alone)
    for k in ("mean", "vmax", "amax", "vmin", "amin"):
        assert torch.equal(o[k][odd], first[k][odd]), k
    assert torch.equal(o["sdev"][odd], alone["sdev"][odd])
    within(tag, "pna mean", o["mean"], u["p64"]["mean"], u["p32"]["mean"])
    within(tag, "pna sdev", o["sdev"], u["p64"]["std"], u["p32"]["std"])
    # the extremes: the first block's winner unless the second's is strictly better
    want = {}
    for name, better in (("max", torch.gt), ("min", torch.lt)):
        v1, a1 = c["p64"][name], c["p64"]["a" + name]
        v2, a2 = u["second"][name], u["second"]["a" + name]
        win = (a2 >= 0) & ((a1 == -1) | better(v2, v1))
        want[name] = (torch.where(win, v2, v1), torch.where(win, -2 - a2, a1))
        assert torch.equal(want[name][0], u["p64"][name])
        assert torch.equal(o["v" + name].cpu().double(), want[name][0])
        assert torch.equal(o["a" + name].cpu(), want[name][1])
    for minimum, name in ((False, "max"), (True, "min")):
        out, arg = K.segment_extreme(csr.rowptr, csr.col, x, full((MANY, F)),
                                     full((MANY, F), torch.int32), minimum=minimum)
        o1, a1 = out.clone(), arg.clone()
        K.segment_extreme(p2.rowptr, p2.col, x, out, arg, minimum=minimum, second=True)
        assert torch.equal(out[odd], o1[odd]) and torch.equal(arg[odd], a1[odd])
        assert torch.equal(out.cpu().double(), want[name][0])
        assert torch.equal(arg.cpu(), want[name][1])


# ------------------------------------------------------------------- (d) repeatability
def _flat(res):
    return [v for k in sorted(res) for v in (_flat(res[k]) if isinstance(res[k], dict)
                                             else [res[k]])]


@pytest.mark.parametrize("F", [128, 150])
def test_ladder_is_bitwise_repeatable(F):
    runs = []
    for _ in range(2):
        res = dict(s=ladder_softmax(F, torch.int32)[1], p=ladder_pna(F, torch.int32)[1],
                   pb=ladder_pna(F, torch.int32, beta1=True)[1],
                   e=ladder_extreme(F, torch.float32, torch.int32, False)[1])
        runs.append(_flat(res))
    assert len(runs[0]) == len(runs[1]) > 10
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_many_rows_are_bitwise_repeatable():
    runs = [_flat(run_many(70)[1]) for _ in range(2)]
    assert len(runs[0]) == len(runs[1]) > 10
    for a, b in zip(*runs):
        assert torch.equal(a, b)
