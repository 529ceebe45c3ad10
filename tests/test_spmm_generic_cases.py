"""Inputs, oracles and case table of tests/test_spmm_generic_variants_gpu.py, which runs the
five kernels of csrc/kernels/spmm.hip (generic CSR SpMM in two data flows, the bf16
row-group kernel, the two hub-split kernels) at every compiled instantiation, and the CPU
tests that pin all of it down first.

* Patterns: :func:`test_segment_cases.ladder_csr` (142 rows, 257 sources: degrees 0..136,
  a 1,027-entry row, four rows that repeat one source) and
  :func:`test_segment_cases.many_rows_csr` (36,867 rows of degree ``r % 4``) for everything
  that depends on the row-to-wave mapping.
* Calls (:func:`make_call`) are dicts of CPU tensors; :func:`formula` writes the definition
  of ``K.spmm`` out once more in a given precision (``absolute``: over |terms|).
* Exact comparison (:func:`assert_exact`): values from the dyadic alphabets of
  test_spmm_f32_variants_gpu.py, small integers (exact in bf16 too), so every fp32 product
  and partial sum in any order is exact: an fp32 output equals fp64 bitwise, a bf16 output
  equals ``ref64.float().bfloat16()`` (one round-to-nearest-even). The hub path of a bf16
  output rounds twice (the main pass stores bf16, the reduce reads it back and stores
  again): :func:`split_expect` rounds at the same two places. The precondition
  (:func:`exact_ok`) is asserted on the reference alone.
* Full mantissa (:func:`allowance`): unit-normal inputs; fp32 under
  ``test_gat_kernels.bound``; a bf16 output adds ``2^-8 |v|`` per element (half a bf16
  ulp, 8 significant bits, is at most that) once per rounding, ``v`` being the fp64 value
  that rounding sees: the final result, and on the hub path also the capped main pass,
  which is what the first store rounds.
* :data:`TABLE`: every GPU case with its kernel configuration, and :func:`reach`, the
  launchers' rules restated by hand (``launch_vec``, ``launch_lpr``, ``launch_rowgroup``,
  ``spmm_hub_partials``' vector choice, the ``XCD`` and pass conditions of ``spmm_csr``),
  which shows that the table reaches all 50 + 100 + 80 + 10 + 2 = 242 instantiations. It
  must be updated with the launchers; it checks the table, not what a kernel selected.

Ids at or above 2^31 are out of scope: the row-group kernel narrows int64 ids to 32 bits
by design.

Largest ``error / allowance`` of the CPU path on the full-mantissa cases, against fp64 (a
record; printed by ``test_cpu_path_meets_the_rule``): generic fp32 0.055, generic bf16
0.977, hub partials 0.036, split path fp32 0.013, split path bf16 0.961 (bf16: the CPU path
rounds once more than fp64 does, and half an ulp of a value just above a power of two is
2^-8 of it).
"""
from __future__ import annotations

import functools
from collections import namedtuple

import pytest
import torch

from dgraph_amd.ops import kernels as K
from dgraph_amd.ops import reference as R
from dgraph_amd.ops.csr import CSR
from test_gat_kernels import bound
from test_segment_cases import MANY, NSRC, ladder_csr, many_rows_csr, with_idx
from test_spmm_f32_variants_gpu import ALPHABETS, _seed, frac_bits, gen, ints, pick

# the sentinel of memory a call must not write: test_spmm_f32_variants_gpu.SENT rounded to
# bf16, so that one value serves both element types
SENT = float(torch.tensor(-12345.0).bfloat16())
HUB_ROW = 137
BF16_ULP = 2.0 ** -8  # per rounding, times |reference| (see the module docstring)

CallSpec = namedtuple("CallSpec", "pat F fam heads epi cap")
CallSpec.__new__.__defaults__ = (1, False, 0)
# view: None, or (element offset, row stride) of the column slices x and out are made as
RunSpec = namedtuple("RunSpec", "dt idx variant xcd pc rg32 view")
RunSpec.__new__.__defaults__ = (4, 0, 128, False, None)


# ------------------------------------------------------------------------------ patterns
def csr_of(pat: str) -> CSR:
    """``ladder``, ``ladderc`` (the ladder row-compacted: ``row_map`` skips row 0) or
    ``many``; int64 ids."""
    if pat == "many":
        return many_rows_csr(torch.int64)
    csr = ladder_csr(torch.int64)
    return csr.compact_rows() if pat == "ladderc" else csr


def nout_of(pat: str) -> int:
    return MANY if pat == "many" else 142


# ------------------------------------------------------------------------------ calls
def make_call(spec: CallSpec, normal: bool = False):
    """The call of one case: rowptr, col, x, out0 (the output buffer before the call),
    beta, heads, cap and the optional edge_weight / col_scale / row_scale / row_map.
    ``fam``: ``w0`` unweighted, ``w1`` edge weights, ``w2`` column scale, ``w3`` both.
    ``epi``: ``beta != 0`` on integer old contents plus ``row_scale``."""
    g = gen("generic", *spec, normal)
    csr = csr_of(spec.pat)
    nsrc, nout, E = csr.num_cols, nout_of(spec.pat), csr.nnz
    val = (lambda shape: torch.randn(shape, generator=g)) if normal else \
        (lambda shape: ints(shape, g))
    c = dict(rowptr=csr.rowptr, col=csr.col.long(), x=val((nsrc, spec.F)), beta=0.0,
             out0=torch.full((nout, spec.F), SENT), heads=spec.heads, cap=spec.cap,
             row_map=csr.row_map)
    wmode = int(spec.fam[1])
    if wmode & 1:
        shape = (E, spec.heads) if spec.heads > 1 else (E,)
        c["edge_weight"] = torch.rand(shape, generator=g) if normal else \
            pick(ALPHABETS["ew"], shape, g)
    if wmode & 2:
        c["col_scale"] = torch.rand(nsrc, generator=g) + 0.5 if normal else \
            pick(ALPHABETS["scale"], (nsrc,), g)
    if spec.epi:
        c["out0"] = val((nout, spec.F))
        c["beta"] = ALPHABETS["beta"][_seed(*spec) % 3]
        c["row_scale"] = torch.rand(nout, generator=g) + 0.5 if normal else \
            pick(ALPHABETS["scale"], (nout,), g)
    return c


def as_bf16(c):
    """The call with x and out0 rounded to bf16 (what a bf16 kernel is handed)."""
    return dict(c, x=c["x"].bfloat16().float(), out0=c["out0"].bfloat16().float())


def formula(c, dtype=torch.float64, absolute: bool = False) -> torch.Tensor:
    """``out[m(r)] = row_scale[m(r)] * sum_{k < cap} ew[j, head(f)] col_scale[c_j] x[c_j, f]
    + beta * out[m(r)]`` over the entries ``j = rowptr[r] + k`` of every CSR row ``r``, with
    ``m = row_map`` (identity without one); rows no CSR row maps to keep their contents.
    The whole output buffer, in ``dtype``. ``absolute``: the same sum over |terms|, the
    row scale not below 1 (bounds the sums before and after it)."""
    a = (lambda t: t.abs()) if absolute else (lambda t: t)
    rp, col = c["rowptr"], c["col"].long()
    n = rp.numel() - 1
    E, F = col.numel(), c["x"].shape[1]
    H = max(int(c.get("heads", 1)), 1)
    out = a(c["out0"]).to(dtype).clone()
    if n <= 0:
        return out
    deg = rp[1:] - rp[:-1]
    rows = torch.repeat_interleave(torch.arange(n), deg)
    w = torch.ones(E, H, dtype=dtype)
    if c.get("edge_weight") is not None:
        w = w * a(c["edge_weight"]).to(dtype).reshape(E, H)
    if c.get("col_scale") is not None:
        w = w * a(c["col_scale"]).to(dtype)[col].unsqueeze(1)
    terms = (a(c["x"]).to(dtype)[col].reshape(E, H, F // H) * w.unsqueeze(2)).reshape(E, F)
    cap = int(c.get("cap", 0))
    if cap > 0:
        keep = torch.arange(E) - rp[:-1][rows] < cap
        rows, terms = rows[keep], terms[keep]
    acc = torch.zeros(n, F, dtype=dtype).index_add_(0, rows, terms)
    m = c["row_map"] if c.get("row_map") is not None else torch.arange(n)
    if c.get("row_scale") is not None:
        rs = a(c["row_scale"]).to(dtype)[m]
        acc = acc * (rs.clamp_min(1.0) if absolute else rs).unsqueeze(1)
    beta = abs(c["beta"]) if absolute else c["beta"]
    if beta != 0.0:
        acc = acc + beta * out[m]
    out[m] = acc
    return out


def exact_ok(c, ref64: torch.Tensor) -> None:
    """What makes a bitwise comparison legitimate, asserted on the reference alone: the
    result is an fp32 number, the operands are bf16 numbers, and the sum of |terms| of
    every output element, in units of the smallest fraction in use, stays below 2^24."""
    assert torch.equal(ref64, ref64.float().double()), "reference is not exact in fp32"
    for k in ("x", "out0"):
        assert torch.equal(c[k], c[k].bfloat16().float()), k
    peak = float(formula(c, absolute=True).abs().max()) if ref64.numel() else 0.0
    assert peak * 2 ** frac_bits(c) < 2 ** 24, (peak, frac_bits(c))


def expect(ref64: torch.Tensor, dt: str) -> torch.Tensor:
    """The output an exact case must produce, as fp64: fp32 the reference itself, bf16 one
    round-to-nearest-even of it."""
    return ref64 if dt == "f32" else ref64.float().bfloat16().double()


def assert_same(got: torch.Tensor, want64: torch.Tensor) -> None:
    g64 = got.double().cpu()
    assert g64.shape == want64.shape, (g64.shape, want64.shape)
    if not torch.equal(g64, want64):
        bad = torch.nonzero((g64 != want64) | (g64.isnan() != want64.isnan()))
        at = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{bad.shape[0]} elements differ; first at {at}: "
                             f"got {float(g64[at])}, expected {float(want64[at])}")


def assert_exact(got: torch.Tensor, c, dt: str, ref64: torch.Tensor | None = None,
                 checked: bool = False) -> None:
    """``got`` (the whole output buffer) equals the fp64 reference bitwise (bf16: after
    one rounding). ``checked``: the caller has run :func:`exact_ok` on this call."""
    ref64 = formula(c) if ref64 is None else ref64
    if not checked:
        exact_ok(c, ref64)
    assert_same(got, expect(ref64, dt))


def allowance(ref64, ref32, dt: str, rounded=()) -> torch.Tensor:
    """Per-element limit of ``|got - fp64|`` of a full-mantissa case: ``bound(ref64,
    ref32)``; a bf16 output adds ``2^-8 |v|`` for the fp64 value ``v`` each of its roundings
    sees: the final result, and every tensor of ``rounded`` (the hub path's main pass)."""
    lim = torch.full_like(ref64, bound(ref64, ref32))
    if dt == "bf16":
        for v in (ref64,) + tuple(rounded):
            lim = lim + BF16_ULP * v.abs()
    return lim


def assert_bound(got, ref64, ref32, dt: str, rounded=(), label="spmm") -> float:
    err = (got.double().cpu() - ref64).abs()
    lim = allowance(ref64, ref32, dt, rounded)
    ratio = float((err / lim).max()) if err.numel() else 0.0
    print(f"{label} [{dt}] err {float(err.max()):.3e} bound {bound(ref64, ref32):.3e} "
          f"allowance {float(lim.max()):.3e} error / allowance {ratio:.3f}")
    assert bool((err <= lim).all()), (label, dt, ratio)
    return ratio


# ------------------------------------------------------------------ the hub split path
def split_parts(c, cap: int, dtype=torch.float64):
    """(main pass, hub tails) of the split path written out: the capped call, and per
    output row ``row_scale * sum`` of the entries past ``cap`` (zero for rows within it)."""
    main = formula(dict(c, cap=cap), dtype)
    rest = dict(c, beta=0.0, out0=torch.zeros_like(c["out0"]))
    tail = formula(rest, dtype) - formula(dict(rest, cap=cap), dtype)
    return main, tail


def split_expect(c, cap: int, dt: str) -> torch.Tensor:
    """The output of ``K.spmm(split=hub_split(cap))`` on an exact call, as fp64: the main
    pass stores its rounded result, the reduce adds the tails of the hub rows to what it
    reads back and stores again; every other row is stored once."""
    main, tail = split_parts(c, cap)
    main = expect(main, dt)
    rp = c["rowptr"]
    m = c["row_map"] if c.get("row_map") is not None else torch.arange(rp.numel() - 1)
    hub = m[(rp[1:] - rp[:-1]) > cap]
    out = main.clone()
    out[hub] = expect(main[hub] + tail[hub], dt)
    return out


SEG_LENS = (1, 3, 4, 5, 63, 64, 65, 129, 1027)


def hub_segments():
    """Hand-made segments of the ladder's entry array, one per length of
    :data:`SEG_LENS`: the whole 1,027-entry row, and ranges that start two entries into
    the row of that degree (so they cross a row boundary: any range is a segment)."""
    rp = ladder_csr().rowptr
    beg = torch.tensor([int(rp[HUB_ROW]) if n == 1027 else int(rp[n]) + 2 for n in SEG_LENS])
    return beg, beg + torch.tensor(SEG_LENS)


def partials_formula(beg, end, col, x, ew=None, cs=None, dtype=torch.float64):
    """``part[i] = sum_{j in [beg[i], end[i])} ew[j] cs[col[j]] x[col[j]]``, a segment at a
    time."""
    out = torch.zeros(beg.numel(), x.shape[1], dtype=dtype)
    for i, (b, e) in enumerate(zip(beg.tolist(), end.tolist())):
        cc = col[b:e].long()
        w = torch.ones(e - b, dtype=dtype)
        if ew is not None:
            w = w * ew[b:e].to(dtype)
        if cs is not None:
            w = w * cs[cc].to(dtype)
        out[i] = (x[cc].to(dtype) * w.unsqueeze(1)).sum(0)
    return out


def make_hub_call(F: int, fam: str, normal: bool = False):
    g = gen("hub", F, fam, normal)
    csr = ladder_csr()
    beg, end = hub_segments()
    c = dict(beg=beg, end=end, col=csr.col.long(),
             x=torch.randn(NSRC, F, generator=g) if normal else ints((NSRC, F), g))
    wmode = int(fam[1])
    if wmode & 1:
        c["ew"] = torch.rand(csr.nnz, generator=g) if normal else \
            pick(ALPHABETS["ew"], (csr.nnz,), g)
    if wmode & 2:
        c["cs"] = torch.rand(NSRC, generator=g) + 0.5 if normal else \
            pick(ALPHABETS["scale"], (NSRC,), g)
    return c


def hub_oracle(c, dtype=torch.float64, absolute=False):
    a = (lambda t: None if t is None else t.abs()) if absolute else (lambda t: t)
    return partials_formula(c["beg"], c["end"], c["col"], a(c["x"]), a(c.get("ew")),
                            a(c.get("cs")), dtype)


def hub_exact_ok(c, ref64) -> None:
    assert torch.equal(ref64, ref64.float().double())
    assert torch.equal(c["x"], c["x"].bfloat16().float())
    bits = (1 if c.get("ew") is not None else 0) + (2 if c.get("cs") is not None else 0)
    assert float(hub_oracle(c, absolute=True).max()) * 2 ** bits < 2 ** 24


REDUCE_SEG_PTR = (0, 1, 4, 9)  # hubs of 1, 3 and 5 segments
REDUCE_ROWS = (7, 2, 11)
REDUCE_NOUT = 14


def make_reduce_call(F: int, scaled: bool, normal: bool = False):
    g = gen("reduce", F, scaled, normal)
    val = (lambda shape: torch.randn(shape, generator=g)) if normal else \
        (lambda shape: ints(shape, g, -64, 64))
    c = dict(part=val((REDUCE_SEG_PTR[-1], F)), seg_ptr=torch.tensor(REDUCE_SEG_PTR),
             rows=torch.tensor(REDUCE_ROWS), out0=val((REDUCE_NOUT, F)))
    if scaled:
        c["rs"] = torch.rand(REDUCE_NOUT, generator=g) + 0.5 if normal else \
            pick(ALPHABETS["scale"], (REDUCE_NOUT,), g)
    return c


def reduce_formula(c, dtype=torch.float64, part=None):
    """``out[rows[h]] += rs[rows[h]] * sum`` of the hub's partial rows."""
    out = c["out0"].to(dtype).clone()
    part = c["part"] if part is None else part
    for h, r in enumerate(c["rows"].tolist()):
        acc = part[int(c["seg_ptr"][h]):int(c["seg_ptr"][h + 1])].to(dtype).sum(0)
        if c.get("rs") is not None:
            acc = acc * c["rs"][r].to(dtype)
        out[r] = out[r] + acc
    return out


# ------------------------------------------------------- the launchers' rules, restated
ELEM = {"f32": 4, "bf16": 2}
GRID_CAP = 256 * 32  # cap_blocks of launch_lpr, in 4-wave blocks


def launch_vec(dt, F, xoff, ldx, ooff, ldo, heads=1, head_dim=None):
    """spmm.hip ``launch_vec``: the widest of {16 / sizeof(T), 4, 1} that divides the row,
    both leading dimensions, the head size and both base pointers (a fresh allocation is
    at least 16-byte aligned, so a pointer's alignment is its element offset's)."""
    head_dim = head_dim or F
    for v in (16 // ELEM[dt], 4):
        if (F % v == 0 and ldx % v == 0 and ldo % v == 0 and xoff % v == 0 and ooff % v == 0
                and (heads <= 1 or head_dim % v == 0)):
            return v
    return 1


def lpr_of(lanes: int) -> int:
    return next((p for p in (4, 8, 16, 32) if lanes <= p), 64)


def generic_blocks(nrows: int, xcd: int):
    """``(blocks, XCD)`` of ``launch_lpr``."""
    blocks = max(1, min((nrows + 3) // 4, GRID_CAP))
    if xcd == 3:
        blocks = (nrows + 3) // 4
    on = xcd in (1, 2) and blocks >= 64
    if on:
        blocks = blocks // 8 * 8
        if xcd == 2:
            blocks = 8 * (((nrows + 7) // 8 + 3) // 4)
    return blocks, on


def launch_lpr(dt, idx, vec, F, nrows, variant, xcd):
    lpr = lpr_of(-(-F // vec))
    if variant >= 2:
        return ("v2", dt, idx, vec, lpr, generic_blocks(nrows, xcd)[1])
    return ("v1", dt, idx, vec, lpr)


def rowgroup_blocks(nrows: int, lpr: int, xcd: int):
    """``(blocks, XCD)`` of ``launch_rowgroup``: XCD needs 64 blocks of four row GROUPS."""
    ngroups = -(-nrows // (64 // lpr))
    blocks = (ngroups + 3) // 4
    on = xcd in (1, 2) and blocks >= 64
    return (8 * (((ngroups + 7) // 8 + 3) // 4) if on else blocks), on


def rowgroup_passes(F: int, pc: int):
    """The (first column, width) passes of the bf16 row-group path of ``spmm_csr``."""
    pc = pc if pc > 0 else 512
    pc = 512 if pc > 512 else (8 if pc < 8 else pc - pc % 8)
    return [(c0, min(pc, F - c0)) for c0 in range(0, F, pc)]


def reach(spec: CallSpec, run: RunSpec):
    """The kernel instantiations ``spmm_csr`` launches for the case, by the rules of
    spmm.hip restated (``("f32rg",)``: the fp32 row-group kernel of spmm_f32.hip)."""
    F, heads = spec.F, spec.heads
    nrows = csr_of(spec.pat).num_rows
    off, ld = run.view if run.view else (0, F)
    wmode = int(spec.fam[1])
    if run.dt == "f32":
        if run.rg32 and heads <= 1 and F % 4 == 0 and ld % 4 == 0 and off % 4 == 0:
            return [("f32rg",)]
        vec = launch_vec("f32", F, off, ld, off, ld, heads, F // heads)
        return [launch_lpr("f32", run.idx, vec, F, nrows, run.variant, run.xcd)]
    if run.variant == 4 and heads <= 1 and F % 8 == 0 and ld % 8 == 0 and off % 8 == 0:
        return [("rg", run.idx, lpr_of(-(-w // 8)), wmode,
                 rowgroup_blocks(nrows, lpr_of(-(-w // 8)), run.xcd)[1])
                for _, w in rowgroup_passes(F, run.pc)]
    pc = run.pc
    if heads == 1 and pc > 0 and F > pc and F % pc == 0:
        return [launch_lpr("bf16", run.idx, launch_vec("bf16", pc, off + c0, ld, off + c0, ld),
                           pc, nrows, run.variant, run.xcd) for c0 in range(0, F, pc)]
    vec = launch_vec("bf16", F, off, ld, off, ld, heads, F // heads)
    return [launch_lpr("bf16", run.idx, vec, F, nrows, run.variant, run.xcd)]


def hub_vec(dt, F, xoff, ldx):
    """``spmm_hub_partials``: bf16 4 / 2 / 1, fp32 2 / 1 -- the widest that divides the row
    width and stride and matches the base pointer."""
    for v in ((4, 2) if dt == "bf16" else (2,)):
        if F % v == 0 and ldx % v == 0 and xoff % v == 0:
            return v
    return 1


# ------------------------------------------------------------------------------ the table
IDX = ("i32", "i64")
FAMS = ("w0", "w1", "w2", "w3")
# (element type, VEC) -> one width per lane-group width 4 / 8 / 16 / 32 / 64 and one that
# needs the column loop
GENERIC_F = {
    ("f32", 1): (3, 7, 13, 29, 47, 153), ("f32", 4): (12, 28, 60, 124, 172, 260),
    ("bf16", 1): (3, 7, 13, 29, 47, 153), ("bf16", 4): (12, 28, 60, 124, 172, 260),
    ("bf16", 8): (24, 56, 120, 248, 264, 520),
}
# (heads, head_dim): a multiple of VEC and head_dim = 3, which lowers VEC to 1
GENERIC_HEADS = {
    ("f32", 1): ((2, 3), (4, 3), (2, 7)), ("f32", 4): ((2, 12), (4, 20), (2, 132)),
    ("bf16", 1): ((2, 3), (4, 3), (2, 7)), ("bf16", 4): ((2, 12), (4, 20), (2, 132)),
    ("bf16", 8): ((2, 8), (4, 72), (2, 264)),
}
CAPS = (5, 64, 100)  # at / below / above the degrees 5, 64 and 100 of the ladder
RG_F = (8, 32, 40, 64, 72, 128, 136, 256, 264, 512)  # two per LPR 4 / 8 / 16 / 32 / 64
RG_CAPS = (64, 65, 100)
# the F = 64 operand as column slices: (element offset, row stride)
VIEWS = ((0, 72), (4, 76), (1, 73), (0, 67))
MANY_RG_F = (8, 40, 72, 136, 264)


def _generic_runs(dt, variants=(1, 2), **kw):
    return tuple(RunSpec(dt, idx, v, **kw) for v in variants for idx in IDX)


def _build_table():
    t = {}
    for (dt, vec), widths in GENERIC_F.items():
        runs = _generic_runs(dt)
        for F in widths:
            calls = [(CallSpec("ladder", F, fam, 1, epi), runs)
                     for fam in FAMS for epi in (False, True)]
            calls.append((CallSpec("ladderc", F, "w3", 1, True), runs))
            calls.append((CallSpec("ladderc", F, "w0"), runs))
            calls += [(CallSpec("ladder", F, "w1", 1, epi, cap), runs)
                      for cap in CAPS for epi in (False, True)]
            if dt == "bf16" and vec < 8:  # the default variant falls back to variant 2
                calls.append((CallSpec("ladder", F, "w3", 1, True), _generic_runs(dt, (4,))))
            t[f"generic-{dt}-vec{vec}-F{F}"] = calls
        calls = []
        for heads, hd in GENERIC_HEADS[(dt, vec)]:
            for fam, epi in (("w1", False), ("w1", True), ("w3", False), ("w3", True)):
                calls.append((CallSpec("ladder", heads * hd, fam, heads, epi), runs))
                # with the fp32 row-group kernel left on and the default variant: how
                # production reaches the generic kernels
                calls.append((CallSpec("ladder", heads * hd, fam, heads, epi),
                              _generic_runs(dt, (4,), rg32=True)))
            calls.append((CallSpec("ladderc", heads * hd, "w3", heads, True, 64), runs))
        t[f"generic-{dt}-vec{vec}-heads"] = calls
    for dt in ("f32", "bf16"):
        calls = []
        for view in VIEWS:
            runs = _generic_runs(dt, view=view)
            # left to the defaults, what their own row-group kernels refuse
            align = 8 if dt == "bf16" else 4
            if view[0] % align or view[1] % align:
                runs += _generic_runs(dt, (4,), view=view, rg32=True)
            calls += [(CallSpec("ladder", 64, "w3", 1, True), runs),
                      (CallSpec("ladder", 64, "w0"), runs)]
        t[f"generic-{dt}-views"] = calls
    # bf16, variant 2: column passes (F > pass_cols, F % pass_cols == 0)
    t["generic-bf16-passes"] = [
        (CallSpec("ladder", 256, "w3", 1, True), _generic_runs("bf16", (2,), pc=128)),
        (CallSpec("ladder", 120, "w2"), _generic_runs("bf16", (2,), pc=60)),
        (CallSpec("ladder", 141, "w1", 1, True), _generic_runs("bf16", (1, 2), pc=47)),
    ]
    # the row-to-wave mapping of the generic kernels: XCD = true at every (VEC, LPR), the
    # capped grids of xcd 0 / 1 (a second row per wave) and xcd 3
    for (dt, vec), widths in GENERIC_F.items():
        calls = []
        for i, F in enumerate(widths[:5]):
            for epi in (False, True):
                runs = tuple(RunSpec(dt, idx, 2, 1 + (i + j) % 2)
                             for j, idx in enumerate(IDX))
                if i in (0, 4):
                    runs += (RunSpec(dt, "i32", 2, 0), RunSpec(dt, "i64", 2, 3),
                             RunSpec(dt, "i64", 1, 0), RunSpec(dt, "i32", 1, 3))
                calls.append((CallSpec("many", F, "w3" if epi else "w0", 1, epi), runs))
        t[f"many-generic-{dt}-vec{vec}"] = calls
    # the bf16 row-group kernel: one pass per width (pass_cols 512)
    for F in RG_F:
        runs = tuple(RunSpec("bf16", idx, 4, 0, 512) for idx in IDX)
        calls = [(CallSpec("ladder", F, fam, 1, epi), runs)
                 for fam in FAMS for epi in (False, True)]
        calls += [(CallSpec("ladderc", F, "w3", 1, True), runs),
                  (CallSpec("ladderc", F, "w0"), runs)]
        calls += [(CallSpec("ladder", F, FAMS[i + 1], 1, epi, cap), runs)
                  for i, cap in enumerate(RG_CAPS) for epi in (False, True)]
        calls.append((CallSpec("ladder", F, "w3", 1, True),
                      tuple(RunSpec("bf16", idx, 4, 0, 512, view=(8, F + 24)) for idx in IDX)))
        t[f"rowgroup-F{F}"] = calls
    # pass splitting: a narrower tail pass, a pass width that is no multiple of 8 (100 runs
    # as 96), one below 8, and pass_cols = 0 (512) with an 8-wide tail
    t["rowgroup-passes"] = [
        (CallSpec("ladder", F, fam, 1, epi), tuple(RunSpec("bf16", idx, 4, 0, pc) for idx in IDX))
        for F, pc in ((200, 128), (200, 100), (24, 4), (520, 0))
        for fam, epi in (("w0", False), ("w3", True))]
    for F in MANY_RG_F:
        calls = []
        for fam in FAMS:
            for epi in (False, True):
                runs = tuple(RunSpec("bf16", idx, 4, 1 + (int(fam[1]) + j) % 2, 512)
                             for j, idx in enumerate(IDX))
                if fam == "w0":
                    runs += (RunSpec("bf16", "i32", 4, 0, 512), RunSpec("bf16", "i64", 4, 3, 512))
                calls.append((CallSpec("many", F, fam, 1, epi), runs))
        t[f"many-rowgroup-F{F}"] = calls
    return t


TABLE = _build_table()

# hub partials: (element type, F, (element offset, row stride) or None) -> VEC
HUB_CASES = {
    ("bf16", 40, None): 4, ("bf16", 260, None): 4, ("bf16", 6, None): 2,
    ("bf16", 130, None): 2, ("bf16", 47, None): 1, ("bf16", 153, None): 1,
    ("f32", 6, None): 2, ("f32", 130, None): 2, ("f32", 47, None): 1, ("f32", 153, None): 1,
    # column slices whose offset or stride lowers the width
    ("bf16", 40, (2, 48)): 2, ("bf16", 40, (1, 48)): 1, ("bf16", 40, (0, 43)): 1,
    ("bf16", 40, (4, 52)): 4, ("f32", 6, (1, 8)): 1, ("f32", 6, (0, 9)): 1,
    ("f32", 6, (2, 10)): 2,
}
SPLIT_CAPS = (16, 64, 70)
SPLIT_F = {"bf16": (40, 47), "f32": (64, 47)}


def split_specs(F: int):
    """The calls of the whole split path: weighted with ``row_scale`` + ``beta`` and
    unweighted with the plain epilogue, on the ladder and on the compacted ladder."""
    return tuple(CallSpec(pat, F, fam, 1, epi) for pat in ("ladder", "ladderc")
                 for fam, epi in (("w3", True), ("w0", False)))


EDGE_SOFTMAX_H = (1, 2, 3, 5, 16, 17, 33, 64)


@functools.lru_cache(maxsize=None)
def ladder_case(spec: CallSpec):
    """(call, fp64 reference) of a ladder case, its precondition asserted; shared by every
    run of the case. (Many-rows calls are large: made, used and dropped.)"""
    assert spec.pat != "many"
    c = make_call(spec)
    ref = formula(c)
    exact_ok(c, ref)
    return c, ref


def test_table_reaches_every_instantiation():
    reached = set()
    for group, calls in TABLE.items():
        for spec, runs in calls:
            assert spec.F % spec.heads == 0 and runs, (group, spec)
            for run in runs:
                keys = reach(spec, run)
                reached.update(keys)
                if group.startswith("generic"):  # the kernel the group's name says
                    want = "v1" if run.variant == 1 else "v2"
                    assert all(k[0] == want and k[1] == run.dt for k in keys), (group, run)
                if group.startswith("rowgroup") or group.startswith("many-rowgroup"):
                    assert all(k[0] == "rg" for k in keys), (group, spec, run)
                if group.startswith("many") and run.xcd in (1, 2):
                    assert all(k[-1] is True for k in keys), (group, spec, run)
    v1 = {("v1", dt, i, v, p) for (dt, v) in GENERIC_F for i in IDX for p in (4, 8, 16, 32, 64)}
    v2 = {("v2",) + k[1:] + (x,) for k in v1 for x in (False, True)}
    rg = {("rg", i, p, w, x) for i in IDX for p in (4, 8, 16, 32, 64) for w in range(4)
          for x in (False, True)}
    assert (len(v1), len(v2), len(rg)) == (50, 100, 80)
    assert reached - {("f32rg",)} == v1 | v2 | rg
    assert ("f32rg",) not in reached  # no case of this table runs another file's kernel
    hp = {(dt, i, hub_vec(dt, F, *(view or (0, F)))) for (dt, F, view) in HUB_CASES for i in IDX}
    for (dt, F, view), vec in HUB_CASES.items():
        assert hub_vec(dt, F, *(view or (0, F))) == vec, (dt, F, view)
    assert hp == {("bf16", i, v) for i in IDX for v in (4, 2, 1)} | \
        {("f32", i, v) for i in IDX for v in (2, 1)} and len(hp) == 10
    for dt, vec in (("bf16", 4), ("bf16", 2), ("bf16", 1), ("f32", 2), ("f32", 1)):
        # the F > 64 * VEC column loop of every hub kernel
        assert any(d == dt and v == vec and F > 64 * vec for (d, F, _), v in HUB_CASES.items())
    assert len(v1 | v2 | rg) + len(hp) + 2 == 242  # + hub_reduce<bf16 / fp32>


def test_xcd_cases_have_their_blocks():
    """Every case claimed to reach ``XCD = true`` has the 64 blocks it needs, and the capped
    grids of ``xcd`` 0 / 1 give some waves a second row."""
    n = MANY
    assert n == 36867 and n % 8 == 3 and n > 4 * GRID_CAP
    for group, calls in TABLE.items():
        for spec, runs in calls:
            for run in runs:
                for k in reach(spec, run):
                    nrows = csr_of(spec.pat).num_rows
                    if k[0] == "v2":
                        blocks, on = generic_blocks(nrows, run.xcd)
                        assert on == k[-1] and (not on or (blocks >= 64 and blocks % 8 == 0))
                    if k[0] == "rg":
                        blocks, on = rowgroup_blocks(nrows, k[2], run.xcd)
                        assert on == k[-1] and (not on or (blocks >= 64 and blocks % 8 == 0))
                        # one group per wave covers every group of every XCD's chunk
                        ngroups = -(-nrows // (64 // k[2]))
                        assert not on or blocks // 8 * 4 >= -(-ngroups // 8)
    assert generic_blocks(n, 0) == (GRID_CAP, False)  # 32,768 waves: 4,099 take two rows
    blocks, on = generic_blocks(n, 1)
    assert on and blocks == GRID_CAP and blocks // 8 * 4 < -(-n // 8)  # a second row per wave
    blocks, on = generic_blocks(n, 2)
    assert on and blocks // 8 * 4 >= -(-n // 8)
    assert generic_blocks(n, 3) == ((n + 3) // 4, False)
    assert generic_blocks(142, 2) == (36, False) and rowgroup_blocks(4032, 4, 2)[1] is False
    assert rowgroup_blocks(4033, 4, 2)[1] is True


def test_rules_on_known_shapes():
    assert launch_vec("bf16", 64, 0, 72, 0, 72) == 8 and launch_vec("bf16", 64, 4, 76, 4, 76) == 4
    assert launch_vec("bf16", 64, 1, 73, 1, 73) == 1 and launch_vec("bf16", 64, 0, 67, 0, 67) == 1
    assert launch_vec("f32", 64, 4, 76, 4, 76) == 4 and launch_vec("f32", 64, 1, 73, 1, 73) == 1
    assert launch_vec("f32", 12, 0, 12, 0, 12, 4, 3) == 1  # head_dim = 3 lowers VEC
    assert launch_vec("bf16", 16, 0, 16, 0, 16, 2, 8) == 8
    assert [lpr_of(n) for n in (1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65)] == \
        [4, 4, 8, 8, 16, 16, 32, 32, 64, 64, 64]
    assert rowgroup_passes(200, 128) == [(0, 128), (128, 72)]
    assert rowgroup_passes(200, 100) == [(0, 96), (96, 96), (192, 8)]
    assert rowgroup_passes(24, 4) == [(0, 8), (8, 8), (16, 8)]
    assert rowgroup_passes(520, 0) == [(0, 512), (512, 8)]
    # the widths of the issue's table, per (VEC, LPR), and the column loop
    for (dt, vec), widths in GENERIC_F.items():
        got = [launch_lpr(dt, "i32", launch_vec(dt, F, 0, F, 0, F), F, 142, 1, 0) for F in widths]
        assert [k[3] for k in got] == [vec] * 6 and [k[4] for k in got] == [4, 8, 16, 32, 64, 64]
        assert widths[5] > 64 * vec >= widths[4]
    # the bf16 column passes of variant 2 keep their vector width at the pass offsets
    assert reach(CallSpec("ladder", 120, "w2"), RunSpec("bf16", "i32", 2, 0, 60)) == \
        [("v2", "bf16", "i32", 4, 16, False)] * 2
    assert reach(CallSpec("ladder", 141, "w1"), RunSpec("bf16", "i32", 1, 0, 47)) == \
        [("v1", "bf16", "i32", 1, 64)] * 3
    # the edited test_spmm_variants_agree_ragged_rows: with the fp32 row-group kernel off
    # its parameters select the kernels they name
    for F in (16, 40, 64, 128, 256):
        assert reach(CallSpec("ladder", F, "w0"), RunSpec("f32", "i32", 1, 0, rg32=True)) == \
            [("f32rg",)]
        assert reach(CallSpec("ladder", F, "w0"), RunSpec("f32", "i32", 1, 0))[0][0] == "v1"


# --------------------------------------------------------- preconditions of every case
@pytest.mark.parametrize("group", list(TABLE))
def test_exactness_preconditions(group):
    """Every call of the table: :func:`exact_ok` on the reference alone."""
    for spec, _ in TABLE[group]:
        if spec.pat == "many":
            c = make_call(spec)
            exact_ok(c, formula(c))
        else:
            ladder_case(spec)


def test_peak_of_the_long_row():
    """The largest sum of |terms|, in units of the smallest fraction: the 1,027-entry row
    at 8 x 2 x 2 (+ 16) x 2^6 stays under 2^24; confirmed on the cases, not trusted."""
    assert 1027 * 8 * 2 * 2 * 2 ** 6 + 16 * 2 ** 6 < 2 ** 24
    worst = 0.0
    for F in (47, 520):
        c, _ = ladder_case(CallSpec("ladder", F, "w3", 1, True))
        worst = max(worst, float(formula(c, absolute=True).max()) * 2 ** frac_bits(c))
    assert 2 ** 16 < worst < 2 ** 24, worst


def test_hub_preconditions():
    for (dt, F, _view) in HUB_CASES:
        for fam in FAMS:
            c = make_hub_call(F, fam)
            hub_exact_ok(c, hub_oracle(c))
    beg, end = hub_segments()
    assert (end - beg).tolist() == list(SEG_LENS) and int(end.max()) <= ladder_csr().nnz
    for F in (6, 47, 130):
        for scaled in (False, True):
            c = make_reduce_call(F, scaled)
            ref = reduce_formula(c)
            assert torch.equal(ref, ref.float().double())
            assert float(ref.abs().max()) * 4 < 2 ** 24
    for dt, widths in SPLIT_F.items():
        for F in widths:
            for cap in SPLIT_CAPS:
                for spec in split_specs(F):
                    c, ref = ladder_case(spec)
                    main, tail = split_parts(c, cap)
                    for t in (main, tail):
                        assert torch.equal(t, t.float().double())
                    assert torch.equal(main + tail * (tail != 0), ref)


# ------------------------------------------------- the formula is the CPU path of K.spmm
def _cpu_path(c, dtype, split_cap=0):
    """``K.spmm`` on CPU tensors of ``dtype``: the whole output buffer."""
    out = c["out0"].to(dtype).clone()
    csr = CSR(c["rowptr"], c["col"], c["x"].shape[0], row_map=c.get("row_map"))
    opt = {k: (None if c.get(k) is None else c[k].to(torch.float64 if dtype == torch.float64
                                                      else torch.float32))
           for k in ("edge_weight", "col_scale", "row_scale")}
    split = csr.hub_split(split_cap) if split_cap else None
    assert split_cap == 0 or split is not None
    K.spmm(c["rowptr"], c["col"], c["x"].to(dtype), out, heads=c.get("heads", 1),
           beta=c["beta"], split=split, row_map=c.get("row_map"), **opt)
    return out


@pytest.mark.parametrize("spec", [
    CallSpec("ladder", 12, "w3", 4, True), CallSpec("ladder", 6, "w1", 2),
    CallSpec("ladderc", 13, "w3", 1, True), CallSpec("ladderc", 24, "w3", 2, True),
    CallSpec("ladder", 28, "w2", 1, True), CallSpec("ladder", 7, "w0")], ids=str)
def test_formula_is_the_cpu_path(spec):
    """In fp64 the written-out formula equals the CPU path of ``K.spmm`` (heads, row_map,
    and ``split``); in fp32, on exact inputs, it equals it bitwise too: another summation
    order and another precision change nothing."""
    c, ref = ladder_case(spec)
    if spec.pat == "ladder":  # (rows outside a row_map keep the sentinel: not rounded)
        assert torch.equal(_cpu_path(c, torch.float64), ref)
    assert torch.equal(_cpu_path(c, torch.float32).double(), ref)
    assert torch.equal(formula(c, torch.float32).double(), ref)
    assert_exact(ref.float(), c, "f32")
    assert_exact(_cpu_path(c, torch.bfloat16), c, "bf16")
    if spec.heads == 1:
        for cap in SPLIT_CAPS:
            assert torch.equal(_cpu_path(c, torch.float32, cap).double(), ref)
            assert_same(_cpu_path(c, torch.bfloat16, cap), split_expect(c, cap, "bf16"))
            assert torch.equal(split_expect(c, cap, "f32"), ref)


@pytest.mark.parametrize("cap", CAPS)
def test_formula_cap_is_the_cpu_path(cap):
    """``cap`` reaches ``K.spmm`` through a split only; the capped main pass itself is
    ``reference.spmm(cap=...)``."""
    c, ref = ladder_case(CallSpec("ladder", 14, "w1", 2, False, cap))
    out = c["out0"].clone()
    R.spmm(c["rowptr"], c["col"], c["x"], out, c["edge_weight"], None, None, 2, 0.0, cap)
    assert torch.equal(out.double(), ref)
    deg = c["rowptr"][1:] - c["rowptr"][:-1]
    assert bool((deg < cap).any() and (deg == cap).any() and (deg > cap).any())
    full = formula(dict(c, cap=0))
    assert torch.equal(full[deg <= cap], ref[deg <= cap])
    assert not torch.equal(full[deg > cap], ref[deg > cap])


def test_hub_formulas_are_the_cpu_path():
    c = make_hub_call(47, "w3")
    ref = hub_oracle(c)
    part = torch.empty(len(SEG_LENS), 47)
    R.spmm_hub_partials(c["beg"], c["end"], c["col"], c["x"], part, c["ew"], c["cs"])
    assert torch.equal(part.double(), ref)
    assert torch.equal(hub_oracle(c, torch.float32).double(), ref)
    r = make_reduce_call(47, True)
    out = r["out0"].clone()
    R.spmm_hub_reduce(r["part"], r["seg_ptr"], r["rows"], out, r["rs"])
    assert torch.equal(out.double(), reduce_formula(r))


# ------------------------------------------------------------------------------ mutations
def _must_fail(check, *args, **kw):
    with pytest.raises(AssertionError):
        check(*args, **kw)


def _edit(c, e: int, dup: bool):
    """The call with entry ``e`` dropped, or (``dup``) present twice."""
    E = c["col"].numel()
    idx = torch.cat([torch.arange(e + 1 if dup else e), torch.arange(e if dup else e + 1, E)])
    rp = c["rowptr"].clone()
    r = int(torch.nonzero(rp > e)[0]) - 1  # the row that holds e
    rp[r + 1:] += 1 if dup else -1
    out = dict(c, rowptr=rp, col=c["col"][idx])
    if c.get("edge_weight") is not None:
        out["edge_weight"] = c["edge_weight"][idx]
    return out


def _without(c, e: int):
    return _edit(c, e, False)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_mutations_are_caught(dt):
    """Each by construction on the CPU; the exact comparison must reject every one (and
    accept the right result)."""
    spec = CallSpec("ladderc", 12, "w3", 4, True)
    c, ref = ladder_case(spec)
    rnd = (lambda t: t.float()) if dt == "f32" else (lambda t: t.float().bfloat16())
    assert_exact(rnd(ref), c, dt, ref)
    rp = c["rowptr"]
    r = 29  # compacted row 29 = ladder row 30: 30 entries
    # an entry of the row whose term is not zero in every head
    live = (c["edge_weight"][rp[r]:rp[r + 1]] != 0).all(1) & \
        (c["x"][c["col"][rp[r]:rp[r + 1]]] != 0).all(1)
    e = int(rp[r]) + int(torch.nonzero(live)[0])
    # one entry dropped
    dropped = _without(c, e)
    assert int(dropped["rowptr"][-1]) == int(rp[-1]) - 1
    assert torch.equal(dropped["rowptr"][:r + 1], rp[:r + 1])
    assert int(dropped["rowptr"][r + 1]) == int(rp[r + 1]) - 1
    _must_fail(assert_exact, rnd(formula(dropped)), c, dt, ref)
    # one entry doubled
    doubled = _edit(c, e, True)
    assert doubled["col"][e] == doubled["col"][e + 1] == c["col"][e]
    _must_fail(assert_exact, rnd(formula(doubled)), c, dt, ref)
    # the head of an edge weight off by one
    ewh = c["edge_weight"].clone()
    ewh[rp[r]:rp[r + 1]] = ewh[rp[r]:rp[r + 1]].roll(1, dims=1)
    _must_fail(assert_exact, rnd(formula(dict(c, edge_weight=ewh))), c, dt, ref)
    # row_scale read at the CSR row instead of the mapped output row
    n = rp.numel() - 1
    rs = c["row_scale"].clone()
    rs[c["row_map"]] = c["row_scale"][:n]
    assert not torch.equal(rs, c["row_scale"])
    _must_fail(assert_exact, rnd(formula(dict(c, row_scale=rs))), c, dt, ref)
    # cap off by one
    cc, cref = ladder_case(CallSpec("ladder", 13, "w1", 1, True, 64))
    for cap in (63, 65):
        _must_fail(assert_exact, rnd(formula(dict(cc, cap=cap))), cc, dt, cref)
    assert_exact(rnd(cref), cc, dt, cref)
    # two hub segments swapped between hubs
    rc = make_reduce_call(47, True)
    want = expect(reduce_formula(rc), dt)
    assert_same(want, want)
    swapped = rc["part"].clone()
    swapped[[0, 1]] = rc["part"][[1, 0]]  # segment 0 of hub 0 <-> segment 0 of hub 1
    _must_fail(assert_same, expect(reduce_formula(rc, part=swapped), dt), want)
    # one partial row of the hand-made segments short by its last entry
    hc = make_hub_call(47, "w3")
    short = dict(hc, end=hc["end"] - (torch.arange(len(SEG_LENS)) == 5).long())
    _must_fail(assert_same, hub_oracle(short), hub_oracle(hc))


def test_bf16_rounding_toward_zero_is_caught():
    c, ref = ladder_case(CallSpec("ladder", 28, "w3", 1, True))
    rne = ref.float().bfloat16()
    bits = ref.float().view(torch.int32)
    rtz = (bits & ~0xFFFF).view(torch.float32).bfloat16()
    assert bool((rtz.double() != rne.double()).any())  # some result is not a bf16 number
    assert_exact(rne, c, "bf16", ref)
    _must_fail(assert_exact, rtz, c, "bf16", ref)
    # and the two roundings of the hub path are not one
    c40, _ = ladder_case(CallSpec("ladder", 40, "w3", 1, True))
    once = expect(formula(c40), "bf16")
    assert any(not torch.equal(split_expect(c40, cap, "bf16"), once) for cap in SPLIT_CAPS)


# --------------------------------------------------- the CPU path on the full-mantissa cases
NORMAL_SPECS = (CallSpec("ladder", 47, "w3", 1, True), CallSpec("ladder", 124, "w3", 1, True),
                CallSpec("ladder", 24, "w3", 2, True), CallSpec("ladder", 264, "w3", 1, True))


def normal_case(spec: CallSpec, dt: str):
    """(call as the kernel sees it, fp64 reference, fp32 reference)."""
    c = make_call(spec, normal=True)
    c = as_bf16(c) if dt == "bf16" else c
    return c, formula(c), formula(c, torch.float32)


def split_normal_case(spec: CallSpec, dt: str, cap: int):
    """... and the fp64 main pass, the value the first rounding of the hub path sees."""
    c, ref64, ref32 = normal_case(spec, dt)
    return c, ref64, ref32, split_parts(c, cap)[0]


def test_cpu_path_meets_the_rule():
    """The CPU path of ``K.spmm`` meets the allowance of the GPU tests on their own
    full-mantissa inputs (measured against fp64, never against a kernel)."""
    worst = {}
    for dt, tdt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        for spec in NORMAL_SPECS:
            c, ref64, ref32 = normal_case(spec, dt)
            worst["generic " + dt] = max(worst.get("generic " + dt, 0.0), assert_bound(
                _cpu_path(c, tdt), ref64, ref32, dt, label=f"cpu {spec.F}"))
            if spec.heads == 1:
                for cap in SPLIT_CAPS:
                    c, ref64, ref32, main = split_normal_case(spec, dt, cap)
                    worst["split " + dt] = max(worst.get("split " + dt, 0.0), assert_bound(
                        _cpu_path(c, tdt, cap), ref64, ref32, dt, (main,), f"cpu split {cap}"))
    for F in (47, 130):
        c = make_hub_call(F, "w3", normal=True)
        part = torch.empty(len(SEG_LENS), F)
        R.spmm_hub_partials(c["beg"], c["end"], c["col"], c["x"], part, c["ew"], c["cs"])
        worst["partials"] = max(worst.get("partials", 0.0), assert_bound(
            part, hub_oracle(c), hub_oracle(c, torch.float32), "f32", label="cpu partials"))
    for k, v in worst.items():
        print(f"cpu path {k}: largest error / allowance {v:.3f}")
    # the rule bites: an operand rounded to bf16 fails the fp32 comparison
    c, ref64, ref32 = normal_case(NORMAL_SPECS[1], "f32")
    _must_fail(assert_bound, formula(as_bf16(c)).float(), ref64, ref32, "f32")
    # and a dropped entry of a degree-100 row fails the bf16 one
    c, ref64, ref32 = normal_case(NORMAL_SPECS[1], "bf16")
    e = int(c["rowptr"][100]) + 50
    _must_fail(assert_bound, formula(_without(c, e)).float().bfloat16(), ref64, ref32, "bf16")


def test_with_idx_keeps_the_pattern():
    for pat in ("ladder", "ladderc", "many"):
        csr = csr_of(pat)
        lo = with_idx(csr, torch.int32)
        assert lo.col.dtype == torch.int32 and torch.equal(lo.col.long(), csr.col.long())
    assert csr_of("ladderc").row_map.tolist() == list(range(1, 142))
