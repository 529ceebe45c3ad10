"""Every compiled variant of the fp32 row-group SpMM (csrc/kernels/spmm_f32.hip) against
the fp64 CPU path of :func:`dgraph_amd.ops.f32.spmm_f32`, on one small pattern that holds
every degree edge of every lane-group width.

Two comparisons (the helpers are shared with test_f32_oracles.py, which shows on the CPU
that they bite):

* exact -- values are small dyadic numbers (``ALPHABETS``), so every fp32 product and every
  partial sum in any order is exact and the kernel must equal fp64 bitwise
  (:func:`assert_exact`). The condition that makes this legitimate is asserted on the
  reference alone, first (:func:`exact_ok`).
* full mantissa -- unit-normal values against ``bound(ref64, ref32)`` of
  test_gat_kernels.py (2e-5 floor, 8x the error of the same formula in fp32 on the CPU):
  small integers are exact in bf16 / tf32 too, so only these cases see a reduced-precision
  product.

Variants launched (104 = 2 index types x 4 lane-group widths x 13 families). Every
``test_variant_sweep[idx-family-F]`` case maps to ``(index type, LPR, WMODE, CMAP, TWO,
KB, GS)`` as follows; ``idx`` is the index type, ``F`` picks LPR, ``family`` the rest:

    F (single pass)   4, 20 -> LPR 8    36, 64 -> LPR 16    68, 128 -> LPR 32
                      132, 256 -> LPR 64
    F (two passes)    260 -> LPR 64 + a 4-wide tail (LPR 8)
                      320 -> LPR 64 + a 64-wide tail (LPR 16)

    family   WMODE  CMAP  TWO  KB  GS        family   WMODE  CMAP  TWO  KB  GS
    w0         0     -     -   -   -         w0m        0     x     -   -   -
    w1 (ew)    1     -     -   -   -         w1m        1     x     -   -   -
    w2 (cs)    2     -     -   -   -         w2m        2     x     -   -   -
    w3         3     -     -   -   -         w3m        3     x     -   -   -
    two        0     -     x   -   -         twom       0     x     x   -   -
    kb         0     -     -   x   -         gs         0     x     -   -   x
                                             gs2        0     x     x   -   x

Every family runs with the plain epilogue and with ``beta != 0`` + ``row_scale``; the
column-mapped families at two map fractions per width (5 % and all, or 50 % and none).
``kb`` rounds F up to whole 32-column keep words (32, 32, 64, 64, 96, 128, 160, 256: the
same LPR; 288 = 256 + a 32-wide tail at LPR 8; 320).
"""
from __future__ import annotations

import functools

import pytest
import torch

from dgraph_amd.ops import f32 as F32
from test_gat_kernels import bound

pytestmark = pytest.mark.gpu
DEV = "cuda"

NROWS, NCOL, HUB = 132, 300, 700
ALPHABETS = dict(ew=(0.0, 0.5, 1.0, 2.0, -1.0), scale=(0.25, 0.5, 1.0, 2.0),
                 beta=(1.0, 0.5, -2.0))
FAMILIES = ("w0", "w1", "w2", "w3", "w0m", "w1m", "w2m", "w3m", "two", "twom", "kb", "gs",
            "gs2")
WIDTHS = (4, 20, 36, 64, 68, 128, 132, 256)  # two per lane-group width 8 / 16 / 32 / 64
FRACS = {0: (0.05, 1.0), 1: (0.5, 0.0)}  # map fractions of the 1st / 2nd width of an LPR
SENT = -12345.0  # sentinel of memory a call must not write
NSPLIT = 170


def _seed(*key) -> int:
    s = 0
    for ch in "/".join(str(k) for k in key):
        s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return s


def gen(*key) -> torch.Generator:
    """A generator seeded by the case's key (stable across processes, unlike ``hash``)."""
    return torch.Generator().manual_seed(_seed(*key))


def pick(alphabet, shape, g) -> torch.Tensor:
    a = torch.tensor(alphabet, dtype=torch.float32)
    return a[torch.randint(0, len(alphabet), shape, generator=g)]


def ints(shape, g, lo=-8, hi=8) -> torch.Tensor:
    return torch.randint(lo, hi + 1, shape, generator=g).float()


@functools.lru_cache(maxsize=None)
def pattern():
    """(rowptr int64 [133], col int64 [E]): 132 rows -- an empty first row, degrees 1..129
    shuffled (every ``deg mod LPR``, a whole chunk, a chunk plus one and the 8-row batch
    edges for LPR 8..64), one row of degree 700 at row 2, an empty last row; 300 columns,
    the second entry of every row repeating its first."""
    g = gen("pattern")
    deg = (torch.randperm(129, generator=g) + 1).tolist()
    deg = [0, deg[0], HUB] + deg[1:] + [0]
    assert len(deg) == NROWS and set(range(130)) <= set(deg)
    rp = torch.zeros(NROWS + 1, dtype=torch.long)
    rp[1:] = torch.cumsum(torch.tensor(deg), 0)
    col = torch.randint(0, NCOL, (int(rp[-1]),), generator=g)
    two = torch.tensor(deg) >= 2
    col[rp[:-1][two] + 1] = col[rp[:-1][two]]
    return rp, col


# ------------------------------------------------------------------------------ calls
# A call is a dict of CPU tensors / scalars: rowptr, col, x, out0 (the output buffer before
# the call) and the optional operands of spmm_f32 under their keyword names.
OPT = ("edge_weight", "col_scale", "row_scale", "col_map", "row_ids", "row_map", "gate",
       "self_add", "self_map", "rowend", "x2", "keep_bits")


def pack_bits(mask: torch.Tensor) -> torch.Tensor:
    """[n, F] bool -> [n, F/32] int32 keep words (bit c % 32 of word c / 32: column c)."""
    n, F = mask.shape
    w = (mask.view(n, F // 32, 32).long() << torch.arange(32)).sum(-1)
    return ((w + (1 << 31)) % (1 << 32) - (1 << 31)).to(torch.int32)


def col_map_of(frac: float, g, ncol=NCOL):
    """int32 [ncol] map onto ``round(frac * ncol)`` compacted rows (-1: unmapped)."""
    nk = int(round(frac * ncol))
    keep = torch.randperm(ncol, generator=g)[:nk].sort().values
    cmap = torch.full((ncol,), -1, dtype=torch.int32)
    cmap[keep] = torch.arange(nk, dtype=torch.int32)
    return cmap, nk


def make_call(family: str, F: int, frac: float = 1.0, epi: bool = False, normal: bool = False,
              key=()):
    """The call of one variant family on :func:`pattern`. ``epi``: ``beta != 0`` on integer
    old contents plus ``row_scale``. ``normal``: unit-normal values and uniform weights
    instead of the exact alphabets."""
    g = gen(family, F, frac, epi, normal, *key)
    rp, col = pattern()
    val = (lambda shape: torch.randn(shape, generator=g)) if normal else \
        (lambda shape: ints(shape, g))
    c = dict(rowptr=rp, col=col, beta=0.0, out0=torch.full((NROWS, F), SENT))
    cmap_on = family.endswith("m") or family.startswith("gs")
    two = family in ("two", "twom", "gs2")
    wmode = int(family[1]) if family[0] == "w" else 0
    nsrc = NCOL
    if cmap_on:
        c["col_map"], nsrc = col_map_of(frac, g)
    if two:
        # (with nothing mapped both sources keep one readable row: column 0's padding slot)
        ns = NSPLIT if not cmap_on else max(nsrc // 2, 1)
        c["x"], c["x2"], c["nsplit"] = val((ns, F)), val((max(nsrc - ns, 1), F)), ns
    else:
        c["x"] = val((max(nsrc, 1), F))
    if wmode & 1:
        c["edge_weight"] = torch.rand(col.numel(), generator=g) if normal else \
            pick(ALPHABETS["ew"], (col.numel(),), g)
    if wmode & 2:
        cs = torch.rand(c["x"].shape[0], generator=g) if normal else \
            pick(ALPHABETS["scale"], (c["x"].shape[0],), g)
        cs[torch.rand(cs.numel(), generator=g) < 0.05] = 0.0  # "unmapped" to the compaction
        c["col_scale"] = cs
    if family == "kb":
        c["keep_mask"] = torch.rand(NROWS, F + (-F) % 32, generator=g) < 0.5
        c["keep_bits"] = pack_bits(c["keep_mask"])
    if family.startswith("gs"):
        nself = 40
        sm = torch.full((NROWS + 3,), -1, dtype=torch.int32)
        at = torch.randperm(NROWS + 3, generator=g)[:90]
        sm[at] = torch.randint(0, nself, (90,), generator=g).to(torch.int32)
        gate = torch.randn(NROWS, F, generator=g) if normal else ints((NROWS, F), g, -2, 2)
        c.update(self_add=val((nself, F)), self_map=sm, self_row0=3, gate=gate)
    if epi:
        c["out0"] = val((NROWS, F))
        c["beta"] = ALPHABETS["beta"][_seed(family, F, frac) % 3]
        c["row_scale"] = torch.rand(NROWS, generator=g) + 0.5 if normal else \
            pick(ALPHABETS["scale"], (NROWS,), g)
    return c


def _kw(c, absolute=False):
    a = (lambda t: t.abs()) if absolute else (lambda t: t)
    kw = {k: c[k] for k in OPT if c.get(k) is not None}
    for k in ("edge_weight", "col_scale", "x2", "self_add"):
        if k in kw:
            kw[k] = a(kw[k])
    kw.update(beta=abs(c["beta"]) if absolute else c["beta"], nsplit=c.get("nsplit", 0),
              self_row0=c.get("self_row0", 0))
    if absolute:
        kw.pop("gate", None)
        kw.pop("keep_bits", None)
        if "row_scale" in kw:  # bounds the sums before and after the row scale
            kw["row_scale"] = kw["row_scale"].clamp_min(1.0)
    return kw


def oracle(c, absolute=False) -> torch.Tensor:
    """The fp64 CPU path of ``F32.spmm_f32`` on the call: the whole output buffer, fp64.
    ``absolute``: the same sum over |terms| with every gate open (the exactness bound)."""
    x = c["x"].abs() if absolute else c["x"]
    out = (c["out0"].abs() if absolute else c["out0"]).double().clone()
    F32.spmm_f32(c["rowptr"], c["col"], x, out, **_kw(c, absolute))
    return out


def formula(c, dtype) -> torch.Tensor:
    """The definition written out once more, evaluated in ``dtype`` (fp32: the ``ref32`` of
    ``bound``; fp64: equal to :func:`oracle`, asserted in test_f32_oracles.py)."""
    rp = c["rowptr"]
    re = c["rowend"] if c.get("rowend") is not None else rp[1:]
    nr = re.numel()
    rows = c["row_ids"] if c.get("row_ids") is not None else torch.arange(nr)
    n = rows.numel()
    o = c["row_map"] if c.get("row_map") is not None else torch.arange(n)
    out = c["out0"].to(dtype).clone()
    F = c["x"].shape[1]
    src = c["x"].to(dtype)
    if c.get("x2") is not None:
        pad = torch.zeros(c["nsplit"] - min(c["nsplit"], src.shape[0]), F, dtype=dtype)
        src = torch.cat([src[:c["nsplit"]], pad, c["x2"].to(dtype)], 0)
    for i in range(n):
        r = int(rows[i])
        e = torch.arange(int(rp[r]), int(re[r]))
        cc = c["col"][e].long()
        w = torch.ones(e.numel(), dtype=dtype)
        if c.get("edge_weight") is not None:
            w = w * c["edge_weight"][e].to(dtype)
        if c.get("col_map") is not None:
            cc = c["col_map"][cc].long()
            w, cc = w[cc >= 0], cc[cc >= 0]
        if c.get("col_scale") is not None:
            w = w * c["col_scale"][cc].to(dtype)
        v = (src[cc] * w.unsqueeze(1)).sum(0) if e.numel() else torch.zeros(F, dtype=dtype)
        oi = int(o[i])
        if c.get("row_scale") is not None:
            v = v * c["row_scale"][oi].to(dtype)
        if c["beta"] != 0.0:
            v = v + c["beta"] * out[oi]
        if c.get("self_add") is not None:
            m = int(c["self_map"][c.get("self_row0", 0) + oi])
            if m >= 0:
                v = v + c["self_add"][m, :F].to(dtype)
        if c.get("gate") is not None:
            v = torch.where(c["gate"][oi, :F] > 0, v, torch.zeros_like(v))
        if c.get("keep_bits") is not None:
            v = torch.where(F32.unpack_keep_bits(c["keep_bits"][oi:oi + 1], F)[0], v,
                            torch.zeros_like(v))
        out[oi] = v
    return out


def frac_bits(c) -> int:
    """Fractional bits a partial result of the call can hold, given ``ALPHABETS``."""
    return ((1 if c.get("edge_weight") is not None else 0)
            + (2 if c.get("col_scale") is not None else 0)
            + (2 if c.get("row_scale") is not None else 0)
            + (1 if float(c["beta"]) != int(c["beta"]) else 0))


def exact_ok(c, ref64: torch.Tensor) -> None:
    """What makes a bitwise comparison legitimate, asserted on the reference alone: the
    result is an fp32 number, and the sum of |terms| of every output element, in units of
    the smallest fraction in use, stays below 2^24 (so every partial sum in every order is
    an fp32 number too)."""
    assert torch.equal(ref64, ref64.float().double()), "reference is not exact in fp32"
    peak = float(oracle(c, absolute=True).abs().max())
    assert peak * 2 ** frac_bits(c) < 2 ** 24, (peak, frac_bits(c))


def assert_exact(got: torch.Tensor, c, ref64: torch.Tensor | None = None,
                 checked: bool = False) -> None:
    """``got`` (the whole output buffer of the call) equals the fp64 reference bitwise.
    ``checked``: the caller has run :func:`exact_ok` on this call already."""
    ref64 = oracle(c) if ref64 is None else ref64
    if not checked:
        exact_ok(c, ref64)
    g64 = got.double().cpu()
    if not torch.equal(g64, ref64):
        bad = torch.nonzero((g64 != ref64) | (g64.isnan() != ref64.isnan()))
        r, f = (int(v) for v in bad[0])
        raise AssertionError(f"{bad.shape[0]} elements differ; first at row {r} column {f}: "
                             f"got {float(g64[r, f])}, expected {float(ref64[r, f])}")


def assert_bound(got: torch.Tensor, c) -> None:
    """Full-mantissa comparison: ``|got - fp64| <= bound(fp64, fp32 on the CPU)``."""
    ref64, ref32 = oracle(c), formula(c, torch.float32)
    err = float((got.double().cpu() - ref64).abs().max())
    lim = bound(ref64, ref32)
    print(f"spmm_f32 err {err:.3e} bound {lim:.3e} "
          f"fp32-cpu err {float((ref32.double() - ref64).abs().max()):.3e}")
    assert err <= lim, (err, lim)


# ------------------------------------------------------------------------------ GPU side
def widen(t: torch.Tensor, off: int = 4, extra: int = 8):
    """``t`` as a column slice of a wider device buffer (16-byte aligned offset) filled
    with the sentinel: (buffer, view)."""
    buf = torch.full((t.shape[0], off + t.shape[1] + extra), SENT, device=DEV)
    view = buf[:, off:off + t.shape[1]]
    view.copy_(t)
    return buf, view


def run_gpu(c, idx=torch.int32, pass_cols=256, cap=0, wide=False, rowptr_dev=None):
    """The call through the raw op; returns the output buffer (CPU). ``wide``: x, x2, out,
    gate and self_add are column slices of wider buffers whose other columns must keep the
    sentinel."""
    from dgraph_amd import _native

    d = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
    bufs = []
    if wide:
        for k in ("x", "x2", "out0", "gate", "self_add"):
            if d.get(k) is not None:
                buf, d[k] = widen(d[k], 4 if k != "x2" else 8)
                bufs.append((k, buf, d[k].shape[1], 4 if k != "x2" else 8))
    out = d["out0"] if wide else d["out0"].clone()
    _native.ops().spmm_f32_ex(
        d["rowptr"] if rowptr_dev is None else rowptr_dev, d["col"].to(idx),
        d.get("edge_weight"), d.get("col_scale"), d.get("row_scale"), d.get("col_map"),
        d.get("row_ids"), d["x"], out, float(c["beta"]), int(cap), d.get("row_map"),
        d.get("gate"), d.get("self_add"), d.get("self_map"), int(c.get("self_row0", 0)),
        d.get("rowend"), d.get("x2"), int(c.get("nsplit", 0)), int(pass_cols),
        d.get("keep_bits"))
    torch.cuda.synchronize()
    for k, buf, w, off in bufs:
        b = buf.cpu()
        assert bool((b[:, :off] == SENT).all()) and bool((b[:, off + w:] == SENT).all()), k
    return out.cpu()


def _fracs(family, F):
    if not (family.endswith("m") or family.startswith("gs")):
        return (1.0,)
    return FRACS[WIDTHS.index(F) % 2] if F in WIDTHS else (0.5, 1.0)


@functools.lru_cache(maxsize=None)
def _case(family, F, frac, epi):
    """(call, fp64 reference): shared by the two index types."""
    c = make_call(family, F, frac, epi)
    ref = oracle(c)
    exact_ok(c, ref)
    return c, ref


@pytest.mark.parametrize("F", WIDTHS + (260, 320))
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("idx", [torch.int32, torch.int64], ids=["i32", "i64"])
def test_variant_sweep(idx, family, F):
    """Each variant (the module docstring's table), plain epilogue and beta + row_scale,
    exact. F = 260 / 320: two column passes with a 4- / 64-wide tail."""
    if family == "kb" and F % 32:
        F += (-F) % 32  # keep words hold whole 32-column groups: 32, 64, 96, 160, 288, 320
    for frac in _fracs(family, F):
        for epi in (False, True):
            c, ref = _case(family, F, frac, epi)
            assert_exact(run_gpu(c, idx), c, ref, checked=True)


@pytest.mark.parametrize("F", [20, 64, 128, 256])
@pytest.mark.parametrize("nrows", [1, 3, 5, 31, 33, 132])
def test_partial_tails(nrows, F):
    """Row counts that leave every rows-per-wave (8 / 4 / 2 / 1) and the 4-wave block a
    partial tail, through ``rowptr[:nrows + 1]``; plain and column-mapped; rows of ``out``
    past ``nrows`` keep the sentinel (part of the comparison)."""
    for family in ("w0", "w3m"):
        c = dict(make_call(family, F, 0.5, True))
        c["rowptr"] = c["rowptr"][:nrows + 1]
        c["out0"] = c["out0"].clone()
        c["out0"][nrows:] = SENT
        assert_exact(run_gpu(c), c)


def split_points(g):
    rp, _ = pattern()
    deg = rp[1:] - rp[:-1]
    return rp[:-1] + (torch.rand(NROWS, generator=g) * (deg + 1).double()).long().clamp(max=deg)


@pytest.mark.parametrize("idx", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("F", [20, 64, 128, 256])
def test_rowend_split_rows(F, idx):
    """``rowend``: every row cut at a random point. The first part, then the second with
    ``beta = 1`` (two calls), equal the unsplit row; so does one two-source call whose
    second-part columns point into ``x2``. Edge weights ride along (indexed by entry)."""
    g = gen("rowend", F)
    rp, col = pattern()
    mid = split_points(g)
    whole = dict(make_call("w1", F, key=("rowend",)))
    ref = oracle(whole)
    first = dict(whole, rowend=mid)
    got = run_gpu(first, idx)
    assert_exact(got, first)
    second = dict(whole, rowptr=mid, rowend=rp[1:].contiguous(), beta=1.0, out0=got)
    assert_exact(run_gpu(second, idx), second, ref)
    # one call: entries at or after the cut read x2 (= x) through columns shifted by NCOL
    e = torch.arange(col.numel())
    seg = torch.repeat_interleave(torch.arange(NROWS), rp[1:] - rp[:-1])
    both = dict(make_call("w0", F, key=("rowend",)))
    ref = oracle(both)
    both.update(col=torch.where(e >= mid[seg], col + NCOL, col), x2=both["x"], nsplit=NCOL)
    assert_exact(run_gpu(both, idx), both, ref)


@pytest.mark.parametrize("F", [36, 256])
def test_rowptr_views_row_ids_row_map(F):
    """``rowptr[r0:r1 + 1]`` views as the executor passes them; ``row_ids`` with repeats;
    ``row_map`` as a permutation into a larger ``out`` whose other rows keep the sentinel;
    every operand a column slice of a wider buffer."""
    g = gen("views", F)
    r0, r1 = 30, 101
    for family in ("w0", "w2m", "gs"):
        c = dict(make_call(family, F, 0.5, True))
        full = c["rowptr"].to(DEV)
        c["rowptr"] = c["rowptr"][r0:r1 + 1]
        c["out0"] = c["out0"].clone()
        c["out0"][r1 - r0:] = SENT
        assert_exact(run_gpu(c, wide=True, rowptr_dev=full[r0:r1 + 1]), c)
    n = 150
    for family in ("w3", "twom", "kb"):
        c = dict(make_call(family, F, 0.5, False))
        c["row_ids"] = torch.randint(0, NROWS, (n,), generator=g)
        c["row_ids"][:4] = 2  # the degree-700 row, four times in one wave
        c["row_map"] = torch.randperm(n + 37, generator=g)[:n]
        c["out0"] = ints((n + 37, F), g)
        c.update(beta=0.5, row_scale=pick(ALPHABETS["scale"], (n + 37,), g))
        if family == "kb":
            c["keep_mask"] = torch.rand(n + 37, F + (-F) % 32, generator=g) < 0.5
            c["keep_bits"] = pack_bits(c["keep_mask"])
            c["x"], c["out0"] = ints((NCOL, F + (-F) % 32), g), ints((n + 37, F + (-F) % 32), g)
        assert_exact(run_gpu(c, wide=True), c)


@pytest.mark.parametrize("cap", [1, 5, 64])
@pytest.mark.parametrize("F", [20, 256])
def test_cap(F, cap):
    """``cap`` through the raw op: the same call with ``rowend = min(rowptr[r] + cap,
    rowptr[r + 1])``."""
    rp, _ = pattern()
    for family in ("w1", "w0m"):
        c = make_call(family, F, 0.5, True)
        ref = dict(c, rowend=torch.minimum(rp[:-1] + cap, rp[1:]))
        assert_exact(run_gpu(c, cap=cap), ref)


@pytest.mark.parametrize("idx", [torch.int32, torch.int64], ids=["i32", "i64"])
def test_degenerate_sources_and_empty_columns(idx):
    """Two sources with ``nsplit = 0`` (every column reads ``x2``; ``x`` is all NaN and
    must never be read) and with a zero-row ``x2`` (``nsplit`` = rows of ``x``); an empty
    column array with ``nrows > 0`` (the output is the epilogue of a zero sum)."""
    F = 64
    c = dict(make_call("w0", F, epi=True))
    ref = oracle(c)
    a = dict(c, x=torch.full((4, F), float("nan")), x2=c["x"], nsplit=0)
    assert_exact(run_gpu(a, idx), dict(a, x=torch.zeros(4, F)), ref)
    b = dict(c, x2=torch.zeros(8, F)[:0], nsplit=NCOL)
    assert_exact(run_gpu(b, idx), b, ref)
    for family in ("w0", "w0m"):
        e = dict(make_call(family, F, 0.5, True), rowptr=torch.zeros(NROWS + 1, dtype=torch.long),
                 col=torch.zeros(0, dtype=torch.long))
        got = run_gpu(e, idx)
        assert_exact(got, e)
        assert torch.equal(got, (e["beta"] * e["out0"].double()).float())


def poison_unreferenced(c):
    """The call with every row of ``x`` / ``x2`` that no entry of the call's row ranges
    references filled with NaN -- except the rows a padding slot reads with weight 0 by
    design: row 0 of each source and the row column id 0 resolves to."""
    rp = c["rowptr"]
    re = c["rowend"] if c.get("rowend") is not None else rp[1:]
    rows = c["row_ids"] if c.get("row_ids") is not None else torch.arange(re.numel())
    e = torch.cat([torch.arange(int(rp[r]), int(re[r])) for r in rows])
    cc = torch.cat([c["col"][e].long(), torch.zeros(1, dtype=torch.long)])
    if c.get("col_map") is not None:
        cc = c["col_map"][cc].long()
        cc = cc[cc >= 0]
    ns = c["nsplit"] if c.get("x2") is not None else c["x"].shape[0]
    out = dict(c)
    for k, ref in (("x", cc[cc < ns]), ("x2", cc[cc >= ns] - ns)):
        if c.get(k) is None:
            continue
        used = torch.zeros(c[k].shape[0], dtype=torch.bool)
        used[ref] = True
        used[0] = True
        out[k] = torch.where(used.unsqueeze(1), c[k], torch.full_like(c[k], float("nan")))
    return out


STRAY_FAMILIES = ("w0", "w3", "w3m", "two", "twom", "gs2")


def stray_call(family, F):
    c = dict(make_call(family, F, 0.5, False, key=("stray",)))
    c["rowend"] = split_points(gen("stray", family, F))
    c["row_ids"] = torch.tensor([0, 1] + list(range(3, 24)))
    c["out0"] = c["out0"][:23].clone()
    return c


@pytest.mark.parametrize("F", [20, 64, 128, 256])
@pytest.mark.parametrize("family", STRAY_FAMILIES)
def test_no_stray_gather(family, F):
    """A read of a wrong row with weight 0 is invisible to every other test: here every
    unreferenced row is NaN, and the output must stay NaN-free and exact. The call covers
    23 rows (``row_ids``), each cut short with ``rowend``, so that unreferenced rows
    exist."""
    c = stray_call(family, F)
    p = poison_unreferenced(c)
    assert bool(p["x"].isnan().any())
    got = run_gpu(p)
    assert not bool(got.isnan().any())
    assert_exact(got, c)


def _tiled_rows(nblocks: int, lpr: int, g):
    return torch.randint(0, NROWS, (4 * (64 // lpr) * nblocks - 1,), generator=g)


@pytest.mark.parametrize("F", [20, 64, 128, 256])
def test_launch_modes(F):
    """Grid caps 1 and 3 (a persistent grid-stride launch) and the XCD block remap at 7, 8,
    9 and 17 blocks: bitwise the default launch and exact against the reference."""
    from dgraph_amd import _native

    ops = _native.ops()
    lpr = {20: 8, 64: 16, 128: 32, 256: 64}[F]
    g = gen("launch", F)
    try:
        for family in ("w0", "w3m", "gs2"):
            for nblocks in (7, 8, 9, 17):
                c = dict(make_call(family, F, 0.5, False))
                c["row_ids"] = _tiled_rows(nblocks, lpr, g)
                n = c["row_ids"].numel()
                c["out0"] = torch.full((n, F), SENT)
                if family == "gs2":
                    c["gate"] = ints((n, F), g, -2, 2)
                    c["self_map"] = torch.randint(-1, 40, (n + 3,), generator=g).to(torch.int32)
                ref = oracle(c)
                ops.set_f32_sched(0, -1, 0)
                base = run_gpu(c)
                assert_exact(base, c, ref)
                ops.set_f32_sched(0, -1, 1)
                assert torch.equal(run_gpu(c), base), ("xcd", family, nblocks)
                if nblocks in (9, 17):
                    for cap in (1, 3):
                        ops.set_f32_sched(cap, -1, 0)
                        assert torch.equal(run_gpu(c), base), ("grid", cap, family, nblocks)
    finally:
        ops.set_f32_sched(0, 1, 0)


@pytest.mark.parametrize("pc", [16, 48, 64, 256])
@pytest.mark.parametrize("F", [32, 96, 160, 256])
def test_keep_bits_passes(F, pc):
    """The keep-bits epilogue over column passes: ``pass_cols`` = 48 starts passes at bit
    16 of a word. Keep words packed in plain torch from a random mask; the reference is the
    unmasked fp64 result with the mask applied."""
    c = make_call("kb", F, epi=True, key=("passes",))
    plain = {k: v for k, v in c.items() if k not in ("keep_bits", "keep_mask")}
    ref = torch.where(c["keep_mask"], oracle(plain), torch.zeros(1, dtype=torch.float64))
    for idx in (torch.int32, torch.int64):
        assert_exact(run_gpu(c, idx, pass_cols=pc), c, ref)


@pytest.mark.parametrize("F", [20, 64, 128, 256])
@pytest.mark.parametrize("family", ["w0", "w3m", "gs2"])
def test_unit_normal(family, F):
    """Full-mantissa values (degrees <= 700): |kernel - fp64| within ``bound``."""
    c = make_call(family, F, 0.5, True, normal=True)
    assert_bound(run_gpu(c), c)
