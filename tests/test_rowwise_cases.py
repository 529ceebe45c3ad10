"""Inputs, fp64 contracts and selection tables of tests/test_rowwise_variants_gpu.py, which
runs the dense row-wise kernels -- csrc/kernels/layernorm.hip, batchnorm.hip, act.hip,
edge_fused.hip, rows.hip -- at every instantiation their launchers can select, and the CPU
tests that pin all of it down first.

* ``*_select``: each launcher's selection rule restated by hand as a function of (F, element
  size, row strides, base alignment): ``ln_cfg``; ``launch_any`` / ``launch_lpr`` of
  batchnorm; ``bias_act_vec`` and the ``fwd_vec`` / ``bwd_vec`` choice of act; ``pick_vec`` /
  ``lanes_for`` of edge_fused; ``copy_dispatch`` / ``pick_lpr`` of rows. EACH MIRROR MUST BE
  UPDATED WITH ITS LAUNCHER: it checks the tables below, not what a kernel selected.
* ``LN_F`` / ``BN_F`` / ``ACT_F`` / ``EDGE_F`` / ``COPY_F``: the widths of the GPU tests per
  kernel and type; ``test_tables_reach_every_instantiation`` names every instantiation a
  launcher can select and shows that a width of the table reaches it. Most widths leave the
  last lane group or chunk partly empty (the ``f < F`` masks).
* ``*_contract``: plain formulas in a ``dtype`` (fp64: the reference; fp32: the error the
  project's bound is derived from). LayerNorm and BatchNorm are pinned against torch's own
  ``layer_norm`` / ``batch_norm`` autograd in fp64.
* Inputs come from fixed generators: ``randn * 3 + 1``; ``1000 + 0.1 randn`` columns / rows
  (``|mean| >> std``; for bf16 ``1000 + 4 k``, which bf16 holds exactly); one constant
  LayerNorm row; zero-gate cases of small integers with a known count of pre-activations
  that are exactly 0 (exact in bf16 too).
* ``many_rows``: per kernel, the row count at which some waves take a second grid-stride
  step, computed from the mirrored grid caps.
* ``inverse_fmix32`` / ``seed_for_hash``: a dropout seed that makes a chosen element hash
  to a chosen value, for the elements between ``floor(double(p) 2^32)`` and
  ``floor(float32(p) 2^32)``.
"""
from __future__ import annotations

import functools
import math

import pytest
import torch

from dgraph_amd.models.norm import dropout_keep_mask
from test_gat_kernels import bound
from test_segment_cases import ladder_csr

BF16_ULP = 2.0 ** -8  # tests/test_spmm_generic_cases.py: half a bf16 ulp is at most 2^-8 |v|
EPS = 1e-5
ELEM = {"fp32": 4, "bf16": 2}
TORCH_DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
EXTRA = 4099  # rows past one sweep of the grid in the many-rows cases (prime)


def lanes_for(need: int, smallest: int = 4) -> int:
    for lanes in (4, 8, 16, 32):
        if lanes >= smallest and need <= lanes:
            return lanes
    return 64


def _vec_ok(F, V, lds, aligned):
    return F % V == 0 and all(ld % V == 0 for ld in lds) and aligned


# ------------------------------------------------------------------ selection mirrors
def ln_select(F: int, elem: int):
    """``ln_cfg`` of layernorm.hip -> (VEC, LPR, CH). Operands are contiguous and torch
    allocations, so strides and alignment do not enter."""
    V = 16 // elem
    vec = V if F % V == 0 else 1
    per = -(-F // vec)
    lpr = lanes_for(per)
    ch = -(-per // lpr)
    ch = 1 if ch <= 1 else 2 if ch <= 2 else 4 if ch <= 4 else 8
    return vec, lpr, ch


def ln_shape_ok(F: int, elem: int) -> bool:
    """``ln_shape_ok`` of bindings.cpp."""
    V = 16 // elem
    per = F // V if F % V == 0 else F
    return -(-per // 64) <= 8


def bn_select(F: int, elem: int, lds=(), aligned: bool = True):
    """``launch_any`` / ``launch_lpr`` of batchnorm.hip -> (VEC, LPR, column tiles).
    ``lds``: the row strides of x and of dy / out where given; ``aligned``: every base on
    16 bytes."""
    V = 16 // elem
    vec = V if _vec_ok(F, V, lds, aligned) else 1
    lpr = lanes_for(-(-F // vec), 8)
    return vec, lpr, -(-F // (lpr * vec))


def act_select(F: int, elem: int, lds=(), aligned: bool = True):
    """``bias_act_vec`` of act.hip -> VEC, or None where the launcher refuses the width
    (a 256-thread block must hold a row: F <= 256 VEC)."""
    V = 16 // elem
    vec = V if _vec_ok(F, V, lds, aligned) and F // V <= 256 else 1
    return vec if F <= 256 * vec else None


def edge_select(F: int, elem: int, lds=(), aligned: bool = True):
    """``pick_vec`` / ``lanes_for`` of edge_fused.hip -> (VEC, LPR)."""
    V = 16 // elem
    vec = V if _vec_ok(F, V, lds, aligned) else 1
    return vec, lanes_for(-(-F // vec))


def copy_select(F: int, elem: int, lds=(), align: int = 16, acc: bool = False):
    """``copy_dispatch`` / ``pick_lpr`` of rows.hip -> (VEC, LPR). ``align``: the largest
    power of two (up to 16 bytes) that divides every base address."""
    def ok(v):
        return F % v == 0 and all(ld % v == 0 for ld in lds) and align % (v * elem) == 0
    if acc:
        assert elem == 4, "accumulate needs an fp32 output"
        vec = 4 if ok(4) else 1
    else:
        V = 16 // elem
        vec = V if ok(V) else 2 if ok(2) else 1
    return vec, lanes_for(-(-F // vec))


# ------------------------------------------------------------------------- the tables
# (type, path) -> widths. "vec": contiguous, aligned operands; "scalar": widths no vector
# divides; "vec2" (copy_rows): widths only the 2-element vector divides.
LN_F = {
    ("fp32", "vec"): (12, 20, 36, 68, 172, 260, 600, 1284, 2048),
    ("fp32", "scalar"): (3, 7, 13, 29, 50, 73, 150, 333, 511),
    ("bf16", "vec"): (24, 40, 72, 136, 344, 520, 1200, 2568, 4096),
    ("bf16", "scalar"): (3, 7, 13, 29, 50, 73, 150, 333, 511),
}
# the widest width ln_shape_ok admits per path (vector, scalar; 512 itself is a vector width)
LN_LIMIT = {"fp32": (2048, 511), "bf16": (4096, 511)}
LN_PAST = {"fp32": (2052, 513), "bf16": (4104, 513)}
BN_F = {
    ("fp32", "vec"): (12, 36, 68, 172, 600),
    ("fp32", "scalar"): (7, 13, 29, 50, 150, 257),
    ("bf16", "vec"): (24, 72, 136, 344, 1032),
    ("bf16", "scalar"): (7, 13, 29, 50, 150, 257),
}
ACT_F = {
    ("fp32", "vec"): (12, 128, 172, 600, 1024),
    ("fp32", "scalar"): (3, 7, 73, 150, 255),
    ("bf16", "vec"): (24, 128, 344, 1032, 2048),
    ("bf16", "scalar"): (3, 7, 73, 150, 255),
}
EDGE_F = {
    ("fp32", "vec"): (12, 20, 36, 68, 172, 600),
    ("fp32", "scalar"): (3, 7, 13, 29, 50, 150),
    ("bf16", "vec"): (24, 40, 72, 136, 344, 1032),
    ("bf16", "scalar"): (3, 7, 13, 29, 50, 150),
}
COPY_F = {
    ("fp32", "vec"): (12, 20, 36, 68, 172, 600),
    ("fp32", "vec2"): (6, 10, 18, 34, 86, 150),
    ("fp32", "scalar"): (3, 7, 13, 29, 51, 151),
    ("bf16", "vec"): (24, 40, 72, 136, 344, 1032),
    ("bf16", "vec2"): (6, 10, 18, 34, 86, 150),
    ("bf16", "scalar"): (3, 7, 13, 29, 51, 151),
}
ACC_F = (12, 20, 36, 68, 172, 600, 3, 7, 13, 29, 34)  # accumulate: VEC 4 | VEC 1 (34: 4 fails)
MASKED_F = (7, 64, 150)  # masked_gather_rows has one instantiation per type: VEC 1, LPR 16
LPRS = (4, 8, 16, 32, 64)
LN_PAIRS = ((4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4), (64, 8))


def widths(table, dt):
    return [(F, path) for (t, path), fs in table.items() if t == dt for F in fs]


def reached(kind: str):
    """{instantiation: [widths]} of a table under its mirror, keyed like the templates."""
    out: dict = {}
    table = dict(ln=LN_F, bn=BN_F, act=ACT_F, edge=EDGE_F, copy=COPY_F)[kind]
    for (dt, path), fs in table.items():
        for F in fs:
            e = ELEM[dt]
            if kind == "ln":
                key = (dt,) + ln_select(F, e)
            elif kind == "bn":
                key = (dt,) + bn_select(F, e)[:2]
            elif kind == "act":
                key = (dt, act_select(F, e))
            elif kind == "edge":
                key = (dt,) + edge_select(F, e)
            else:
                key = (dt,) + copy_select(F, e)
            out.setdefault(key, []).append(F)
            want = {"vec": 16 // e, "vec2": 2, "scalar": 1}[path]
            assert key[1] == want, (kind, dt, path, F, key)
    return out


def every_instantiation(kind: str):
    """What each launcher can select, written out from its switch / if chain. The remaining
    template parameters (RES, MODE, ACT, IdxT, BWD) do not depend on the width: the GPU tests
    run each of them at every width. ACC (copy_rows accumulate, fp32 only) has VEC 4 and 1:
    ``ACC_F`` holds a width for each of its (VEC, LPR)."""
    res = set()
    for dt, e in ELEM.items():
        for vec in (16 // e, 1):
            if kind == "ln":
                res |= {(dt, vec, l, c) for l, c in LN_PAIRS}
            elif kind == "bn":
                res |= {(dt, vec, l) for l in (8, 16, 32, 64)}
            elif kind == "act":
                res.add((dt, vec))
            elif kind == "edge":
                res |= {(dt, vec, l) for l in LPRS}
        if kind == "copy":
            res |= {(dt, vec, l) for vec in (16 // e, 2, 1) for l in LPRS}
    return res


def test_accumulate_widths_reach_every_instantiation():
    got = {copy_select(F, 4, acc=True) for F in ACC_F}
    assert got == {(v, l) for v in (4, 1) for l in LPRS}, sorted(got)


@pytest.mark.parametrize("kind", ["ln", "bn", "act", "edge", "copy"])
def test_tables_reach_every_instantiation(kind):
    got, want = reached(kind), every_instantiation(kind)
    for key in sorted(want, key=str):
        print(f"{kind} {key}: F = {got.get(key)}")
    assert set(got) == want, (sorted(want - set(got), key=str), sorted(set(got) - want, key=str))
    assert len(want) == dict(ln=32, bn=16, act=4, edge=20, copy=30)[kind]


def test_tables_cover_the_edges_the_kernels_have():
    for (dt, path), fs in LN_F.items():
        assert all(ln_shape_ok(F, ELEM[dt]) for F in fs)
    for dt in ELEM:
        e, V = ELEM[dt], 16 // ELEM[dt]
        for lim, past in zip(LN_LIMIT[dt], LN_PAST[dt]):
            # ``lim``: the widest width of the path; ``past``: the next one of the same path
            assert ln_shape_ok(lim, e) and not ln_shape_ok(past, e)
            same = [F for F in range(1, past + 1) if (F % V == 0) == (lim % V == 0)]
            assert past in same and all(ln_shape_ok(F, e) == (F <= lim) for F in same)
        # a partly empty last chunk or lane group in most widths
        part = [F for F, _ in widths(LN_F, dt)
                if (-(-F // ln_select(F, e)[0])) % ln_select(F, e)[1] != 0]
        assert len(part) >= 12
        # BatchNorm: a vector and a scalar width above one column tile
        tiles = {path: max(bn_select(F, e)[2] for F in BN_F[(dt, path)])
                 for path in ("vec", "scalar")}
        assert tiles["vec"] >= 3 and tiles["scalar"] >= 5
        # bias_act: vector widths above 256 up to the limit, and the widths past it
        assert max(ACT_F[(dt, "vec")]) == 256 * V and act_select(256 * V + V, e) is None
        assert act_select(257, e) is None and act_select(256 * V, e, aligned=False) is None
        assert act_select(256, e, lds=(257,)) == 1 and act_select(255, e) == 1
        # edge kernels: a width of several passes of LPR * VEC columns
        assert max(EDGE_F[(dt, "vec")]) > 2 * 64 * V and max(EDGE_F[(dt, "scalar")]) > 2 * 64
    # strides and alignment move a vector width to the scalar instantiation
    assert bn_select(68, 4, lds=(77,))[0] == 1 and bn_select(68, 4, aligned=False)[0] == 1
    assert bn_select(68, 4, lds=(80, 72))[0] == 4
    assert edge_select(36, 4, lds=(37,)) == (1, 64) and edge_select(36, 4, lds=(40,)) == (4, 16)
    assert copy_select(36, 4, lds=(38,)) == (2, 32) and copy_select(36, 4, align=4) == (1, 64)
    assert copy_select(36, 4, acc=True) == (4, 16) and copy_select(34, 4, acc=True) == (1, 64)
    assert copy_select(50, 4, align=4) == (1, 64) and copy_select(50, 2, align=2) == (1, 64)


# ------------------------------------------------------------------- many-rows cases
def many_rows(kind: str) -> int:
    """Rows (edges) past which a wave of the narrowest instantiation takes a second
    grid-stride step, from the launchers' grid caps (``cap_blocks(..., cap)``; blocks of 4
    waves), plus 4,099."""
    if kind == "ln":  # ln_fwd: cap 256 * 32 blocks of 4 G rows, G = 1 at LPR 64
        return 256 * 32 * 4 * (64 // ln_select(50, 4)[1]) + EXTRA
    if kind == "bn":  # bn_apply: cap 256 * 16 blocks of RB = 4 * (64 / LPR) rows
        return 256 * 16 * 4 * (64 // bn_select(50, 4)[1]) + 1031
    if kind == "act":  # fwd_vec: cap 256 * 8 blocks of rpi = 256 / (F / VEC) rows
        return 256 * 8 * (256 // (1024 // act_select(1024, 4))) + 77
    if kind == "pair":  # launch_pair: cap 256 * 64 blocks, one wave per row
        return 256 * 64 * 4 + EXTRA
    if kind == "gaa":  # launch_gaa: cap 256 * 64 blocks of 4 G edges
        return 256 * 64 * 4 * (64 // edge_select(50, 4)[1]) + EXTRA
    if kind == "copy":  # copy_launch: cap 256 * 32 blocks of 4 G U rows, U = 4
        return 256 * 32 * 4 * (64 // copy_select(50, 4, align=4)[1]) * 4 + EXTRA
    raise KeyError(kind)


def test_many_rows_counts():
    assert many_rows("ln") == 32768 + 4099 and ln_select(50, 4)[1] == 64
    assert many_rows("bn") == 16384 + 1031 and bn_select(50, 4)[1] == 64
    assert many_rows("act") == 2048 + 77 and act_select(1024, 4) == 4
    assert many_rows("pair") == 65536 + 4099
    assert many_rows("gaa") == 65536 + 4099 and edge_select(50, 4) == (1, 64)
    assert many_rows("copy") == 131072 + 4099


def test_ladder_has_every_boundary_degree():
    """Degrees G - 1, G, G + 1, 4G - 1, 4G, 4G + 1 of pair_relu's four-in-flight loop and
    single-step tail, for the G = 64 / LPR of every LPR."""
    deg = set(ladder_csr().degree().tolist())
    for lpr in LPRS:
        G = 64 // lpr
        assert {G - 1, G, G + 1, 4 * G - 1, 4 * G, 4 * G + 1, 8 * G + 1} <= deg, lpr
    assert 0 in deg and 1027 in deg


@functools.lru_cache(maxsize=None)
def many_pattern(n: int, nsrc: int = 257, seed: int = 3):
    """(rowptr, col) of ``n`` rows of degree ``r % 4`` over ``nsrc`` sources."""
    g = torch.Generator().manual_seed(seed)
    rowptr = torch.zeros(n + 1, dtype=torch.long)
    rowptr[1:] = torch.cumsum(torch.arange(n) % 4, 0)
    return rowptr, torch.randint(0, nsrc, (int(rowptr[-1]),), generator=g)


# -------------------------------------------------------------------------- inputs
def rnd(shape, seed, dt="fp32", kind="plain"):
    """fp32 values a tensor of type ``dt`` holds exactly. ``plain``: ``randn * 3 + 1``;
    ``big``: ``1000 + 0.1 randn`` (bf16: ``1000 + 4 k``, |k| <= 6, a spacing bf16 has)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "plain":
        x = torch.randn(shape, generator=g) * 3 + 1
    elif dt == "bf16":
        x = 1000 + 4 * (torch.randn(shape, generator=g) * 2).round().clamp(-6, 6)
    else:
        x = 1000 + 0.1 * torch.randn(shape, generator=g)
    return x.to(TORCH_DT[dt]).float()


def ints(shape, seed, lo=-3, hi=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def off_zero(x, pres, dt="fp32", margin=1e-3, step=0.5):
    """``x`` with the entries moved by ``step`` at which one of the pre-activations
    ``pre(x)`` (fp64) of ``pres`` lies within ``margin`` of 0: a ReLU gate of the random
    cases must not hang on the last bit of an fp32 rounding (the zero-gate cases test the
    gate itself, on exact integers). 1e-3 is far above any fp32 rounding of values of
    magnitude 10 and moves fewer than one entry in a thousand."""
    for _ in range(8):
        near = torch.zeros_like(x, dtype=torch.bool)
        for pre in pres:
            near |= pre(x.double()).abs() < margin
        if not bool(near.any()):
            return x
        x = torch.where(near, x + step, x).to(TORCH_DT[dt]).float()
    raise AssertionError("pre-activations still near 0")


def test_off_zero():
    x = torch.tensor([[0.0, 1.0, -2.0, 2.0005]])
    y = off_zero(x, [lambda v: v, lambda v: v - 2.0])
    assert torch.equal(y, torch.tensor([[0.5, 1.0, -2.0, 2.5005]]))


# ----------------------------------------------------------------------- contracts
def _opt(t, dtype):
    return None if t is None else t.to(dtype)


def ln_fwd_contract(x, gamma, beta, res, eps=EPS, dtype=torch.float64):
    """(y, mean, rstd): two-pass mean / variance over a row, ``y = xhat g + b + res``.
    The mean is ``sum * (1 / F)`` as the kernel writes it (in fp64 the same number)."""
    x = x.to(dtype)
    invF = torch.tensor(1.0, dtype=dtype) / x.shape[1]
    mean = x.sum(1, keepdim=True) * invF
    d = x - mean
    rstd = torch.rsqrt((d * d).sum(1, keepdim=True) * invF + eps)
    y = d * rstd
    if gamma is not None:
        y = y * gamma.to(dtype) + beta.to(dtype)
    if res is not None:
        y = y + res.to(dtype)
    return y, mean[:, 0], rstd[:, 0]


def ln_bwd_contract(dy, x, mean, rstd, gamma, dtype=torch.float64):
    """(dx, dgamma, dbeta) from the saved per-row ``mean`` / ``rstd``."""
    dy, x = dy.to(dtype), x.to(dtype)
    rs = rstd.to(dtype).unsqueeze(1)
    xh = (x - mean.to(dtype).unsqueeze(1)) * rs
    d = dy if gamma is None else dy * gamma.to(dtype)
    m1, m2 = d.mean(1, keepdim=True), (d * xh).mean(1, keepdim=True)
    return rs * (d - m1 - xh * m2), (dy * xh).sum(0), dy.sum(0)


def keep_scale(keep, p, dtype):
    """None, or the keep mask times 1 / (1 - p)."""
    return None if keep is None else keep.to(dtype) / (1.0 - p)


def bn_stats_contract(x, center, dtype=torch.float64):
    """bn_reduce mode 0: [sum (x - center), sum (x - center)^2] over the rows."""
    d = x.to(dtype) - center.to(dtype)
    return torch.stack([d.sum(0), (d * d).sum(0)])


def _bn_pre(x, mean, rstd, g, b, dtype):
    xh = (x.to(dtype) - mean.to(dtype)) * rstd.to(dtype)
    pre = xh
    if g is not None:
        pre = pre * g.to(dtype)
    if b is not None:
        pre = pre + b.to(dtype)
    return xh, pre


def bn_fwd_contract(x, mean, rstd, g, b, relu, keep=None, p=0.0, dtype=torch.float64):
    """bn_apply mode 0: ``drop(act((x - mean) rstd g + b))``."""
    _, y = _bn_pre(x, mean, rstd, g, b, dtype)
    if relu:
        y = y.clamp_min(0)
    return y if keep is None else y * keep_scale(keep, p, dtype)


def _bn_dy(x, dy, mean, rstd, g, b, relu, keep, p, dtype):
    xh, pre = _bn_pre(x, mean, rstd, g, b, dtype)
    d = dy.to(dtype)
    if keep is not None:
        d = d * keep_scale(keep, p, dtype)
    if relu:
        d = d * (pre > 0)
    return xh, d


def bn_bwd_reduce_contract(x, dy, mean, rstd, g, b, relu, keep=None, p=0.0,
                           dtype=torch.float64):
    """bn_reduce mode 1: [sum dy', sum dy' xhat], dy' = dy keep / (1 - p) [pre > 0]."""
    xh, d = _bn_dy(x, dy, mean, rstd, g, b, relu, keep, p, dtype)
    return torch.stack([d.sum(0), (d * xh).sum(0)])


def bn_bwd_apply_contract(x, dy, mean, rstd, g, b, c1, c2, relu, keep=None, p=0.0,
                          dtype=torch.float64):
    """bn_apply mode 1: ``dx = (dy' - c1 - xhat c2) rstd g``."""
    xh, d = _bn_dy(x, dy, mean, rstd, g, b, relu, keep, p, dtype)
    if c1 is not None:
        d = d - c1.to(dtype)
    if c2 is not None:
        d = d - xh * c2.to(dtype)
    d = d * rstd.to(dtype)
    return d if g is None else d * g.to(dtype)


def act_value(t, act: str):
    if act == "relu":
        return t.clamp_min(0)
    if act == "silu":
        return t * torch.sigmoid(t)
    if act == "leaky":
        return torch.where(t > 0, t, 0.2 * t)
    return t


def act_slope(t, act: str):
    if act == "relu":
        return (t > 0).to(t.dtype)
    if act == "silu":
        s = torch.sigmoid(t)
        return s * (1 + t * (1 - s))
    if act == "leaky":
        return torch.where(t > 0, torch.ones_like(t), torch.full_like(t, 0.2))
    return torch.ones_like(t)


BIAS_ACTS = {0: "none", 1: "silu", 2: "relu"}  # act.hip
EDGE_ACTS = {0: "none", 1: "relu", 2: "silu", 3: "leaky"}  # edge_fused.hip


def bias_act_contract(z, b, act: int, dy=None, dtype=torch.float64):
    """Forward ``act(z + b)``; with ``dy``: ``dz = dy act'(z + b)``. The bias gradient is
    the column sum of the STORED dz (:func:`colsum_contract`)."""
    t = z.to(dtype) if b is None else z.to(dtype) + b.to(dtype)
    if dy is None:
        return act_value(t, BIAS_ACTS[act])
    return dy.to(dtype) * act_slope(t, BIAS_ACTS[act])


def colsum_contract(stored, dtype=torch.float64):
    return stored.to(dtype).sum(0)


def _rows_of(rowptr):
    n = rowptr.numel() - 1
    return torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1])


def pair_relu_contract(rowptr, col, mode: int, rowterm, gat, gat2=None, rowmul=None,
                       dtype=torch.float64):
    """mode 0: ``sum_c relu(R[r] + X[c])``; 1: ``M[r] #{c: R[r] + X[c] > 0}``;
    2: ``sum_c X2[c] [R[r] + X[c] > 0]`` -- per row, entries in CSR order."""
    rows, col = _rows_of(rowptr), col.long()
    n, F = rowptr.numel() - 1, gat.shape[1]
    pre = rowterm.to(dtype)[rows] + gat.to(dtype)[col]
    if mode == 0:
        term = pre.clamp_min(0)
    elif mode == 1:
        term = (pre > 0).to(dtype)
    else:
        term = gat2.to(dtype)[col] * (pre > 0)
    out = torch.zeros(n, F, dtype=dtype).index_add_(0, rows, term)
    return out * rowmul.to(dtype)[:n] if mode == 1 else out


def gaa_contract(E, F, Y, P, src, Q, dst, act: int, gin=None, dtype=torch.float64):
    """``act(Y[e] + P[src[e]] + Q[dst[e]])`` (absent terms are 0); with ``gin``:
    ``gin[e] act'(same)``. Summed in the kernel's order: Y, then P, then Q."""
    t = torch.zeros(E, F, dtype=dtype)
    if Y is not None:
        t = t + Y.to(dtype)[:E]
    if P is not None:
        t = t + P.to(dtype)[src[:E]]
    if Q is not None:
        t = t + Q.to(dtype)[dst[:E]]
    if gin is None:
        return act_value(t, EDGE_ACTS[act])
    return gin.to(dtype)[:E] * act_slope(t, EDGE_ACTS[act])


def copy_rows_contract(x, src, dst, out, accumulate=False):
    """``out[dst[i]] (+)= x[src[i]]`` on a copy of ``out``: a negative source moves zeros,
    a negative destination skips. Without ``accumulate`` the destinations of one call are
    distinct (the callers' contract), so order does not matter."""
    n = (src if src is not None else dst).numel() if (src is not None or dst is not None) \
        else x.shape[0]
    s = torch.arange(n) if src is None else src.long()
    d = torch.arange(n) if dst is None else dst.long()
    vals = torch.where((s >= 0).unsqueeze(1), x[s.clamp(min=0)], torch.zeros_like(x[:1]))
    live = d >= 0
    res = out.clone()
    if accumulate:
        return res.index_add_(0, d[live], vals[live])
    res[d[live]] = vals[live]
    return res


def masked_gather_contract(x, idx, mask, value, out):
    res = out.clone()
    sel = mask == value
    res[:idx.numel()][sel] = x[idx[sel]]
    return res


def allowance(ref64, ref32, dt: str, roundings: int = 1):
    """The project's rule: ``|kernel - fp64| <= bound(ref64, ref32)``
    (tests/test_gat_kernels.py), and a bf16 output adds ``2^-8 |v|`` per rounding
    (tests/test_spmm_generic_cases.py). fp32 outputs of a bf16 kernel have no rounding:
    pass ``dt = "fp32"`` for them."""
    lim = torch.full_like(ref64.double(), bound(ref64, ref32))
    return lim + roundings * BF16_ULP * ref64.double().abs() if dt == "bf16" else lim


# ------------------------------------------------------- contracts against autograd
@pytest.mark.parametrize("F,affine,res", [(12, True, True), (73, True, False),
                                          (50, False, True), (7, False, False)])
def test_ln_contract_matches_autograd(F, affine, res):
    N = 23
    x = rnd((N, F), 1).double().requires_grad_()
    g = rnd((F,), 2).double().requires_grad_() if affine else None
    b = rnd((F,), 3).double().requires_grad_() if affine else None
    r = rnd((N, F), 4).double() if res else None
    dy = rnd((N, F), 5).double()
    want = torch.nn.functional.layer_norm(x, (F,), g, b, EPS)
    want = want + r if res else want
    y, mean, rstd = ln_fwd_contract(x.detach(), g, b, r)
    assert torch.allclose(y, want.detach(), rtol=1e-12, atol=1e-12)
    want.backward(dy)
    dx, dg, db = ln_bwd_contract(dy, x.detach(), mean, rstd, None if g is None else g.detach())
    assert torch.allclose(dx, x.grad, rtol=1e-10, atol=1e-10)
    if affine:
        assert torch.allclose(dg, g.grad, rtol=1e-10, atol=1e-10)
        assert torch.allclose(db, b.grad, rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("F,affine,relu", [(12, True, True), (29, True, False),
                                           (7, False, True)])
def test_bn_contracts_match_autograd(F, affine, relu):
    """The four passes chained as models/norm.py chains them equal torch's batch_norm (+
    relu) and its autograd in fp64. The tolerances of these CPU pins compare fp64 with fp64
    and only tell a wrong formula (errors of order 1) from rounding (1e-16 per operation):
    1e-12 for single formulas as in tests/test_segment_cases.py, 1e-10 / 1e-9 where rstd
    (about 1 / 3) to the third power, sums over the rows and the chain of four passes
    multiply the roundings, still seven orders below any formula error."""
    N = 37
    x = rnd((N, F), 6).double().requires_grad_()
    g = rnd((F,), 7).double().requires_grad_() if affine else None
    b = rnd((F,), 8).double().requires_grad_() if affine else None
    dy = rnd((N, F), 9).double()
    want = torch.nn.functional.batch_norm(x, None, None, g, b, True, 0.0, EPS)
    want = torch.relu(want) if relu else want
    xd = x.detach()
    s = bn_stats_contract(xd, xd[0])
    m1 = s[0] / N
    mean, rstd = xd[0] + m1, torch.rsqrt(s[1] / N - m1 * m1 + EPS)
    gd, bd = (None, None) if g is None else (g.detach(), b.detach())
    y = bn_fwd_contract(xd, mean, rstd, gd, bd, relu)
    assert torch.allclose(y, want.detach(), rtol=1e-10, atol=1e-10)
    want.backward(dy)
    r = bn_bwd_reduce_contract(xd, dy, mean, rstd, gd, bd, relu)
    dx = bn_bwd_apply_contract(xd, dy, mean, rstd, gd, bd, r[0] / N, r[1] / N, relu)
    assert torch.allclose(dx, x.grad, rtol=1e-9, atol=1e-9)
    if affine:
        assert torch.allclose(r[1], g.grad, rtol=1e-9, atol=1e-9)
        assert torch.allclose(r[0], b.grad, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_activation_contracts_match_autograd(act):
    t = rnd((11, 13), 10).double().requires_grad_()
    name = EDGE_ACTS[act]
    want = {"none": lambda v: v, "relu": torch.relu, "silu": torch.nn.functional.silu,
            "leaky": lambda v: torch.nn.functional.leaky_relu(v, 0.2)}[name](t)
    assert torch.allclose(act_value(t.detach(), name), want.detach(), rtol=1e-12, atol=1e-12)
    want.sum().backward()
    assert torch.allclose(act_slope(t.detach(), name), t.grad, rtol=1e-12, atol=1e-12)


def test_pair_relu_contract_matches_autograd():
    """Modes 1 and 2 are the adjoints of mode 0 with respect to P and Q."""
    csr = ladder_csr()
    rowptr, col = csr.rowptr, csr.col.long()
    n, F = csr.num_rows, 5
    P = rnd((n, F), 11).double().requires_grad_()
    Q = rnd((csr.num_cols, F), 12).double().requires_grad_()
    g = rnd((n, F), 13).double()
    rows = _rows_of(rowptr)
    out = torch.zeros(n, F, dtype=torch.float64).index_add_(0, rows,
                                                           torch.relu(P[rows] + Q[col]))
    assert torch.allclose(pair_relu_contract(rowptr, col, 0, P.detach(), Q.detach()),
                          out.detach(), rtol=1e-12, atol=1e-12)
    out.backward(g)
    dP = pair_relu_contract(rowptr, col, 1, P.detach(), Q.detach(), rowmul=g)
    assert torch.allclose(dP, P.grad, rtol=1e-12, atol=1e-12)
    t = csr.transpose()
    dQ = pair_relu_contract(t.rowptr, t.col, 2, Q.detach(), P.detach(), gat2=g)
    assert torch.allclose(dQ, Q.grad, rtol=1e-12, atol=1e-12)


def test_copy_contracts():
    x = rnd((6, 3), 14)
    out = torch.full((5, 3), -1.0)
    src, dst = torch.tensor([4, -1, 2, 0]), torch.tensor([3, 1, -1, 0])
    r = copy_rows_contract(x, src, dst, out)
    assert torch.equal(r[3], x[4]) and torch.equal(r[1], torch.zeros(3))
    assert torch.equal(r[0], x[0]) and torch.equal(r[[2, 4]], out[[2, 4]])
    acc = copy_rows_contract(x, torch.tensor([1, 2, 3]), torch.tensor([0, 0, -1]), out, True)
    assert torch.equal(acc[0], out[0] + x[1] + x[2]) and torch.equal(acc[1:], out[1:])
    m = masked_gather_contract(x, torch.tensor([5, 4, 3]), torch.tensor([1, 0, 1]), 1, out)
    assert torch.equal(m[0], x[5]) and torch.equal(m[2], x[3]) and torch.equal(m[[1, 3, 4]],
                                                                               out[[1, 3, 4]])


# ------------------------------------------------------------------ zero-gate cases
def zero_gate_pair(csr, F, seed=20):
    """Integer ``P`` [rows, F], ``Q`` [sources, F], ``g`` in -3..3: ``P[i] + Q[j]`` is an
    exact small integer, 0 on about 1 / 7 of the (entry, feature) pairs."""
    return (ints((csr.num_rows, F), seed), ints((csr.num_cols, F), seed + 1),
            ints((max(csr.num_rows, csr.num_cols), F), seed + 2, 1, 3))


def zero_gate_count_pair(csr, P, Q):
    rows = _rows_of(csr.rowptr)
    return int(((P[rows] + Q[csr.col.long()]) == 0).sum())


def zero_gate_bias(N, F, seed=30):
    """Integer ``z`` [N, F], ``b`` [F], ``dy``: ``z + b`` is 0 where ``z == -b``."""
    return ints((N, F), seed), ints((F,), seed + 1), ints((N, F), seed + 2, 1, 3)


def zero_gate_bn(N, F, seed=40):
    """``x`` integers around an integer ``mean``, ``rstd = 0.5``, ``g = 2`` (or none with
    ``rstd = 1``), ``b`` integer: ``xhat g + b = (x - mean) + b`` exactly, 0 where
    ``x == mean - b``."""
    mean = ints((F,), seed, -2, 2)
    x = mean + ints((N, F), seed + 1)
    return dict(x=x, mean=mean, rstd=torch.full((F,), 0.5), g=torch.full((F,), 2.0),
                b=ints((F,), seed + 2, -1, 1), dy=ints((N, F), seed + 3, 1, 3),
                c1=ints((F,), seed + 4, -1, 1), c2=ints((F,), seed + 5, -1, 1))


def zero_gate_gaa(E, F, nP, nQ, seed=50):
    g = torch.Generator().manual_seed(seed)
    return dict(Y=ints((E, F), seed + 1), P=ints((nP, F), seed + 2), Q=ints((nQ, F), seed + 3),
                src=torch.randint(0, nP, (E,), generator=g),
                dst=torch.randint(0, nQ, (E,), generator=g), gin=ints((E, F), seed + 4, 1, 3))


def share_tol(p: float, n: int) -> float:
    """Four standard deviations of the share of hits among ``n`` independent draws that
    each hit with probability ``p``."""
    return 4.0 * math.sqrt(p * (1.0 - p) / n)


def test_zero_gate_cases_hold_exact_zeros():
    """Every construction has pre-activations that are EXACTLY 0, in fp32 and after a round
    trip through bf16, and the share the construction says (uniform integers: 1 / 7 for a
    difference of two draws from -3..3 is 7 / 49), within :func:`share_tol` of the number of
    independent draws (for pair_relu the entries of P: the entries of a row share them)."""
    csr = ladder_csr()
    P, Q, _ = zero_gate_pair(csr, 12)
    z = zero_gate_count_pair(csr, P, Q)
    total = csr.nnz * 12
    print(f"pair_relu: {z} of {total} pre-activations are 0")
    assert z >= 1 and abs(z / total - 1 / 7) < share_tol(1 / 7, P.numel())
    for t in (P, Q):
        assert torch.equal(t.bfloat16().float(), t)
    zz, b, _ = zero_gate_bias(203, 12)
    nz = int((zz + b == 0).sum())
    print(f"bias_act: {nz} of {zz.numel()}")
    assert nz >= 1 and abs(nz / zz.numel() - 1 / 7) < share_tol(1 / 7, zz.numel())
    c = zero_gate_bn(203, 12)
    pre32 = torch.addcmul(c["b"], (c["x"] - c["mean"]) * c["rstd"], c["g"])
    _, pre64 = _bn_pre(c["x"], c["mean"], c["rstd"], c["g"], c["b"], torch.float64)
    nb = int((pre64 == 0).sum())
    print(f"batchnorm: {nb} of {pre64.numel()}")
    assert nb >= 1 and torch.equal(pre32.double(), pre64)
    assert abs(nb / pre64.numel() - 1 / 7) < share_tol(1 / 7, pre64.numel())
    d = zero_gate_gaa(203, 12, 31, 17)
    pre = d["Y"] + d["P"][d["src"]] + d["Q"][d["dst"]]
    ng = int((pre == 0).sum())
    print(f"gather_add_act: {ng} of {pre.numel()}")
    # three draws from -3..3 sum to 0 in 37 of 343 ways
    assert ng >= 1 and abs(ng / pre.numel() - 37 / 343) < share_tol(37 / 343, pre.numel())
    for value in LN_CONST:
        assert torch.equal(ln_zero_gate(12, value)[5], torch.full((12,), value))


LN_CONST = (3.0, 1000.0)  # one tensor each: the bound is one number per tensor


def ln_zero_gate(F, value=3.0, N=11, seed=60):
    """LayerNorm input whose row 5 is constant (``value``): variance 0, ``y = beta (+ res)``,
    ``rstd = eps^-1/2``. At 1000 a mean that is off by half an fp32 ulp (3e-5) moves y by
    0.01 gamma: that row tells a kernel that subtracts an unrounded ``sum * (1 / F)`` from
    one that subtracts the mean it stores, at the widths where the rounded product is 1000
    itself. The two values are separate inputs, so that the fp32 contract's own error on
    the row of 1000s does not widen the bound of the row of 3s."""
    x = rnd((N, F), seed)
    x[5] = value
    return x


def test_constant_row_contract():
    F = 12
    g, b = rnd((F,), 61), rnd((F,), 62)
    y, mean, rstd = ln_fwd_contract(ln_zero_gate(F), g, b, None)
    assert torch.equal(y[5], b.double()) and float(mean[5]) == 3.0
    # fp64 against fp64: 1e-9 is far above the 1e-13 a rounding of 12000 * (1 / 12) leaves
    assert abs(float(rstd[5]) - EPS ** -0.5) < 1e-9
    x = ln_zero_gate(F, 1000.0)
    y, _, _ = ln_fwd_contract(x, g, b, None)
    assert torch.allclose(y[5], b.double(), rtol=0, atol=1e-9) and torch.equal(
        x[5].bfloat16().float(), x[5])


COUNT_DEG = (771, 263, 5)  # pair_relu mode 1: counts a bf16 cannot hold (771 -> 772, 263 -> 264)


def count_case(F):
    """Rows of degree 771, 263 and 5 whose every pre-activation is 1 (``P = 0, Q = 1``): the
    count is the degree, and ``rowmul`` runs over 1..7, so ``out = bf16(deg m)`` exactly
    ONCE rounded; a count rounded to bf16 before the multiply gives another number."""
    rowptr = torch.zeros(len(COUNT_DEG) + 1, dtype=torch.long)
    rowptr[1:] = torch.cumsum(torch.tensor(COUNT_DEG), 0)
    col = torch.arange(int(rowptr[-1])) % 9
    m = (torch.arange(F) % 7 + 1).float().repeat(len(COUNT_DEG), 1)
    return rowptr, col, torch.zeros(len(COUNT_DEG), F), torch.ones(9, F), m


def test_count_case_tells_a_rounded_count():
    _, _, _, _, m = count_case(12)
    deg = torch.tensor(COUNT_DEG).float().unsqueeze(1)
    once = (deg * m).bfloat16()
    twice = (deg.bfloat16().float() * m).bfloat16()
    assert max(COUNT_DEG) > 256 and not torch.equal(deg.bfloat16().float(), deg)
    assert int((once != twice).sum()) >= 1


# --------------------------------------------------------------------- dropout gap
M32 = 0xFFFFFFFF


def fmix32(h: int) -> int:
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def _unshift(h: int, s: int) -> int:
    """Inverse of ``h ^= h >> s`` on 32 bits."""
    x = h
    for _ in range(32 // s + 1):
        x = h ^ (x >> s)
    return x


def inverse_fmix32(h: int) -> int:
    h = _unshift(h, 16)
    h = (h * pow(0xC2B2AE35, -1, 1 << 32)) & M32
    h = _unshift(h, 13)
    h = (h * pow(0x85EBCA6B, -1, 1 << 32)) & M32
    return _unshift(h, 16)


def seed_for_hash(idx: int, h: int) -> int:
    """A seed (below 2^32, so its high word adds nothing) under which element ``idx`` of a
    tensor (``idx = r F + c < 2^32``) hashes to ``h`` in ``dropout_keep``."""
    assert 0 <= idx < (1 << 32)
    return inverse_fmix32(h) ^ idx


def f32(p: float) -> float:
    return float(torch.tensor(p, dtype=torch.float32))


def kernel_threshold(p: float) -> int:
    """``set_dropout`` of batchnorm.hip on the value the binding passes:
    ``static_cast<float>(drop_p)``, then ``floor(double(p32) * 2^32)`` clamped."""
    p32 = f32(p)
    if not 0.0 < p32 < 1.0:
        return 0
    t = p32 * 4294967296.0
    return 4294967295 if t >= 4294967295.0 else int(max(t, 1.0))


GAP_P = (0.05, 0.1, 0.2, 0.3)
GAP_SHAPE, GAP_ELEM = (8, 24), (5, 7)


def gap_cases():
    """(p, seed, hash, kernel keeps) for the two edges of the gap between the threshold of
    the Python double and that of the fp32 the kernels receive."""
    idx = GAP_ELEM[0] * GAP_SHAPE[1] + GAP_ELEM[1]
    res = []
    for p in GAP_P:
        lo, hi = int(p * 4294967296.0), int(f32(p) * 4294967296.0) - 1
        assert lo <= hi, p  # float32(p) > p at these p: a gap of hi - lo + 1 hashes
        for h in (lo, hi):
            res.append((p, seed_for_hash(idx, h), h, h >= kernel_threshold(p)))
    return res


def test_fmix32_inverse():
    g = torch.Generator().manual_seed(70)
    for h in [0, 1, M32, 429496730] + torch.randint(0, 1 << 32, (200,), generator=g).tolist():
        assert fmix32(inverse_fmix32(h)) == h and inverse_fmix32(fmix32(h)) == h
    # the element the defect was shown on: seed 448867595, p = 0.1, (5, 7) of [8, 24]
    assert fmix32(127 ^ 448867595) == 429496730
    assert seed_for_hash(127, 429496730) == 448867595


def test_thresholds_table():
    want = {0.1: (429496736, 429496729), 0.2: (858993472, 858993459),
            0.3: (1288490240, 1288490188), 0.05: (214748368, 214748364)}
    for p, (kern, dbl) in want.items():
        assert kernel_threshold(p) == kern and int(p * 4294967296.0) == dbl
    for p in (0.25, 0.5):
        assert kernel_threshold(p) == int(p * 4294967296.0)
    assert kernel_threshold(0.0) == 0 and kernel_threshold(1.0) == 0


@pytest.mark.parametrize("p,seed,h,kernel_keeps", gap_cases())
def test_gap_elements_are_treated_alike(p, seed, h, kernel_keeps):
    """An element whose hash lies between the two thresholds gets ONE answer from the CPU
    mask and from the kernels' rule ``h >= thresh``."""
    N, F = GAP_SHAPE
    r, c = GAP_ELEM
    mask = dropout_keep_mask(seed, N, F, "cpu", p)
    assert fmix32((r * F + c) ^ seed) == h
    assert bool(mask[r, c]) == kernel_keeps, (p, h, kernel_threshold(p))


@pytest.mark.parametrize("p", GAP_P + (0.25, 0.5, 0.9))
def test_mask_equals_the_kernel_rule_everywhere(p):
    N, F, seed = 64, 50, (7 << 32) + 12345
    idx = torch.arange(N * F)
    hi_mix = ((0 + (seed >> 32)) * 0x9E3779B1) & M32
    h = torch.tensor([fmix32(int(i) ^ (seed & M32) ^ hi_mix) for i in idx])
    assert torch.equal(dropout_keep_mask(seed, N, F, "cpu", p).reshape(-1),
                       h >= kernel_threshold(p))


# --------------------------------------------------------------- CPU sanity of bounds
def test_allowance_rule():
    r64 = torch.tensor([1.0, -300.0], dtype=torch.float64)
    r32 = r64.float()
    assert torch.equal(allowance(r64, r32, "fp32"), torch.full((2,), 2e-5 * 300, dtype=torch.float64))
    a = allowance(r64, r32, "bf16", 2)
    assert math.isclose(float(a[1]), 2e-5 * 300 + 2 * 300 / 256)
