"""Inputs and oracles of tests/test_dense_epilogue_variants_gpu.py -- the edge softmax over
CSR rows (csrc/kernels/edge_softmax.hip, 7 instantiations by lanes per edge) and the bf16
path's elementwise epilogues (``bias_relu_pack``, ``relu_mask_bwd``, ``col_sum_partial`` in
csrc/kernels/elementwise.hip) -- with the launchers' rules restated by hand, and the CPU
tests that pin them down.

* Edge softmax: :func:`softmax_contract` is the contract of kernels.h per row and head in a
  given precision, ``-inf`` scores included (their weight is 0; a row of nothing else is
  all 0). :func:`softmax_pattern` has, per lanes-per-edge width, rows of degree 0, 1,
  ``EPW - 1``, ``EPW``, ``EPW + 1``, ``2 EPW + 3`` and a 301-entry hub, and entries before
  the first and after the last row that belong to no row and must keep a sentinel.
  The bound is ``test_gat_kernels.bound`` of the fp64 and fp32 evaluations.
* ``bias_relu_pack`` / ``relu_mask_bwd``: :func:`pack_inputs` keeps every ``y + bias`` at
  least 0.1 from 0, so every keep bit is decided (the cap on uncompared bits is zero);
  :func:`pack_words` restates the mask layout (512-element chunks, word ``j`` bit ``l`` =
  element ``8 l + j``) and is checked against ``reference._mask_to_words``.
* ``col_sum``: :func:`col_sum_plan` restates the partition of ``col_sum_op`` /
  ``col_sum_partial`` (vector width incl. the 16-byte base rule, rows per block and per
  iteration); the allowance per column is ``D 2^-24 sum|x|`` with ``D`` the longest chain of
  additions, ``ceil(rpb / rpi) + rpi + nblocks``.
"""
from __future__ import annotations

import functools

import pytest
import torch

from dgraph_amd.ops import reference as R

SENT = -12345.0
# ------------------------------------------------------------------------------ edge softmax
HEADS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)
SCORES = ("small", "large", "offset")  # scale 0.5, scale 40, scale 0.5 + 80
FRONT, BACK = 3, 5                      # entries of no row around the pattern
MANY_ROWS = 40000                       # more rows than the grid has waves (256 * 32 * 4)
MANY_HEADS = (1, 3, 17, 64)


def lpe_for(H: int) -> int:
    """``lpe_for``: lanes per edge, the next power of two."""
    l = 1
    while l < H:
        l <<= 1
    return l


def softmax_degrees(H: int):
    epw = 64 // lpe_for(H)
    return [0, 1, epw - 1, epw, epw + 1, 2 * epw + 3, 0, 301, 2, 0] * 2 + [0]


def softmax_pattern(H: int):
    """(rowptr, number of entries of the score array): the first row starts at ``FRONT``
    and ``BACK`` entries follow the last."""
    deg = torch.tensor([max(0, d) for d in softmax_degrees(H)])
    rowptr = torch.zeros(deg.numel() + 1, dtype=torch.long)
    rowptr[1:] = torch.cumsum(deg, 0)
    rowptr += FRONT
    return rowptr, int(rowptr[-1]) + BACK


def many_pattern():
    deg = torch.arange(MANY_ROWS) % 3
    rowptr = torch.zeros(MANY_ROWS + 1, dtype=torch.long)
    rowptr[1:] = torch.cumsum(deg, 0)
    return rowptr, int(rowptr[-1])


def _gen(*key) -> torch.Generator:
    seed = 0
    for k in key:
        for ch in str(k):
            seed = (seed * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def softmax_inputs(rowptr, E: int, H: int, kind: str, neg_inf: bool = False):
    """Scores and output gradient [E, H] in fp32. ``neg_inf``: the first non-empty row of
    each degree above 1 is all ``-inf``, the next one mixes ``-inf`` into finite scores."""
    g = _gen("softmax", E, H, kind)
    s = torch.randn(E, H, generator=g) * (40.0 if kind == "large" else 0.5)
    if kind == "offset":
        s += 80.0
    gr = torch.randn(E, H, generator=g)
    if neg_inf:
        seen = {}
        for r in range(rowptr.numel() - 1):
            b, e = int(rowptr[r]), int(rowptr[r + 1])
            n = seen.get(e - b, 0)
            seen[e - b] = n + 1
            if e - b < 1:
                continue
            if n == 0:
                s[b:e] = float("-inf")
            elif n == 1 and e - b > 1:
                s[b:e:2] = float("-inf")
                s[b + 1, 0] = float("-inf")  # head 0 of this row: one more
    return s, gr


def softmax_contract(rowptr, s, gr=None, alpha=None, dtype=torch.float64):
    """``alpha[j, h] = exp(s[j, h] - max_row) / sum_row exp(.)`` (0 for ``-inf`` scores and
    for a row of nothing else) over the entries of each row; with ``gr`` and ``alpha``
    instead the adjoint ``ds = alpha (g - sum_row alpha g)``. Entries of no row: NaN."""
    nr = rowptr.numel() - 1
    deg = rowptr[1:] - rowptr[:-1]
    rows = torch.repeat_interleave(torch.arange(nr), deg)
    idx = torch.arange(int(rowptr[0]), int(rowptr[-1]))
    if alpha is None:
        x = s.to(dtype)
        H = x.shape[1]
        out = torch.full_like(x, float("nan"))
        sv = x[idx]
        m = torch.full((nr, H), -float("inf"), dtype=dtype).index_reduce(
            0, rows, sv, "amax", include_self=True)
        m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
        ex = torch.exp(sv - m[rows])
        den = torch.zeros(nr, H, dtype=dtype).index_add_(0, rows, ex)
        out[idx] = torch.where(den[rows] > 0, ex / den[rows], torch.zeros_like(ex))
        return out
    a, g = alpha.to(dtype), gr.to(dtype)
    out = torch.full_like(a, float("nan"))
    dot = torch.zeros(nr, a.shape[1], dtype=dtype).index_add_(0, rows, a[idx] * g[idx])
    out[idx] = a[idx] * (g[idx] - dot[rows])
    return out


# ------------------------------------------------------------------------------ mask epilogues
PACK_SHAPES = [(1, 8), (9, 8), (33, 64), (777, 40), (63, 168), (64, 16384)]
PACK_BIG = (65600, 256)  # > 2048 blocks x 16 chunks x 512 elements: the grid-stride loop
WORD_FILL = 0x5A5A5A5A


def pack_blocks(numel: int) -> int:
    """Grid of ``bias_relu_pack`` / ``relu_mask_bwd``: 16 chunks per block, 2048 at most."""
    nch = (numel + 511) // 512
    return max(1, min(2048, (nch + 15) // 16))


def pack_inputs(shape, dtype, with_bias: bool, device="cpu"):
    """``y`` (odd multiples of 1/8 in [-4, 4], plus N(0, 1e-3) in fp32) and ``bias``
    (multiples of 1/4 in [-2, 2] plus N(0, 1e-3); fp32): ``|y + bias| >= 0.1`` always."""
    g = torch.Generator(device=device).manual_seed(sum(shape) + with_bias)
    L, F = shape
    y = (2 * torch.randint(-16, 16, (L, F), generator=g, device=device) + 1) / 8.0
    if dtype == torch.float32:
        y = y + torch.randn(L, F, generator=g, device=device) * 1e-3
    bias = None
    if with_bias:
        bias = torch.randint(-8, 9, (F,), generator=g, device=device) / 4.0 + \
            torch.randn(F, generator=g, device=device) * 1e-3
    return y.to(dtype), bias


def pack_oracle(y, bias, relu: bool):
    """fp64 ``t = y + bias``, the keep bits ``t > 0`` and the output."""
    t = y.double() if bias is None else y.double() + bias.double()
    keep = t > 0
    return t, keep, (torch.where(keep, t, torch.zeros_like(t)) if relu else t)


def pack_words(keep) -> torch.Tensor:
    """int32 words of a keep mask: per 512-element chunk eight 64-bit words (low half
    first), bit ``l`` of word ``j`` = element ``8 l + j``; elements past the end are 0."""
    flat = keep.reshape(-1)
    n = flat.numel()
    nch = (n + 511) // 512
    pad = torch.zeros(nch * 512, dtype=torch.int64, device=flat.device)
    pad[:n] = flat
    k = pad.view(nch, 2, 32, 8)                       # [chunk, half, lane, j]
    w = (k << torch.arange(32, device=flat.device).view(1, 1, 32, 1)).sum(2)  # [chunk, half, j]
    w = w.permute(0, 2, 1).reshape(-1)                # [chunk, j, half]
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


# ------------------------------------------------------------------------------ col_sum
COLSUM_F = {torch.float32: (1, 5, 8, 64, 73, 172, 256, 1024),
            torch.bfloat16: (1, 5, 8, 64, 73, 172, 256, 2048)}
COLSUM_L = (1, 255, 257, 1000, 262400)


def col_sum_plan(L: int, F: int, ld: int, dtype, base_aligned: bool = True):
    """(vec, nblocks, rows per block, rows per iteration, D) of ``col_sum``."""
    vec = 4 if dtype == torch.float32 else 8
    if F % vec or ld % vec or not base_aligned:
        vec = 1
    assert F // vec <= 256
    nb = max(1, min(1024, (L + 255) // 256))
    rpb = (L + nb - 1) // nb
    rpi = 256 // (F // vec)
    return vec, nb, rpb, rpi, (rpb + rpi - 1) // rpi + rpi + nb


# ------------------------------------------------------------------------------ CPU tests
def test_heads_cover_every_width():
    by = {}
    for H in HEADS:
        by.setdefault(lpe_for(H), []).append(H)
    assert sorted(by) == [1, 2, 4, 8, 16, 32, 64]
    for lpe, hs in by.items():
        assert lpe in hs                       # an exact head count
        assert lpe <= 2 or min(hs) < lpe       # and one that leaves lanes idle (none exists
    assert {lpe_for(H) for H in MANY_HEADS} >= {1, 4, 32, 64}  # below 3 lanes per edge)


@pytest.mark.parametrize("H", HEADS)
def test_softmax_pattern(H):
    rowptr, E = softmax_pattern(H)
    epw = 64 // lpe_for(H)
    deg = set((rowptr[1:] - rowptr[:-1]).tolist())
    assert {0, 1, epw, epw + 1, 2 * epw + 3, 301} <= deg and (epw == 1 or epw - 1 in deg)
    assert int(rowptr[0]) == FRONT and E == int(rowptr[-1]) + BACK
    assert (rowptr[1:] - rowptr[:-1])[-1] == 0  # the last row is empty


def test_many_pattern_outruns_the_grid():
    rowptr, E = many_pattern()
    assert MANY_ROWS > 256 * 32 * 4 and set((rowptr[1:] - rowptr[:-1]).tolist()) == {0, 1, 2}


@pytest.mark.parametrize("kind", SCORES)
def test_softmax_contract(kind):
    """Against ``torch.softmax`` and its autograd adjoint row by row; the ``-inf`` rules."""
    H = 3
    rowptr, E = softmax_pattern(H)
    s, gr = softmax_inputs(rowptr, E, H, kind)
    a = softmax_contract(rowptr, s)
    ds = softmax_contract(rowptr, None, gr, a)
    assert bool(torch.isnan(a[:FRONT]).all() and torch.isnan(a[-BACK:]).all())
    for r in range(rowptr.numel() - 1):
        b, e = int(rowptr[r]), int(rowptr[r + 1])
        if e == b:
            continue
        x = s[b:e].double().requires_grad_(True)
        y = torch.softmax(x, 0)
        torch.testing.assert_close(a[b:e], y.detach(), rtol=1e-12, atol=1e-15)
        (y * gr[b:e].double()).sum().backward()
        torch.testing.assert_close(ds[b:e], x.grad, rtol=1e-9, atol=1e-13)
    if kind == "large":  # without the max subtraction fp32 overflows
        assert bool(torch.isinf(torch.exp(s[FRONT:-BACK])).any())
    s2, _ = softmax_inputs(rowptr, E, H, kind, neg_inf=True)
    a2 = softmax_contract(rowptr, s2)
    body = a2[FRONT:-BACK]
    assert not bool(torch.isnan(body).any())
    assert bool((body[torch.isinf(s2[FRONT:-BACK])] == 0).all())
    nr = rowptr.numel() - 1
    rows = torch.repeat_interleave(torch.arange(nr), rowptr[1:] - rowptr[:-1])
    sums = torch.zeros(nr, H, dtype=torch.float64).index_add_(0, rows, body)
    dead = torch.full((nr, H), True).index_reduce(
        0, rows, torch.isinf(s2[FRONT:-BACK]), "amin", include_self=True) | \
        ((rowptr[1:] - rowptr[:-1]) == 0).unsqueeze(1)
    assert bool(dead.any() and (~dead).any())
    assert bool((sums[dead] == 0).all())
    torch.testing.assert_close(sums[~dead], torch.ones_like(sums[~dead]))
    # mixed rows exist: -inf next to finite scores
    assert bool(((sums > 0.5) & (torch.zeros(nr, H).index_add_(
        0, rows, torch.isinf(s2[FRONT:-BACK]).float()) > 0)).any())


def test_pack_words_layout():
    g = torch.Generator().manual_seed(3)
    for n in (8, 72, 512, 520, 31080):
        keep = torch.rand(n, generator=g) > 0.5
        w = pack_words(keep)
        assert w.numel() == (n + 511) // 512 * 16
        assert torch.equal(w, R._mask_to_words(keep))
        assert torch.equal(R._words_to_mask(w, n), keep)
        for i in (0, 7, n // 2, n - 1):   # the definition, bit by bit
            ch, l, j = i // 512, (i % 512) // 8, i % 8
            word = int(w[ch * 16 + 2 * j + (l >= 32)]) & 0xFFFFFFFF
            assert bool((word >> (l % 32)) & 1) == bool(keep[i])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pack_inputs_decide_every_bit(dtype):
    """No ``y + bias`` within a rounding of 0 (none within 0.1), both signs occur, the fp32
    evaluation has the fp64 keep bits, and bf16 outputs do get rounded."""
    for shape in PACK_SHAPES:
        for wb in (False, True):
            y, bias = pack_inputs(shape, dtype, wb)
            assert y.dtype == dtype
            t, keep, out = pack_oracle(y, bias, True)
            assert float(t.abs().min()) >= 0.1
            if y.numel() >= 72:
                assert bool(keep.any() and (~keep).any())
            t32 = y.float() if bias is None else y.float() + bias
            assert torch.equal(t32 > 0, keep)
            assert bool(((t32.double() - t).abs() <= 2.0 ** -24 * t.abs()).all())
            if dtype == torch.bfloat16 and wb:
                assert float((t.float().bfloat16().double() != t).double().mean()) > 0.5
    assert PACK_BIG[0] * PACK_BIG[1] > 2048 * 16 * 512
    assert pack_blocks(PACK_BIG[0] * PACK_BIG[1]) == 2048
    assert 16384 * 4 <= 64 * 1024 < 16392 * 4  # the LDS limit of the bias staging


def test_col_sum_plan():
    assert col_sum_plan(1000, 64, 64, torch.bfloat16)[0] == 8
    assert col_sum_plan(1000, 64, 64, torch.bfloat16, base_aligned=False)[0] == 1
    assert col_sum_plan(1000, 73, 73, torch.float32)[0] == 1
    assert col_sum_plan(1000, 8, 12, torch.bfloat16)[0] == 1
    vec, nb, rpb, rpi, D = col_sum_plan(262400, 2048, 2048, torch.bfloat16)
    assert (vec, nb, rpb, rpi) == (8, 1024, 257, 1) and D == 257 + 1 + 1024
    assert (nb - 1) * rpb > 262400             # the last block's rows start past L
    vec, nb, rpb, rpi, D = col_sum_plan(1000, 5, 5, torch.float32)
    assert (vec, nb, rpb, rpi) == (1, 4, 250, 51) and D == 5 + 51 + 4
    for dt, fs in COLSUM_F.items():
        for F in fs:
            for L in COLSUM_L:
                assert col_sum_plan(L, F, F, dt)[-1] >= 3
