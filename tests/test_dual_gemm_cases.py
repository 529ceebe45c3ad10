"""Inputs, oracle and case table of tests/test_dual_gemm_variants_gpu.py, which runs the two
bf16 dual-GEMM kernels (csrc/kernels/dual_gemm.hip, the column-half kernel
``dual_gemm_kernel<NT, NC1, NC2>``; csrc/kernels/dual_gemm_bs.hip, the B-stationary kernel
``dual_gemm_bs_kernel<NT, K, HC, HM, RELU>``) at every compiled instantiation, and the CPU
tests that pin all of it down first.

* Contract (kernels.h): ``v = A1 B1 (+ A2 B2) (+ bias) (+ cin)``, then the input keep mask
  (``v = 0`` where its bit is 0), then ReLU (``keep = v > 0``, written as a tile32 mask).
  :func:`product` and :func:`epilogue` evaluate it in fp64 from the bf16 inputs;
  ``epilogue`` is elementwise and runs wherever its operands live, so the GPU tests move
  the CPU product over once per shape and apply the eight flag combinations there.
* Exact data (:func:`make_inputs` ``"exact"``): A integers in [-2, 2], B multiples of 1/4
  in [-1, 1], bias multiples of 1/8 in [-2, 2) (odd ones on the columns of one sign, below;
  even ones elsewhere, so that exact zeros occur), cin multiples of 1/8 in [-2, 2].
  Every product is a multiple of 1/4 of magnitude <= 2 and every partial sum a multiple of
  1/8 below 2^11: at most 14 significant bits, exact in fp32 in any order. The output must
  be ``v.float().bfloat16()`` bitwise (one round-to-nearest-even) and every keep bit
  ``v > 0``. Zero-mean sums of this alphabet stay below 32, where every multiple of 1/8 is
  a bf16 number, so three rows in four hold non-negative entries and three columns in four
  entries of one sign: those elements are near +-K/2 and an odd multiple of 1/8 there is
  not a bf16 number, while the other rows and columns keep sums around 0 (both signs, and
  exact zeros) for the keep bits. :func:`unrepresentable` >= 1/4 is asserted per case.
* Full mantissa (``"full"``): A ~ N(0, 1), B ~ N(0, 1/K), bias and cin ~ N(0, 1). Per
  element (:func:`allowance`) ``2^-8 |out| + (K1 + K2 + 3) 2^-24 S`` with ``S`` the fp64
  sum of the absolute products plus ``|bias| + |cin|``: one bf16 rounding of the value
  that is stored, and fp32 accumulation of K1 + K2 + 2 terms in any order. A keep bit is
  compared where ``|v|`` exceeds the second term or the input mask already decided it
  (:func:`sure`); the rest may not exceed 0.5 % of a case (:data:`OMIT_CAP`).
* :data:`TABLE` and :func:`reach`: the launchers' dispatch restated by hand (``dual_gemm``'s
  choice between the kernels, ``by_nc1`` / ``by_nc2``, ``bs_by_k`` / ``bs_by_flags``), and
  ``ring_depth`` / ``BsCfg::NBUF`` restated for the cases that depend on the ring depth.
  They must be updated with the launchers; they check the table, not what a launch chose.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import pytest
import torch

from dgraph_amd.ops import reference as R

NS = (128, 192, 256)
K1S = (128, 192, 256)
K2S = (0, 128, 192, 256)
SHAPES = [(N, K1, K2) for N in NS for K1 in K1S for K2 in K2S]
FLAGS = [(c, m, r) for c in (0, 1) for m in (0, 1) for r in (0, 1)]  # (cin, mask_in, relu)
PRODUCTION = [(1, 0, 1), (0, 1, 0)]  # the SAGE forward and backward launches
M_TAIL = 289
SMALL_MS = (1, 31, 32, 33, 255, 256, 257)
OMIT_CAP = 0.005
FILL = 0x5A5A5A5A5A5A5A5A  # what mask_out holds before a call
SENT = float(torch.tensor(-12345.0).bfloat16())  # what out holds around a slice

Case = namedtuple("Case", "variant N K1 K2 cin mask_in relu")


def m_cus(cus: int) -> int:
    """Three or four 32-row tiles for every B-stationary block (one block per CU)."""
    return 32 * 3 * cus + 17


def m_long(cus: int) -> int:
    """Two turns of the deepest (8-slot) ring and two tiles more for every block."""
    return 32 * cus * (2 * 8 + 2) + 17


# ------------------------------------------------------------------ the dispatch, restated
def supported(N: int, K1: int, K2: int) -> bool:
    """``dual_gemm_supported``."""
    return N in (128, 192, 256) and K1 in (128, 192, 256) and K2 in (0, 128, 192, 256)


def bs_supported(N: int, K1: int, K2: int) -> bool:
    """``dual_gemm_bs_supported``."""
    return supported(N, K1, K2) and K1 + K2 in (192, 256, 512)


def reach(variant: int, N: int, K1: int, K2: int, cin, mask_in, relu):
    """The instantiation a call launches: ``("bs", NT, K, HC, HM, RELU)`` or
    ``("ch", NT, NC1, NC2)``."""
    if not supported(N, K1, K2):
        raise ValueError((N, K1, K2))
    NT = {128: 4, 192: 6, 256: 8}[N]               # switch (N) of dual_gemm / dual_gemm_bs
    if variant == 2 and bs_supported(N, K1, K2):   # dual_gemm
        K = {192: 192, 256: 256, 512: 512}[K1 + K2]  # bs_by_k
        return ("bs", NT, K, bool(cin), bool(mask_in), bool(relu))  # bs_by_flags
    nc1 = {4: 4, 6: 6, 8: 8}[K1 // 32]             # by_nc1
    nc2 = {0: 0, 4: 4, 6: 6, 8: 8}[K2 // 32]       # by_nc2
    return ("ch", NT, nc1, nc2)


def ring_depth(nc: int) -> int:
    """``ring_depth<NC>()`` of the column-half kernel (``DG_PD = 8``)."""
    if nc % 8 == 0 and nc >= 16:
        return 8
    if nc % 4 == 0 and nc >= 8:
        return 4
    if nc % 3 == 0 and nc >= 6:
        return 3
    return 2


def bs_nbuf(NT: int, K: int, cin, mask_in) -> int:
    """``BsCfg<NT, K, HC, HM>::NBUF``: the B-stationary kernel's LDS ring depth."""
    rpi = 2 if K <= 256 else 1
    a_bytes = 32 // rpi * 1040
    c_bytes = 64 * 32 * NT if cin else 0
    m_bytes = 128 * NT if mask_in else 0
    buf = (a_bytes + c_bytes + m_bytes + 15) // 16 * 16
    fixed = NT * 32 * 40 * 2 + 1024
    return min(8, (160 * 1024 - fixed) // buf)


# one shape per NT and per ring depth of the column-half kernel gets all eight flag
# combinations (its flags are run-time values); every other shape the two production ones
V1_ALL_FLAGS = {(128, 128, 0): 2, (192, 192, 0): 3, (256, 128, 128): 4, (128, 256, 256): 8,
                (192, 128, 128): 4, (256, 192, 0): 3}


def shape_runs(N: int, K1: int, K2: int):
    """[(variant, [flags])] of one shape."""
    runs = [(1, FLAGS if (N, K1, K2) in V1_ALL_FLAGS else PRODUCTION)]
    if bs_supported(N, K1, K2):
        runs.append((2, FLAGS))
    return runs


TABLE = [Case(v, N, K1, K2, *f) for (N, K1, K2) in SHAPES for v, fl in shape_runs(N, K1, K2)
         for f in fl]
# operand layouts, the small row counts: one shape per kernel family and NT
LAYOUT_SHAPES = {1: (192, 256), 2: (128, 128)}  # variant -> (K1, K2); K = 448 has no bs kernel
LAYOUTS = ("cols", "alias", "rows")


def long_cases():
    """One B-stationary case per distinct ring depth ``NBUF`` and one column-half case."""
    seen, out = set(), []
    for N in (256, 192, 128):
        for K1, K2 in ((256, 256), (128, 128), (192, 0)):
            for f in ((1, 1, 1), (1, 0, 1), (0, 1, 1), (0, 0, 1)):
                nb = bs_nbuf(N // 32, K1 + K2, f[0], f[1])
                if nb not in seen:
                    seen.add(nb)
                    out.append(Case(2, N, K1, K2, *f))
    out.append(Case(1, 256, 256, 256, 1, 1, 1))
    return out


# ------------------------------------------------------------------------------ inputs
def _gen(*key) -> torch.Generator:
    seed = 0
    for k in key:
        for ch in str(k):
            seed = (seed * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def make_inputs(N: int, K1: int, K2: int, M: int, data: str):
    """CPU operands of one shape: A1 [M, K1], B1t [N, K1], A2, B2t (None with K2 = 0) and cin
    [M, N] in bf16, bias [N] in fp32, keep_in [M, N] bool. The flags of a case choose which
    of cin and keep_in a call uses."""
    g = _gen(N, K1, K2, M, data)
    K = K1 + K2
    if data == "exact":
        prow = (torch.arange(M) % 4 != 3).unsqueeze(1)     # rows of non-negative entries
        A = torch.where(prow, torch.randint(0, 3, (M, K), generator=g),
                        torch.randint(-2, 3, (M, K), generator=g)).float()
        c = torch.arange(N)
        sign = torch.where(c % 4 == 0, 1, torch.where(c % 4 == 1, -1, torch.where(
            c % 4 == 2, 0, torch.where((c // 4) % 2 == 0, 1, -1))))
        Bt = torch.where((sign == 0).unsqueeze(1),
                         torch.randint(-4, 5, (N, K), generator=g),
                         sign.unsqueeze(1) * torch.randint(0, 5, (N, K), generator=g)) / 4.0
        bias = (2 * torch.randint(-8, 8, (N,), generator=g) + (sign != 0).long()) / 8.0
        cin = torch.randint(-16, 17, (M, N), generator=g) / 8.0
    elif data == "full":
        A = torch.randn(M, K, generator=g)
        Bt = torch.cat([torch.randn(N, K1, generator=g) / K1 ** 0.5] +
                       ([torch.randn(N, K2, generator=g) / K2 ** 0.5] if K2 else []), 1)
        bias = torch.randn(N, generator=g)
        cin = torch.randn(M, N, generator=g)
    else:
        raise ValueError(data)
    keep_in = torch.rand(M, N, generator=g) > 0.4
    A, Bt, cin = A.bfloat16(), Bt.bfloat16(), cin.bfloat16()
    return dict(A1=A[:, :K1].contiguous(), B1t=Bt[:, :K1].contiguous(),
                A2=A[:, K1:].contiguous() if K2 else None,
                B2t=Bt[:, K1:].contiguous() if K2 else None,
                bias=bias.float(), cin=cin, keep_in=keep_in, K=K, data=data)


# ------------------------------------------------------------------------------ oracle
def product(c):
    """fp64 ``A1 B1 (+ A2 B2)`` and the same over the absolute values."""
    P = c["A1"].double() @ c["B1t"].double().t()
    SP = c["A1"].double().abs() @ c["B1t"].double().abs().t()
    if c["A2"] is not None:
        P = P + c["A2"].double() @ c["B2t"].double().t()
        SP = SP + c["A2"].double().abs() @ c["B2t"].double().abs().t()
    return P, SP


def epilogue(P, SP, bias, cin, keep_in, relu):
    """The rest of the contract in fp64, elementwise (``cin`` / ``keep_in``: None = absent):
    ``v`` before the masks, ``S`` its absolute sum, ``out`` and ``keep`` (``v > 0`` after the
    input mask; what a ReLU call writes to mask_out)."""
    v = P
    S = SP
    if bias is not None:
        v = v + bias.double()
        S = S + bias.double().abs()
    if cin is not None:
        v = v + cin.double()
        S = S + cin.double().abs()
    vm = v if keep_in is None else torch.where(keep_in, v, torch.zeros_like(v))
    keep = vm > 0
    out = torch.where(keep, vm, torch.zeros_like(vm)) if relu else vm
    return dict(v=v, S=S, vm=vm, keep=keep, out=out)


def oracle(c, cin, mask_in, relu):
    P, SP = product(c)
    return epilogue(P, SP, c["bias"], c["cin"] if cin else None,
                    c["keep_in"] if mask_in else None, relu)


def accumulation(e, K: int):
    """The second term of the allowance: fp32 accumulation of K + 2 terms in any order."""
    return (K + 3) * 2.0 ** -24 * e["S"]


def allowance(e, K: int):
    return 2.0 ** -8 * e["out"].abs() + accumulation(e, K)


def sure(e, K: int, keep_in):
    """Where a keep bit is compared on full-mantissa data."""
    s = e["vm"].abs() > accumulation(e, K)
    return s if keep_in is None else s | ~keep_in


def unrepresentable(v) -> float:
    """The share of ``v`` (fp64) that is not a bf16 number."""
    return float((v.float().bfloat16().double() != v).double().mean())


def exact_ok(c, e) -> None:
    """The precondition of the bitwise comparison, from the reference alone."""
    assert float(e["S"].max()) < 2 ** 11                # <= 11 bits above the point
    assert bool((e["v"] * 8 == (e["v"] * 8).round()).all())  # and 3 below: 14 <= 24
    assert unrepresentable(e["v"]) >= 0.25, unrepresentable(e["v"])


# ------------------------------------------------------------------------------ CPU tests
def test_table_reaches_every_instantiation():
    got = {reach(*c) for c in TABLE}
    ch = {("ch", nt, a, b) for nt in (4, 6, 8) for a in (4, 6, 8) for b in (0, 4, 6, 8)}
    bs = {("bs", nt, k, hc, hm, r) for nt in (4, 6, 8) for k in (192, 256, 512)
          for hc in (False, True) for hm in (False, True) for r in (False, True)}
    assert len(ch) == 36 and len(bs) == 72
    assert got == ch | bs
    # variant 1 reaches every column-half kernel on its own, with both production flags
    for f in PRODUCTION:
        assert {reach(*c) for c in TABLE if c.variant == 1 and tuple(c[4:]) == f} == ch
    # every shape the B-stationary kernel accepts, every flag combination
    assert sum(bs_supported(*s) for s in SHAPES) == 12
    for s in SHAPES:
        if bs_supported(*s):
            assert {tuple(c[4:]) for c in TABLE if c.variant == 2 and c[1:4] == s} == set(FLAGS)


def test_all_flags_per_nt_and_ring_depth():
    for (N, K1, K2), depth in V1_ALL_FLAGS.items():
        assert ring_depth((K1 + K2) // 32) == depth
        assert {tuple(c[4:]) for c in TABLE if c.variant == 1 and c[1:4] == (N, K1, K2)} == \
            set(FLAGS)
    assert {n for n, _, _ in V1_ALL_FLAGS} == set(NS)
    assert set(V1_ALL_FLAGS.values()) == {2, 3, 4, 8}
    assert {ring_depth(nc) for nc in (4, 6, 10)} == {2, 3} and ring_depth(14) == 2
    for v, (K1, K2) in LAYOUT_SHAPES.items():
        for N in NS:
            assert reach(v, N, K1, K2, 1, 1, 1)[0] == ("ch" if v == 1 else "bs")


def test_long_cases_cover_every_ring_depth():
    every = {bs_nbuf(nt, k, hc, hm) for nt in (4, 6, 8) for k in (192, 256, 512)
             for hc in (0, 1) for hm in (0, 1)}
    cases = long_cases()
    got = [bs_nbuf(c.N // 32, c.K1 + c.K2, c.cin, c.mask_in) for c in cases if c.variant == 2]
    assert sorted(got) == sorted(every) and min(every) >= 2
    assert bs_nbuf(8, 512, 1, 0) == 2 and bs_nbuf(8, 256, 0, 0) == 8
    assert [reach(*c)[0] for c in cases].count("ch") == 1
    # an 8-slot ring turns over twice and every block of 256 CUs runs 18 or 19 tiles
    assert (m_long(256) + 31) // 32 == 18 * 256 + 1 and (m_cus(256) + 31) // 32 == 3 * 256 + 1


def test_row_counts():
    # column-half: a full 256-row tile, then a full wave, a wave with one row, six past M
    assert M_TAIL == 256 + 32 + 1
    # B-stationary: nine full 32-row tiles and a one-row tile
    assert divmod(M_TAIL, 32) == (9, 1)


@pytest.mark.parametrize("flags", FLAGS, ids=str)
def test_oracle_against_dense_evaluation(flags):
    """The oracle against the contract written out term by term, the masks through a
    tile32 round trip."""
    N, K1, K2, M = 128, 128, 192, 37
    c = make_inputs(N, K1, K2, M, "full")
    cin, mask_in, relu = flags
    e = oracle(c, *flags)
    A = torch.cat([c["A1"], c["A2"]], 1).double()
    B = torch.cat([c["B1t"], c["B2t"]], 1).double().t()
    terms = A.unsqueeze(2) * B.unsqueeze(0)            # [M, K, N]
    v = terms.sum(1) + c["bias"].double()
    S = terms.abs().sum(1) + c["bias"].double().abs()
    if cin:
        v, S = v + c["cin"].double(), S + c["cin"].double().abs()
    torch.testing.assert_close(e["v"], v, rtol=0, atol=1e-12)
    torch.testing.assert_close(e["S"], S, rtol=0, atol=1e-12)
    if mask_in:
        kin = R.tile32_decode(R.tile32_encode(c["keep_in"]), M, N)
        assert torch.equal(kin, c["keep_in"])
        v = v * kin
    if relu:
        v = v.clamp_min(0)
    torch.testing.assert_close(e["out"], v, rtol=0, atol=1e-12)
    assert torch.equal(e["keep"], (e["vm"] > 0))
    assert torch.equal(R.tile32_decode(R.tile32_encode(e["keep"]), M, N), e["keep"])
    assert bool((allowance(e, K1 + K2) > 0).all())


@pytest.mark.parametrize("N", NS)
def test_caps_hold_on_every_shape(N):
    """At M = 289 and the small row counts: the exact data is exact and rounds (at least a
    quarter of ``v`` is no bf16 number), and the full-mantissa data leaves at most 0.5 % of
    the keep bits uncompared. The GPU tests assert the same at their larger row counts."""
    for K1 in K1S:
        for K2 in K2S:
            for data in ("exact", "full"):
                c = make_inputs(N, K1, K2, M_TAIL, data)
                P, SP = product(c)
                for f in FLAGS:
                    e = epilogue(P, SP, c["bias"], c["cin"] if f[0] else None,
                                 c["keep_in"] if f[1] else None, f[2])
                    if data == "exact":
                        exact_ok(c, e)
                        assert bool((e["v"] == 0).any())  # keep is v > 0, not v >= 0
                    else:
                        s = sure(e, K1 + K2, c["keep_in"] if f[1] else None)
                        assert float((~s).double().mean()) <= OMIT_CAP


def test_exact_data_has_both_signs_and_zeros():
    c = make_inputs(256, 256, 256, M_TAIL, "exact")
    e = oracle(c, 0, 0, 1)
    share = float(e["keep"].double().mean())
    assert 0.3 < share < 0.7
    assert bool((e["v"] == 0).any())
    # keep bits vary along rows and along columns
    assert bool((e["keep"].any(0) & ~e["keep"].all(0)).sum() >= 64)
    assert bool((e["keep"].any(1) & ~e["keep"].all(1)).all())
