"""The comparisons of the fp32 kernel tests bite, shown without a kernel: each oracle's
correct CPU result passes the assertion the GPU tests use, and each of a list of
deliberately wrong results (one term dropped, an off-by-one range, swapped sources, a
padding row counted, a shifted unit boundary, a stale slab, a flipped bit, the wrong tie)
fails it. Also here, because they need no GPU: the exactness preconditions of every exact
case, the written-out formula against the CPU path it restates, and the CPU path's
``rowend`` against the dense definition.
"""
from __future__ import annotations

import pytest
import torch

import test_f32_small_kernels_gpu as SK
import test_spmm_f32_variants_gpu as SP
import test_wgrad_f32_units_gpu as WG
from dgraph_amd.ops import f32 as F32


# ------------------------------------------------------------------------------ SpMM
@pytest.mark.parametrize("family", SP.FAMILIES)
def test_spmm_exactness_preconditions(family):
    """Every call of the variant sweep: the fp64 reference is an fp32 number and the sums
    of |terms| stay below 2^24 units of the smallest fraction (:func:`exact_ok`)."""
    for F in SP.WIDTHS + (260, 320):
        F = F + (-F) % 32 if family == "kb" else F
        for frac in SP._fracs(family, F):
            for epi in (False, True):
                SP._case(family, F, frac, epi)  # asserts exact_ok


@pytest.mark.parametrize("family", SP.FAMILIES)
def test_spmm_formula_is_the_cpu_path(family):
    """The written-out formula (the fp32 side of ``bound``) in fp64 equals the fp64 CPU
    path; in fp32, on an exact call, it equals it too: another summation order and another
    precision change nothing, which is what the bitwise comparison rests on."""
    F = 64 if family == "kb" else 36
    c = SP.make_call(family, F, 0.5, True)
    ref = SP.oracle(c)
    assert torch.equal(SP.formula(c, torch.float64), ref)
    assert torch.equal(SP.formula(c, torch.float32).double(), ref)
    SP.assert_exact(ref.float(), c)


def test_spmm_cpu_path_rowend_dense():
    """The CPU path's ``rowend`` (nothing else pins it) against a dense matrix built from
    the entries ``[rowptr[r], rowend[r])``, with edge weights and a row list."""
    rp, col = SP.pattern()
    g = SP.gen("dense")
    c = SP.make_call("w1", 36)
    re = SP.split_points(g)
    rows = torch.randint(0, SP.NROWS, (50,), generator=g)
    A = torch.zeros(SP.NROWS, SP.NCOL, dtype=torch.float64)
    for r in range(SP.NROWS):
        e = torch.arange(int(rp[r]), int(re[r]))
        A[r].index_add_(0, col[e], c["edge_weight"][e].double())
    out = torch.zeros(50, 36, dtype=torch.float64)
    F32.spmm_f32(rp, col, c["x"], out, edge_weight=c["edge_weight"], rowend=re, row_ids=rows)
    assert torch.equal(out, A[rows] @ c["x"].double())
    # and the partitioned form: the second run of every row, starting at the cut
    out2 = out.clone()
    F32.spmm_f32(re, col, c["x"], out2, edge_weight=c["edge_weight"],
                 rowend=rp[1:].contiguous(), row_ids=rows, beta=1.0)
    whole = torch.zeros(50, 36, dtype=torch.float64)
    F32.spmm_f32(rp, col, c["x"], whole, edge_weight=c["edge_weight"], row_ids=rows)
    assert torch.equal(out2, whole)


def _must_fail(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


def test_spmm_mutations_are_caught():
    F = 36
    rp, col = SP.pattern()
    deg = rp[1:] - rp[:-1]
    # a row whose last chunk has padding slots at every lane-group width
    r = int(torch.nonzero((deg >= 2) & (deg % 8 != 0))[3])
    # one entry of one row dropped
    c = SP.make_call("w3", F, epi=True)
    keep = torch.ones(col.numel(), dtype=torch.bool)
    keep[int(rp[r]) + 1] = False
    cut = rp.clone()
    cut[r + 1:] -= 1
    wrong = SP.oracle(dict(c, rowptr=cut, col=col[keep], edge_weight=c["edge_weight"][keep]))
    SP.assert_exact(SP.oracle(c).float(), c)
    assert not torch.equal(wrong, SP.oracle(c))
    _must_fail(SP.assert_exact, wrong.float(), c)
    # rowend off by one
    c = dict(SP.make_call("w0", F), rowend=SP.split_points(SP.gen("mut")))
    re = c["rowend"].clone()
    re[r] += 1 if int(re[r]) < int(rp[r + 1]) else -1
    _must_fail(SP.assert_exact, SP.oracle(dict(c, rowend=re)).float(), c)
    # x and x2 swapped for one column: one entry reads the other source's row
    c = SP.make_call("two", F)
    e = int(rp[r])
    other = col.clone()
    other[e] = SP.NSPLIT + int(col[e]) % (SP.NCOL - SP.NSPLIT) if int(col[e]) < SP.NSPLIT \
        else int(col[e]) - SP.NSPLIT
    assert (int(other[e]) < SP.NSPLIT) != (int(col[e]) < SP.NSPLIT)
    _must_fail(SP.assert_exact, SP.oracle(dict(c, col=other)).float(), c)
    # a padding slot's row (row 0) added with weight 1
    for family in ("w0", "twom", "gs2"):
        c = SP.make_call(family, F, 0.5)
        wrong = SP.oracle(c)
        wrong[r] += c["x"][0].double()
        _must_fail(SP.assert_exact, wrong.float(), c)
    # a NaN from a stray gather
    c = SP.stray_call("w3m", F)
    wrong = SP.oracle(c)
    wrong[5, 7] = float("nan")
    _must_fail(SP.assert_exact, wrong.float(), c)


def test_spmm_bound_rejects_bf16_products():
    """The full-mantissa comparison rejects an operand rounded to bf16 and accepts the
    fp32 evaluation."""
    for family in ("w0", "w3m", "gs2"):
        c = SP.make_call(family, 64, 0.5, True, normal=True)
        SP.assert_bound(SP.formula(c, torch.float32), c)
        low = dict(c, x=c["x"].bfloat16().float())
        if c.get("x2") is not None:
            low["x2"] = c["x2"].bfloat16().float()
        _must_fail(SP.assert_bound, SP.oracle(low).float(), c)


# ------------------------------------------------------------------------------ wgrad
def test_wgrad_exactness_preconditions():
    for K, N in WG.PAIRS:
        for split in WG.SPLITS:
            c = WG.make_case(K, N, WG.split_of(split, K), 1000, 7, 3)
            WG.exact_ok(c, WG.slabs_ref(c))
    c = WG.make_case(128, 128, 64, 32 * 259 - 5, 259, 129)
    WG.exact_ok(c, WG.slabs_ref(c))
    # an fp32 evaluation (another order, another precision) is the same number
    c = WG.make_case(256, 176, 128, 1000, 7, 3)
    for a, b in zip(WG.slabs_ref(c, torch.float32), WG.slabs_ref(c)):
        assert torch.equal(a.double(), b)


def test_wgrad_contract_units():
    """The contract's arithmetic: M = 33 in 7 units leaves five empty ones; the units of a
    call partition its rows in order."""
    assert WG.unit_bounds(33, 7) == [0, 32, 33, 33, 33, 33, 33, 33]
    assert WG.unit_bounds(1000, 7) == [0, 160, 320, 480, 640, 800, 960, 1000]
    assert WG.unit_bounds(65, 2) == [0, 64, 65]
    c = WG.make_case(128, 128, 64, 1000, 7, 0)
    slabs, cols = WG.slabs_ref(c)
    assert torch.equal(slabs[:7].sum(0), WG.operand(c).double().t() @ c["G"].double())
    assert torch.equal(cols[:7].sum(0), c["G"].double().sum(0))
    assert torch.equal(slabs[7:], c["old"][7:].double())


def test_wgrad_mutations_are_caught():
    c = WG.make_case(128, 176, 64, 1000, 7, 3)
    good = WG.slabs_ref(c)
    WG.assert_slabs_exact(tuple(t.float() for t in good), c)
    # one unit boundary shifted by 32 rows
    b = WG.unit_bounds(1000, 7)
    b[4] += 32
    _must_fail(WG.assert_slabs_exact, tuple(t.float() for t in WG.slabs_ref(c, bounds=b)), c)
    # fresh_from off by one, either way
    for ff in (2, 4):
        wrong = WG.slabs_ref(dict(c, fresh_from=ff))
        _must_fail(WG.assert_slabs_exact, tuple(t.float() for t in wrong), c)
        # (the slabs alone, and the column sums alone)
        _must_fail(WG.assert_slabs_exact, (wrong[0].float(), good[1].float()), c)
        _must_fail(WG.assert_slabs_exact, (good[0].float(), wrong[1].float()), c)
    # a slab past P written
    wrong = (good[0].clone(), good[1])
    wrong[0][8, 5, 5] += 1
    _must_fail(WG.assert_slabs_exact, tuple(t.float() for t in wrong), c)
    # a1_rows applied to the A2 columns too
    both = dict(c, A2=c["A2"][c["a1_rows"].clamp(max=999)])
    _must_fail(WG.assert_slabs_exact, tuple(t.float() for t in WG.slabs_ref(both)), c)
    # a bf16-truncated operand against the full-mantissa bound
    n = WG.make_case(128, 176, 64, 1000, 7, 3, normal=True)
    WG.assert_slabs_bound(WG.slabs_ref(n, torch.float32), n)
    low = dict(n, G=n["G"].bfloat16().float())
    _must_fail(WG.assert_slabs_bound, tuple(t.float() for t in WG.slabs_ref(low)), n)


# ------------------------------------------------------------------------------ bits, loss
def test_keep_bit_flip_is_caught():
    g = SP.gen("flip")
    mask = torch.rand(7, 96, generator=g) < 0.5
    SK.assert_bits_equal(SP.pack_bits(mask), mask)
    flipped = mask.clone()
    flipped[3, 48] = ~flipped[3, 48]
    _must_fail(SK.assert_bits_equal, SP.pack_bits(flipped), mask)
    # the packing itself: bit c % 32 of word c / 32, as the ops' own unpacking reads it
    assert torch.equal(F32.unpack_keep_bits(SP.pack_bits(mask), 96), mask)
    h = SK.keep_values(7, 96, g)
    assert torch.equal(F32.row_keep_bits(h), SP.pack_bits(h > 0))
    assert not bool((h > 0)[(h == 0) | h.isnan()].any())


def test_second_tied_argmax_is_caught():
    C = 129
    z, rows, y = SK.argmax_case(C)
    zr = z[rows][:, :C]
    SK.assert_hits(SK.first_argmax_hits(z, rows, y, C), z, rows, y, C)
    last = C - 1 - (zr == zr.max(1, keepdim=True).values).int().flip(1).argmax(1)
    _must_fail(SK.assert_hits, (last == y).to(torch.uint8), z, rows, y, C)
    # torch's own argmax follows the first-maximum rule the helper states
    assert torch.equal(SK.first_argmax_hits(z, rows, y, C), (zr.argmax(1) == y).to(torch.uint8))


def test_xent_bound_rejects_missing_max_subtraction():
    """The loss comparison accepts the fp32 CPU evaluation and rejects a softmax without
    the max subtraction on the scaled logits (inf / inf)."""
    C, n = 65, 5
    g = SP.gen("xent", C, n, 150.0)
    z = torch.randn(n + 13, C, generator=g) * 150.0
    rows, y = torch.arange(n), torch.randint(0, C, (n,), generator=g)
    loss, dz = SK.xent_ref(z, rows, y, 0.5, C, torch.float32)
    SK.assert_xent(loss, dz, z, rows, y, 0.5, C)
    e = z[rows].exp()
    naive = e.sum(1).log() - z[rows].gather(1, y.unsqueeze(1)).squeeze(1)
    _must_fail(SK.assert_xent, naive, dz, z, rows, y, 0.5, C)
