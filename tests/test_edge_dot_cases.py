"""Inputs and references of tests/test_edge_dot_variants_gpu.py, which runs the per-edge dot
product kernel (csrc/kernels/sddmm.hip) at every (VEC, L, NB) plan its launcher can pick, and
the CPU tests that pin both down first. Nothing here touches the native library.

* :func:`plan_of` / :func:`chunk_of`: the launcher's rule restated from the header comment
  of sddmm.hip, and :data:`PLAN_CASES`, the ``(F, heads)`` of the GPU tests with the plan each
  must reach. The table covers the 17 plans of ``launch_typed``'s dispatch list (read from the
  source), each with one head and with several, each path with heads that are no power of two.
* :func:`boundary_csr`: a pattern built from a plan's chunk size ``c`` (the slots a wave
  resolves with one search of ``rowptr``), so that for every plan chunk boundaries fall on a
  row end, on the start of a run of empty rows, inside a run of degree-1 rows and inside a
  long row, with empty rows in front and behind.
* :func:`deep_csr`: ``nrows`` rows, all empty but the first, the last and those at
  ``64^j - 1, 64^j, 64^j + 1``: the row counts at which the 64-ary search gains a level.
  ``mult`` widens every non-empty row so that later chunks start inside deep rows.
* :func:`refs`: inputs, fp64 and fp32 contract (``test_edge_dot.edge_dot_contract``) of one
  ``(case, dtype, pattern)``, computed once and shared by every test that needs them.
* The sensitivity test: on the boundary pattern, one slot at a chunk start scored with the
  wrong a-row, without its last term, with the next head of a, or with the wrong row scale is
  further from the fp64 contract than ``test_gat_kernels.bound`` allows, for every case. The
  accuracy rule of the GPU tests therefore notices one wrong slot.
"""
from __future__ import annotations

import functools
import pathlib
import re

import pytest
import torch

from dgraph_amd.ops.csr import CSR
from test_edge_dot import edge_dot_contract, slot_rows
from test_gat_kernels import bound
from test_pna import skewed_csr, values

NCOLS = 257
KWAVE = 64
CHUNK_MAX = 512
SCALE = -0.35  # of the boundary pattern, with row_scale = linspace(0.25, 2.0, nrows)


# ------------------------------------------------------------------------------ the plan
def plan_of(F, heads):
    """``(VEC, L, NB)`` the launcher picks: VEC elements per lane, L lanes per head, NB
    resident column blocks (0: the run-time loop)."""
    assert F > 0 and heads > 0 and F % heads == 0
    D = F // heads
    q = D // 4
    if D % 4 == 0 and D <= 1024 and q & (q - 1) == 0:
        L = min(q, KWAVE)
        return 4, L, q // L
    L = 1
    while L < D and L < KWAVE:
        L *= 2
    return 1, L, 1 if D <= KWAVE else 0


def chunk_of(F, heads):
    """Slots per chunk: 16 batches of (slot, head) pairs, at most 512 slots, at least the
    slots of one batch."""
    _, L, NB = plan_of(F, heads)
    ku = 8 // NB if NB > 0 else 4
    batch = KWAVE // L * ku
    return max(-(-batch // heads), min(CHUNK_MAX, 16 * batch // heads))


ALL_PLANS = ([(4, L, 1) for L in (1, 2, 4, 8, 16, 32, 64)] + [(4, 64, 2), (4, 64, 4)]
             + [(1, L, 1) for L in (1, 2, 4, 8, 16, 32, 64)] + [(1, 64, 0)])

# (F, heads) -> the plan it must select
PLAN_CASES = {
    (4, 1): (4, 1, 1), (12, 3): (4, 1, 1), (64, 16): (4, 1, 1),
    (8, 1): (4, 2, 1), (24, 3): (4, 2, 1),
    (16, 1): (4, 4, 1), (64, 4): (4, 4, 1),
    (32, 1): (4, 8, 1), (256, 8): (4, 8, 1),
    (64, 1): (4, 16, 1), (512, 8): (4, 16, 1),
    (128, 1): (4, 32, 1), (384, 3): (4, 32, 1),
    (256, 1): (4, 64, 1), (512, 2): (4, 64, 1),
    (512, 1): (4, 64, 2), (1024, 2): (4, 64, 2),
    (1024, 1): (4, 64, 4), (2048, 2): (4, 64, 4),
    (1, 1): (1, 1, 1), (3, 3): (1, 1, 1),
    (2, 1): (1, 2, 1), (6, 3): (1, 2, 1),
    (3, 1): (1, 4, 1), (12, 4): (1, 4, 1),
    (5, 1): (1, 8, 1), (6, 1): (1, 8, 1), (7, 1): (1, 8, 1), (14, 2): (1, 8, 1),
    (9, 1): (1, 16, 1), (12, 1): (1, 16, 1), (15, 1): (1, 16, 1), (30, 2): (1, 16, 1),
    (17, 1): (1, 32, 1), (24, 1): (1, 32, 1), (31, 1): (1, 32, 1), (58, 2): (1, 32, 1),
    (33, 1): (1, 64, 1), (48, 1): (1, 64, 1), (63, 1): (1, 64, 1), (100, 2): (1, 64, 1),
    (65, 1): (1, 64, 0), (172, 1): (1, 64, 0), (192, 1): (1, 64, 0), (600, 3): (1, 64, 0),
    (2048, 1): (1, 64, 0),
}

# one case per plan for the layout test; the vector ones with F % 8 == 0, so that a row
# stride of F + 12 is divisible by 4 and not by 8
LAYOUT_CASES = [(64, 16), (24, 3), (64, 4), (256, 8), (512, 8), (384, 3), (512, 2), (1024, 2),
                (2048, 2), (3, 3), (6, 3), (12, 4), (14, 2), (30, 2), (58, 2), (100, 2),
                (600, 3)]

DEEP_ROWS = [1, 2, 64, 65, 4096, 4097, 262145]


def plan_tag(F, heads):
    v, L, nb = plan_of(F, heads)
    return f"{'vec' if v == 4 else 'gen'} L={L} NB={nb}"


# ------------------------------------------------------------------------------ patterns
BOUNDARY_TAIL = [2, 0, 3, 7, 0, 0]


def boundary_degrees(c):
    return [0] * 3 + [c] + [0] * 5 + [1] * (c + 3) + [2 * c + 1] + BOUNDARY_TAIL


@functools.lru_cache(maxsize=None)
def _boundary(c):
    deg = torch.tensor(boundary_degrees(c))
    rowptr = torch.zeros(deg.numel() + 1, dtype=torch.long)
    rowptr[1:] = torch.cumsum(deg, 0)
    # the seed is a condition on the inputs: with it the column of the designated slot makes
    # every corruption of the sensitivity test exceed the bound in every case (seeds 100,
    # 300, ... 900 each leave some head's last term under it)
    col = torch.randint(0, NCOLS, (int(rowptr[-1]),),
                        generator=torch.Generator().manual_seed(1100 + c))
    return rowptr, col


def boundary_csr(c, idx=torch.int64) -> CSR:
    """``c + 19`` rows, ``4 c + 16`` slots over 257 columns, for a chunk of ``c`` slots: three
    empty rows; a row of ``c`` (it ends at slot ``c``); five empty rows (the run starts on
    the boundary); ``c + 3`` rows of one entry (across the boundary at ``2 c``, an a-reload
    per slot); a row of ``2 c + 1`` (across ``3 c`` and ``4 c``); rows of 2, 0, 3 and 7; two
    empty rows."""
    rowptr, col = _boundary(int(c))
    return CSR(rowptr, col.to(idx), NCOLS)


@functools.lru_cache(maxsize=None)
def _deep(nrows, mult):
    deg = torch.zeros(nrows, dtype=torch.long)
    marks = {0, nrows - 1}
    p = KWAVE
    while p - 1 < nrows:
        marks.update(r for r in (p - 1, p, p + 1) if r < nrows)
        p *= KWAVE
    for i, r in enumerate(sorted(marks)):
        deg[r] = (1 + i % 3) * mult
    if nrows == 1:
        deg[0] = 3 * mult
    rowptr = torch.zeros(nrows + 1, dtype=torch.long)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, NCOLS, (int(rowptr[-1]),),
                        generator=torch.Generator().manual_seed(200 + nrows % 97))
    return rowptr, col


def deep_csr(nrows, idx=torch.int64, mult=1) -> CSR:
    """``nrows`` rows, empty except the first, the last and ``64^j - 1, 64^j, 64^j + 1``
    (j >= 1) where they exist; those hold ``mult`` times 1, 2, 3, 1, ... entries in row
    order (a single row: 3)."""
    rowptr, col = _deep(int(nrows), int(mult))
    return CSR(rowptr, col.to(idx), NCOLS)


def case_inputs(F, nrows, dtype=torch.float32):
    """a [nrows, F] and b [257, F], rounded to ``dtype`` and returned as fp32."""
    a, b = values("plain", nrows, F, F + 1), values("plain", NCOLS, F, F + 2)
    return a.to(dtype).float(), b.to(dtype).float()


@functools.lru_cache(maxsize=None)
def refs(F, heads, dtype=torch.float32, pattern="skewed"):
    """(a, b, row_scale, scale, fp64 scores, fp32 scores) of one case on ``"skewed"``
    (``test_pna.skewed_csr``, no scaling) or ``"boundary"`` (``boundary_csr`` of the case's
    chunk, rows scaled by 0.25 .. 2.0 and everything by -0.35). Callers leave them unchanged."""
    if pattern == "skewed":
        csr, rs, scale = skewed_csr(), None, 1.0
    else:
        csr = boundary_csr(chunk_of(F, heads))
        rs, scale = torch.linspace(0.25, 2.0, csr.num_rows), SCALE
    a, b = case_inputs(F, csr.num_rows, dtype)
    r64 = edge_dot_contract(csr.rowptr, csr.col, a, b, heads, scale, rs)
    r32 = edge_dot_contract(csr.rowptr, csr.col, a, b, heads, scale, rs, dtype=torch.float32)
    return a, b, rs, scale, r64, r32


# ------------------------------------------------------------------------------ the table
def test_plan_table_is_the_dispatch_list():
    for (F, heads), plan in PLAN_CASES.items():
        assert plan_of(F, heads) == plan, (F, heads)
    assert set(PLAN_CASES.values()) == set(ALL_PLANS) and len(set(ALL_PLANS)) == 17
    src = pathlib.Path(__file__).resolve().parents[1] / "csrc" / "kernels" / "sddmm.hip"
    listed = re.findall(r"DG_SDDMM\((\d+), (\d+), (\d+)\)", src.read_text())
    assert sorted(tuple(map(int, t)) for t in listed) == sorted(ALL_PLANS)


def test_plan_table_heads_and_widths():
    for plan in ALL_PLANS:
        hs = [h for (F, h), p in PLAN_CASES.items() if p == plan]
        assert 1 in hs and max(hs) > 1, plan
    for vec in (4, 1):
        assert any(h & (h - 1) for (F, h), p in PLAN_CASES.items() if p[0] == vec)
    # generic resident plans: the smallest D of the L, D = L - 1, and a multiple of 4 that
    # the vector path refuses
    for L in (8, 16, 32, 64):
        ds = {F // h for (F, h), p in PLAN_CASES.items() if p == (1, L, 1)}
        assert {L // 2 + 1, L - 1}.issubset(ds), L
        assert L == 8 or any(d % 4 == 0 for d in ds), L  # 5 .. 7 holds no multiple of 4
    assert sorted({plan_of(*c) for c in LAYOUT_CASES}) == sorted(ALL_PLANS)
    assert len(LAYOUT_CASES) == 17
    assert all(F % 8 == 0 for F, h in LAYOUT_CASES if plan_of(F, h)[0] == 4)


def test_chunk_sizes():
    """The rule against figures worked out by hand from the header comment, and the range."""
    by_hand = {(4, 1): 512, (2048, 2): 16, (1024, 1): 32, (512, 1): 64, (256, 1): 128,
               (512, 2): 64, (600, 3): 21, (2048, 1): 64, (33, 1): 128, (17, 1): 256,
               (64, 16): 512, (3, 1): 512}
    for case, c in by_hand.items():
        assert chunk_of(*case) == c, case
    chunks = {chunk_of(*c) for c in PLAN_CASES}
    assert min(chunks) == 16 and max(chunks) == 512 and any(c % 2 for c in chunks)


@pytest.mark.parametrize("c", sorted({chunk_of(*c) for c in PLAN_CASES}))
def test_boundary_pattern_properties(c):
    csr = boundary_csr(c, torch.int32)
    rp, deg = csr.rowptr.tolist(), csr.degree().tolist()
    assert csr.num_rows == c + 19 and csr.nnz == 4 * c + 16 and csr.col.dtype == torch.int32
    assert deg == boundary_degrees(c)
    assert int(csr.col.min()) >= 0 and int(csr.col.max()) < NCOLS
    # leading and trailing empty rows
    assert rp[:4] == [0, 0, 0, 0] and deg[3] == c
    assert rp[-3:] == [csr.nnz] * 3 and deg[-3] == 7
    # row 3 ends exactly at slot c and the run of five empty rows starts on that boundary
    assert rp[4] == c and rp[4:10] == [c] * 6
    # rows 9 .. c + 11 hold one entry each; the one that ends at 2 c is inside the run
    assert deg[9:c + 12] == [1] * (c + 3)
    assert rp[9] < 2 * c < rp[c + 12] and rp[c + 9] == 2 * c
    ends = [r for r in range(csr.num_rows) if deg[r] > 0 and rp[r + 1] % c == 0]
    assert ends[:2] == [3, c + 8]
    # the long row straddles two boundaries
    assert deg[c + 12] == 2 * c + 1 and rp[c + 12] < 3 * c < 4 * c < rp[c + 13]
    again = boundary_csr(c, torch.int64)
    assert again.col.dtype == torch.int64 and torch.equal(again.col, csr.col.long())


@pytest.mark.parametrize("nrows", DEEP_ROWS)
@pytest.mark.parametrize("mult", [1, 300])
def test_deep_pattern_properties(nrows, mult):
    csr = deep_csr(nrows, torch.int32, mult)
    deg = csr.degree()
    full = torch.nonzero(deg).flatten().tolist()
    want = {0, nrows - 1} | {r for p in (64, 4096, 262144) for r in (p - 1, p, p + 1)
                             if r < nrows}
    assert full == sorted(want)
    assert csr.num_rows == nrows and int(csr.rowptr[0]) == 0
    assert set((deg[full] // mult).tolist()) <= {1, 2, 3} and int((deg[full] % mult).sum()) == 0
    if nrows == 1:
        assert csr.nnz == 3 * mult
    if mult > 1 and nrows > 2:
        # chunks of 512 slots start inside rows past the first
        rows = slot_rows(csr.rowptr)
        starts = rows[torch.arange(0, csr.nnz, CHUNK_MAX)]
        assert int(starts.max()) >= 63


# ------------------------------------------------------------------------------ sensitivity
def designated_slot(rowptr, c):
    """The first slot of the second chunk, or of the first later chunk whose first slot
    starts a row; with the row before it."""
    rows = slot_rows(rowptr)
    k = c
    while int(rows[k]) == int(rows[k - 1]):
        k += c
    return k, int(rows[k]), int(rows[k - 1])


@pytest.mark.parametrize("F,heads", list(PLAN_CASES))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_one_wrong_slot_exceeds_the_bound(F, heads, dtype):
    c = chunk_of(F, heads)
    csr = boundary_csr(c)
    a, b, rs, scale, r64, r32 = refs(F, heads, dtype, "boundary")
    bd = bound(r64, r32)
    k, r, prev = designated_slot(csr.rowptr, c)
    assert k % c == 0 and k >= c and prev != r and int(csr.degree()[prev]) > 0
    D = F // heads
    ar, ap = a[r].double().view(heads, D), a[prev].double().view(heads, D)
    bc = b[int(csr.col[k])].double().view(heads, D)
    f, fprev = scale * float(rs[r].double()), scale * float(rs[prev].double())
    right = f * (ar * bc).sum(-1)
    assert float((right - r64[k]).abs().max()) <= 1e-12 * max(1.0, float(r64.abs().max()))
    wrong = {"a-row of the row before": f * (ap * bc).sum(-1),
             "row_scale of the row before": fprev * (ar * bc).sum(-1)}
    for h in range(heads):
        if D > 1:
            w = right.clone()
            w[h] = f * (ar[h, :D - 1] * bc[h, :D - 1]).sum()
            wrong[f"head {h} without its last term"] = w
        if heads > 1:
            w = right.clone()
            w[h] = f * (ar[(h + 1) % heads] * bc[h]).sum()
            wrong[f"head {h} with a's head {(h + 1) % heads}"] = w
    for name, w in wrong.items():
        err = float((w - r64[k]).abs().max())
        print(f"[F={F},H={heads}] slot {k}, {name}: off by {err:.3e}, bound {bd:.3e}")
        assert err > bd, f"{name}: off by {err:.3e}, within the bound {bd:.3e}"
