"""The per-edge dot product kernel (csrc/kernels/sddmm.hip) on the GPU at every one of its 17
(VEC, L, NB) plans, with fp32 and bf16 inputs and int32 and int64 column ids (68 kernels),
against the contract of tests/test_edge_dot.py evaluated in fp64. The cases, the patterns and
the references come from tests/test_edge_dot_cases.py, which also shows on the CPU that the
accuracy rule notices one wrong slot.

Accuracy rule, as in tests/test_edge_dot_gpu.py: ``|kernel - fp64| <= test_gat_kernels.bound(
ref64, ref32)`` with both references from the contract; nothing is taken from the kernel's own
output. For bf16 the contract takes the bf16-rounded inputs. Every ``error / bound`` is
printed before it is asserted. Scores go into a sentinel-filled buffer with 8 spare rows,
which must stay untouched.

Largest error / bound seen on an MI355X, per plan over its cases, both patterns and both
index widths (fp32 / bf16), and of the row search (a record, not an input to any bound):

    vector  L=1        0.004 / 0.004      generic L=1        0.003 / 0.003
    vector  L=2        0.005 / 0.003      generic L=2        0.003 / 0.003
    vector  L=4        0.005 / 0.003      generic L=4        0.004 / 0.004
    vector  L=8        0.006 / 0.004      generic L=8        0.007 / 0.003
    vector  L=16       0.007 / 0.006      generic L=16       0.006 / 0.004
    vector  L=32       0.005 / 0.004      generic L=32       0.006 / 0.005
    vector  L=64 NB=1  0.006 / 0.007      generic L=64 NB=1  0.007 / 0.004
    vector  L=64 NB=2  0.007 / 0.006      generic L=64 NB=0  0.007 / 0.006
    vector  L=64 NB=4  0.006 / 0.005      row search, F = 4 and F = 3 (fp32)  0.005

(The floor of the bound, 2e-5 of the largest value, is what most cases meet; the kernel's
fma's are closer to fp64 than the fp32 contract is.) The module takes about 3 s.

Checked once against a scratch build of the kernel with one line changed at a time (a head
change that does not reload a's segment, a row change that does not, a row walk that stops one
row early at a row end, a generic path that drops its last column): each fails between 58 and
266 of these tests. With G = 64 / L lane groups a multiple of ``heads`` a lane never sees a
second head, so the stale-head change can only show where it is not: those cases fail it.
"""
from __future__ import annotations

import functools

import pytest
import torch

from dgraph_amd import _native
from dgraph_amd.ops import kernels as K
from test_edge_dot import edge_dot_contract
from test_edge_dot_cases import (DEEP_ROWS, LAYOUT_CASES, NCOLS, PLAN_CASES, boundary_csr,
                                 chunk_of, deep_csr, plan_of, plan_tag, refs)
from test_gat_kernels import bound
from test_pna import skewed_csr, values

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.25e9  # what the score buffer holds outside the block the kernel may write
RATIOS: dict = {}
DTYPES = [torch.float32, torch.bfloat16]
DTYPE_IDS = ["fp32", "bf16"]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(RATIOS):
        print(f"\n[edge_dot variants] largest error / bound, {k}: {RATIOS[k]:.3f}", end="")


def within(tag, key, got, ref64, ref32):
    """|got - fp64| against :func:`bound`; prints the figures, records the ratio under
    ``key``."""
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape, f"{tag}: shape {got.shape} != {ref64.shape}"
    assert bool(torch.isfinite(got).all()), f"{tag}: not finite"
    err = float((got - ref64.double()).abs().max())
    bd = bound(ref64, ref32)
    print(f"{tag}: err {err:.3e} bound {bd:.3e} ratio {err / bd:.3f}")
    RATIOS[key] = max(RATIOS.get(key, 0.0), err / bd)
    assert err <= bd, f"{tag}: error {err:.3e} above the bound {bd:.3e}"


def run(csr, a, b, heads, scale=1.0, rs=None):
    """The kernel into a narrow view of a sentinel buffer; asserts the tail stays untouched."""
    buf = torch.full((csr.nnz + 8, heads), SENT, device=a.device)
    s = K.edge_dot(csr.rowptr, csr.col, a, b, buf[:csr.nnz], heads=heads, scale=scale,
                   row_scale=rs)
    assert s.data_ptr() == buf.data_ptr()
    assert bool((buf[csr.nnz:] == SENT).all()), "the kernel wrote past its scores"
    return s


def pattern_csr(pattern, F, heads, idx):
    return skewed_csr(idx) if pattern == "skewed" else boundary_csr(chunk_of(F, heads), idx)


def test_plan_table_is_what_the_library_launches():
    ops = _native.ops()
    for (F, heads), plan in PLAN_CASES.items():
        assert K.edge_dot_vec_path(F, heads) == (plan[0] == 4), (F, heads)
        assert int(ops.edge_dot_chunk_slots(F, heads)) == chunk_of(F, heads), (F, heads)


@pytest.mark.parametrize("F,heads", list(PLAN_CASES))
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("pattern", ["skewed", "boundary"])
def test_forward(F, heads, dtype, pattern):
    a, b, rs, scale, r64, r32 = refs(F, heads, dtype, pattern)
    ad, bd = a.to(DEV).to(dtype), b.to(DEV).to(dtype)
    rsd = None if rs is None else rs.to(DEV)
    tag = f"{pattern}[F={F},H={heads},{plan_tag(F, heads)},{DTYPE_IDS[DTYPES.index(dtype)]}"
    key = f"{plan_tag(F, heads)} {DTYPE_IDS[DTYPES.index(dtype)]}"
    out = {}
    for idx in (torch.int32, torch.int64):
        csr = pattern_csr(pattern, F, heads, idx).to(DEV)
        assert csr.col.dtype == idx and csr.num_rows == a.shape[0]
        out[idx] = run(csr, ad, bd, heads, scale, rsd).clone()
        assert out[idx].dtype == torch.float32
        within(f"{tag},{'i32' if idx == torch.int32 else 'i64'}]", key, out[idx], r64, r32)
    assert torch.equal(out[torch.int32], out[torch.int64])
    assert torch.equal(run(csr, ad, bd, heads, scale, rsd), out[torch.int64])


def offset_view(t, vec):
    """``t`` copied into a view that is as misaligned as its path allows, inside a NaN-filled
    allocation. Vector: columns 4 .. 4 + F of a ``[rows, F + 12]`` buffer (base aligned to 4
    elements and not to 8, row stride divisible by 4 and not by 8). Generic: base one element
    past the allocation's start, row stride ``F + 3``."""
    rows, F = t.shape
    es = t.element_size()
    if vec:
        buf = torch.full((rows, F + 12), float("nan"), device=t.device, dtype=t.dtype)
        v = buf[:, 4:4 + F]
        assert v.stride(0) % 4 == 0 and v.stride(0) % 8 != 0
        assert v.data_ptr() % (4 * es) == 0 and v.data_ptr() % (8 * es) != 0
    else:
        flat = torch.full((rows * (F + 3) + 1,), float("nan"), device=t.device, dtype=t.dtype)
        v = flat[1:].view(rows, F + 3)[:, :F]
        assert v.stride(0) == F + 3 and v.data_ptr() == flat.data_ptr() + es
    v.copy_(t)
    return v


@pytest.mark.parametrize("F,heads", LAYOUT_CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_layouts_are_bitwise_the_contiguous_run(F, heads, dtype):
    a, b, rs, scale, r64, r32 = refs(F, heads, dtype, "boundary")
    ad, bd, rsd = a.to(DEV).to(dtype), b.to(DEV).to(dtype), rs.to(DEV)
    csr = boundary_csr(chunk_of(F, heads), torch.int32).to(DEV)
    vec = plan_of(F, heads)[0] == 4
    assert K.edge_dot_vec_path(F, heads) == vec
    s = run(csr, ad, bd, heads, scale, rsd).clone()
    tag = f"layout[F={F},H={heads},{plan_tag(F, heads)},{DTYPE_IDS[DTYPES.index(dtype)]}]"
    within(tag, f"{plan_tag(F, heads)} {DTYPE_IDS[DTYPES.index(dtype)]}", s, r64, r32)
    av, bv = offset_view(ad, vec), offset_view(bd, vec)
    assert torch.equal(run(csr, av, bv, heads, scale, rsd), s)
    assert torch.equal(run(csr, av, bd, heads, scale, rsd), s)


@functools.lru_cache(maxsize=None)
def deep_refs(nrows, F, mult):
    csr = deep_csr(nrows, torch.int64, mult)
    a, b = values("plain", nrows, F, 300 + F), values("plain", NCOLS, F, 301 + F)
    rs = torch.linspace(0.25, 2.0, nrows)
    r64 = edge_dot_contract(csr.rowptr, csr.col, a, b, 1, 1.0, rs)
    r32 = edge_dot_contract(csr.rowptr, csr.col, a, b, 1, 1.0, rs, dtype=torch.float32)
    return a, b, rs, r64, r32


@pytest.mark.parametrize("nrows", DEEP_ROWS)
@pytest.mark.parametrize("F", [4, 3])
@pytest.mark.parametrize("idx", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("mult", [1, 300])
def test_row_search(nrows, F, idx, mult):
    """Row counts around the powers of 64, nearly all rows empty. ``mult = 1``: one chunk,
    the search must return the first row and the walk cross every empty run; ``mult = 300``:
    chunks of 512 slots start inside the rows at 64^j - 1 .. 64^j + 1."""
    assert chunk_of(F, 1) == 512 and plan_of(F, 1) == ((4, 1, 1) if F == 4 else (1, 4, 1))
    a, b, rs, r64, r32 = deep_refs(nrows, F, mult)
    csr = deep_csr(nrows, idx, mult).to(DEV)
    s = run(csr, a.to(DEV), b.to(DEV), 1, 1.0, rs.to(DEV))
    within(f"deep[rows={nrows},F={F},x{mult},{'i32' if idx == torch.int32 else 'i64'}]",
           f"row search F={F}", s, r64, r32)
