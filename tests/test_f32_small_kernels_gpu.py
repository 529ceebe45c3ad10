"""The small kernels of the fp32 step: the 1-bit keep masks (csrc/kernels/bits.hip) against
words packed in plain torch, and the fused cross-entropy / argmax rows
(csrc/kernels/loss.hip) against fp64 ``log_softmax``, at the widths, row counts, strides
and values where a lane-per-float4 / lane-per-column kernel goes wrong.
"""
from __future__ import annotations

import pytest
import torch

from test_gat_kernels import bound
from test_spmm_f32_variants_gpu import SENT, gen, pack_bits, widen

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from dgraph_amd import _native

    return _native.ops()


# ------------------------------------------------------------------------------ keep bits
def keep_values(n: int, F: int, g) -> torch.Tensor:
    """Normal values with 0.0, -0.0 and NaN sprinkled in (all three: "drop"); no
    subnormals."""
    h = torch.randn(n, F, generator=g)
    kind = torch.randint(0, 12, (n, F), generator=g)
    h[kind == 0] = 0.0
    h[kind == 1] = -0.0
    h[kind == 2] = float("nan")
    return h


def assert_bits_equal(got: torch.Tensor, mask: torch.Tensor) -> None:
    """Keep words equal the words packed from the boolean mask, bit for bit."""
    want = pack_bits(mask)
    if not torch.equal(got.cpu(), want):
        bad = torch.nonzero(got.cpu() != want)[0]
        raise AssertionError(f"keep word differs at row {int(bad[0])} word {int(bad[1])}")


@pytest.mark.parametrize("rows_kind", ["all", "list"])
@pytest.mark.parametrize("n", [1, 7, 123])
@pytest.mark.parametrize("F", [32, 64, 96, 160, 256])
def test_row_keep_bits(F, n, rows_kind):
    """``row_keep_bits`` of a column slice (``ld > F``), all rows or a row list with
    repeats. At F = 96 and 160 a row's lanes straddle waves."""
    g = gen("bits", F, n, rows_kind)
    nh = n if rows_kind == "all" else n + 20
    h = keep_values(nh, F, g)
    rows = None if rows_kind == "all" else torch.randint(0, nh, (n,), generator=g)
    if rows is not None and n > 1:
        rows[-1] = rows[0]
    _, hv = widen(h)
    out = torch.full((n + 1, F // 32), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    _ops().row_keep_bits(hv, None if rows is None else rows.to(DEV), out)
    mask = (h if rows is None else h[rows]) > 0
    assert_bits_equal(out[:n], mask)
    assert bool((out[n:] == 0x5A5A5A5A).all())  # no word past the rows


@pytest.mark.parametrize("n", [1, 7, 123])
@pytest.mark.parametrize("F", [32, 64, 96, 160, 256])
def test_apply_keep_bits(F, n):
    """``apply_keep_bits`` in place on a column slice: every row, then a row subset with
    a repeat (bits indexed by the same rows); rows outside the subset and columns outside
    the slice are bitwise unchanged."""
    g = gen("apply", F, n)
    mask = torch.rand(n, F, generator=g) < 0.5
    bits = pack_bits(mask).to(DEV)
    gr = torch.randn(n, F, generator=g)
    buf, gv = widen(gr)
    _ops().apply_keep_bits(gv, bits, None)
    want = torch.where(mask, gr, torch.zeros_like(gr))
    assert torch.equal(gv.cpu(), want)
    b = buf.cpu()
    assert bool((b[:, :4] == SENT).all()) and bool((b[:, 4 + F:] == SENT).all())
    rows = torch.randperm(n, generator=g)[:max(1, n // 3)]
    rows = torch.cat([rows, rows[:1]])
    buf, gv = widen(gr)
    _ops().apply_keep_bits(gv, bits, rows.to(DEV))
    sel = torch.zeros(n, dtype=torch.bool)
    sel[rows] = True
    assert torch.equal(gv.cpu(), torch.where(sel.unsqueeze(1), want, gr))


# ------------------------------------------------------------------------------ loss rows
CS = [1, 2, 63, 64, 65, 128, 129, 255, 256]


def xent_ref(z, rows, y, scale, C, dtype=torch.float64):
    """(row_loss [n], dz [n, C]) from ``log_softmax`` in ``dtype``."""
    ls = torch.log_softmax(z[rows][:, :C].to(dtype), 1)
    loss = -ls.gather(1, y.unsqueeze(1)).squeeze(1)
    dz = ls.exp()
    dz[torch.arange(rows.numel()), y] -= 1.0
    return loss, dz * scale


def assert_xent(loss, dz, z, rows, y, scale, C) -> None:
    """|kernel - fp64| within ``bound`` (fp32 CPU ``log_softmax`` as ``ref32``)."""
    ref, ref32 = xent_ref(z, rows, y, scale, C), xent_ref(z, rows, y, scale, C, torch.float32)
    for name, got, r64, r32 in (("loss", loss, ref[0], ref32[0]), ("dz", dz, ref[1], ref32[1])):
        err = float((got.double().cpu() - r64).abs().max())
        lim = bound(r64, r32)
        print(f"xent_rows {name} C={C} err {err:.3e} bound {lim:.3e} "
              f"fp32-cpu err {float((r32.double() - r64).abs().max()):.3e}")
        assert err <= lim, (name, err, lim)


@pytest.mark.parametrize("amp", [3.0, 150.0], ids=["x3", "x150"])
@pytest.mark.parametrize("n", [1, 5, 150])
@pytest.mark.parametrize("C", CS)
def test_xent_rows(C, n, amp):
    """``xent_rows`` on logits that are a column slice (``ldz > C``), rows with repeats,
    labels including 0 and C - 1, ``dz`` exactly C wide and padded (padding written 0,
    columns beyond the width keep the sentinel). ``x150``: the same logits scaled by 50,
    which overflow without the max subtraction."""
    g = gen("xent", C, n, amp)
    nz = n + 13
    z = torch.randn(nz, C, generator=g) * amp
    rows = torch.randint(0, nz, (n,), generator=g)
    y = torch.randint(0, C, (n,), generator=g)
    y[0] = C - 1
    if n > 1:
        y[1], rows[-1] = 0, rows[0]
    _, zv = widen(z, off=4, extra=8 + (-C) % 4)
    for W in sorted({C, min(256, C + (-C) % 64)}):
        buf, dzv = widen(torch.full((n, W), SENT), off=4, extra=4)
        loss = torch.full((n + 1,), SENT, device=DEV)
        _ops().xent_rows(zv, rows.to(DEV), y.to(DEV), 0.5, dzv, loss, C)
        assert_xent(loss[:n], dzv[:, :C], z, rows, y, 0.5, C)
        assert bool((dzv[:, C:] == 0).all()) and float(loss[n]) == SENT
        b = buf.cpu()
        assert bool((b[:, :4] == SENT).all()) and bool((b[:, 4 + W:] == SENT).all())


TIES = ((3, 67), (5, 70), (10, 65), (70, 200))  # column c sits in lane c % 64


def first_argmax_hits(z, rows, y, C) -> torch.Tensor:
    """uint8 [n]: the first maximum of ``z[rows[i], :C]`` is ``y[i]``."""
    zr = z[rows][:, :C]
    first = (zr == zr.max(1, keepdim=True).values).int().argmax(1)
    return (first == y).to(torch.uint8)


def argmax_case(C: int, n: int = 40):
    """(z, rows, y): ties within one lane's registers (columns 3 and 67), across lanes with
    the lower column in the lower lane (5 and 70) and in the higher lane (10 and 65), an
    all-equal row (index 0 wins) and rows holding ``-inf``; each tie labelled with the
    first (a hit), then the second (a miss), maximum. No NaN."""
    g = gen("argmax", C)
    z = torch.randn(n + 5, C, generator=g) * 3
    ties = [(a, b) for a, b in TIES + ((0, C - 1),) if a < b < C]
    y = torch.randint(0, C, (n,), generator=g)
    rows = torch.randint(0, n + 5, (n,), generator=g)
    rows[:20] = torch.arange(20)
    for k, (a, b) in enumerate(ties):
        for j, label in enumerate((a, b)):
            z[2 * k + j, a] = z[2 * k + j, b] = 50.0 + k
            y[2 * k + j] = label
    z[16] = 1.25  # all equal: index 0
    y[16] = 0
    z[17] = 1.25
    y[17] = C - 1
    z[18] = float("-inf")  # nothing but -inf: index 0
    y[18] = 0
    z[19, : C // 2] = float("-inf")  # the maximum lies behind a run of -inf
    y[19] = int(z[19].argmax()) if C > 1 else 0
    return z, rows, y


def assert_hits(got: torch.Tensor, z, rows, y, C) -> None:
    want = first_argmax_hits(z, rows, y, C)
    assert torch.equal(got.cpu(), want), torch.nonzero(got.cpu() != want).flatten()
    assert C == 1 or (0 < int(want.sum()) < want.numel())  # both outcomes occur


@pytest.mark.parametrize("C", CS)
def test_argmax_hits(C):
    """``argmax_hits`` with the first-maximum rule on :func:`argmax_case`, logits as a
    column slice; the entry past the rows keeps its sentinel."""
    z, rows, y = argmax_case(C)
    n = rows.numel()
    _, zv = widen(z, off=4, extra=8 + (-C) % 4)
    hit = torch.full((n + 1,), 9, dtype=torch.uint8, device=DEV)
    _ops().argmax_hits(zv, rows.to(DEV), y.to(DEV), hit, C)
    assert_hits(hit[:n], z, rows, y, C)
    assert int(hit[n]) == 9
