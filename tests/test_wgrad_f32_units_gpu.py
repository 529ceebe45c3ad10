"""The split-M fp32 weight gradient (csrc/kernels/wgrad_f32.hip) slab by slab: the raw
``wgrad_f32`` / ``wgrad_f32_reduce`` ops against fp64, each unit's partial slab on its own
instead of the reduced sum that ``WgradAcc`` shows.

The unit/slab contract of a call with ``P`` units over ``M`` rows (``launch_wgrad``):

* ``rpu = ceil32(ceil(M / P))``; slab ``u`` is ``[A1[a1_rows] | A2]^T G`` over the rows
  ``[u rpu, min((u + 1) rpu, M))``, zero for a unit past ``M``;
* slab ``u`` is added to the old contents when ``u < fresh_from``, else it overwrites them;
* ``col_partials[u]`` = that unit's column sums of G, by the same rule;
* slabs and column rows ``>= P`` are untouched.

Exact cases use integers in [-4, 4] (every product and partial sum an fp32 number, asserted
on the reference by :func:`exact_ok`) and compare bitwise; the unit-normal cases use
``bound`` of test_gat_kernels.py (fp32 products through a bf16 / tf32 path would pass the
integer cases). All 8 ``(K, N)`` instantiations run under both the static and the dynamic
unit schedule.
"""
from __future__ import annotations

import pytest
import torch

from dgraph_amd.ops import f32 as F32
from test_gat_kernels import bound
from test_spmm_f32_variants_gpu import gen, ints

pytestmark = pytest.mark.gpu
DEV = "cuda"

PAIRS = [(K, N) for K in (128, 256) for N in (128, 176, 192, 256)]
SPLITS = ("K|0", "K/2|K/2", "64|K-64", "4|K-4", "K-4|4")
EXTRA = 2  # slabs / column rows past P that a call must leave alone


def split_of(name: str, K: int) -> int:
    """Columns of A1 (the rest belong to A2; K: no A2)."""
    return {"K|0": K, "K/2|K/2": K // 2, "64|K-64": 64, "4|K-4": 4, "K-4|4": K - 4}[name]


def rows_per_unit(M: int, P: int) -> int:
    per = -(-M // P)
    return -(-per // 32) * 32


def unit_bounds(M: int, P: int):
    """Row boundaries of the P units: unit u covers rows [b[u], b[u + 1])."""
    rpu = rows_per_unit(M, P)
    return [min(u * rpu, M) for u in range(P + 1)]


def make_case(K, N, K1, M, P, fresh_from, gather=True, normal=False, key=()):
    """CPU operands of one call: A1 source rows (gathered through ``a1_rows`` with repeats
    when ``gather``), A2 (K - K1 columns, None when K1 = K), G, and the old contents of
    P + EXTRA slabs and column rows."""
    g = gen("wgrad", K, N, K1, M, P, fresh_from, gather, normal, *key)
    val = (lambda s: torch.randn(s, generator=g)) if normal else (lambda s: ints(s, g, -4, 4))
    c = dict(K=K, N=N, K1=K1, M=M, P=P, fresh_from=fresh_from)
    c["A1"] = val((M + 9 if gather else M, K1))
    c["a1_rows"] = torch.randint(0, M + 9, (M,), generator=g) if gather else None
    if gather and M > 1:
        c["a1_rows"][M // 2] = c["a1_rows"][0]  # a repeat
    c["A2"] = val((M, K - K1)) if K1 < K else None
    c["G"] = val((M, N))
    c["old"] = val((P + EXTRA, K, N)) if normal else ints((P + EXTRA, K, N), g, -50, 50)
    c["old_col"] = val((P + EXTRA, N)) if normal else ints((P + EXTRA, N), g, -50, 50)
    return c


def operand(c) -> torch.Tensor:
    """[A1[a1_rows] | A2] of the call, as given (fp32)."""
    a = c["A1"][c["a1_rows"]] if c["a1_rows"] is not None else c["A1"][:c["M"]]
    return a if c["A2"] is None else torch.cat([a, c["A2"]], 1)


def slabs_ref(c, dtype=torch.float64, absolute=False, bounds=None):
    """(slabs [P + EXTRA, K, N], column rows [P + EXTRA, N]) after the call, by the
    contract, evaluated in ``dtype``. ``absolute``: over |terms| (the exactness bound).
    ``bounds``: other unit boundaries than the contract's (test_f32_oracles.py)."""
    ab = (lambda t: t.abs()) if absolute else (lambda t: t)
    a, G = ab(operand(c)).to(dtype), ab(c["G"]).to(dtype)
    slabs, cols = ab(c["old"]).to(dtype).clone(), ab(c["old_col"]).to(dtype).clone()
    b = unit_bounds(c["M"], c["P"]) if bounds is None else bounds
    for u in range(c["P"]):
        m0, m1 = b[u], b[u + 1]
        p, cs = a[m0:m1].t() @ G[m0:m1], G[m0:m1].sum(0)
        if u < c["fresh_from"]:
            p, cs = slabs[u] + p, cols[u] + cs
        slabs[u], cols[u] = p, cs
    return slabs, cols


def exact_ok(c, ref) -> None:
    """Every slab and column sum of the reference is an fp32 number, and the sums of
    |terms| (integers: no fractional bits) stay below 2^24."""
    for r, a in zip(ref, slabs_ref(c, absolute=True)):
        assert torch.equal(r, r.float().double()), "reference is not exact in fp32"
        assert float(a.max()) < 2 ** 24, float(a.max())


def assert_slabs_exact(got, c, ref=None, cols=True) -> None:
    """``got`` = (slabs, column rows) of the call equal the fp64 contract bitwise, slab by
    slab (``cols`` False: the call had no ``col_partials``; its rows must be untouched)."""
    ref = slabs_ref(c) if ref is None else ref
    exact_ok(c, ref)
    want_cols = ref[1] if cols else c["old_col"].double()
    for u in range(c["P"] + EXTRA):
        assert torch.equal(got[0][u].double().cpu(), ref[0][u]), \
            f"slab {u} of {c['P']} (+{EXTRA} untouched), fresh_from {c['fresh_from']}"
        assert torch.equal(got[1][u].double().cpu(), want_cols[u]), f"column sums of unit {u}"


def _wide(t, off=4, extra=4):
    buf = torch.full((t.shape[0], off + t.shape[1] + extra), 77.0, device=DEV)
    view = buf[:, off:off + t.shape[1]]
    view.copy_(t)
    return view


def run_gpu(c, cols=True, wide=False):
    """The call on the GPU: (slabs, column rows) of all P + EXTRA units."""
    from dgraph_amd import _native

    put = (lambda t: None if t is None else _wide(t.to(DEV))) if wide else \
        (lambda t: None if t is None else t.to(DEV))
    slabs, col = c["old"].to(DEV), c["old_col"].to(DEV)
    _native.ops().wgrad_f32(put(c["A1"]), put(c["A2"]),
                            None if c["a1_rows"] is None else c["a1_rows"].to(DEV),
                            put(c["G"]), slabs, c["P"], c["fresh_from"], col if cols else None)
    torch.cuda.synchronize()
    return slabs.cpu(), col.cpu()


def both_schedules(c, cols=True, wide=False, check=None):
    """Run under the static and the dynamic unit schedule: slab-for-slab identical, and
    each checked against the contract."""
    from dgraph_amd import _native

    check = assert_slabs_exact if check is None else check
    ref = slabs_ref(c)
    try:
        res = []
        for dynamic in (0, 1):
            _native.ops().set_f32_sched(-1, dynamic, -1)
            res.append(run_gpu(c, cols, wide))
            check(res[-1], c, ref, cols)
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    finally:
        _native.ops().set_f32_sched(0, 1, 0)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("K,N", PAIRS)
def test_every_instantiation_and_split(K, N, split):
    """All 8 (K, N) kernels x 5 A1 | A2 splits, gathered A1 rows with repeats (they apply
    to the A1 columns only: A2 is read densely), operands as column slices of wider
    buffers, M = 1000 in 7 units with the first 3 accumulated."""
    c = make_case(K, N, split_of(split, K), 1000, 7, 3)
    both_schedules(c, wide=True)


@pytest.mark.parametrize("P", [1, 2, 3, 7])
@pytest.mark.parametrize("M", [1, 31, 32, 33, 64, 65, 1000])
def test_units_and_fresh_from(M, P):
    """Row counts around the 32-row stage and unit counts that leave empty units (M = 33,
    P = 7: five of them), at ``fresh_from`` 0, P // 2 and P, with and without the column
    sums; the (K, N) pair cycles through all eight."""
    K, N = PAIRS[(M + P) % 8]
    for i, ff in enumerate(sorted({0, P // 2, P})):
        c = make_case(K, N, K // 2, M, P, ff, gather=bool((M + i) % 2))
        both_schedules(c, cols=bool((P + i) % 2))


def test_more_units_than_blocks():
    """P = CUs + 3 units of one 32-row stage each (the last one short): under the static
    schedule three blocks run a second unit (the ``it > 0`` path); the dynamic one pulls
    them. Both exact, slab for slab."""
    P = torch.cuda.get_device_properties(0).multi_processor_count + 3
    c = make_case(128, 128, 64, 32 * P - 5, P, P // 2)
    assert rows_per_unit(c["M"], P) == 32
    both_schedules(c)


@pytest.mark.parametrize("P", [1, 15, 16, 17, 33])
@pytest.mark.parametrize("shape", [(128, 128), (1, 176)])
def test_reduce(P, shape):
    """``wgrad_f32_reduce``: the 16-deep batches and their tail, at a slab size that is a
    multiple of 64 and at the ``[P, 1, 176]`` shape of the column sums; the input slabs
    are unchanged afterwards."""
    from dgraph_amd import _native

    g = gen("reduce", P, shape)
    slabs = ints((P,) + shape, g, -1000, 1000)
    ref = slabs.double().sum(0)
    assert torch.equal(ref, ref.float().double()) and float(slabs.abs().sum(0).max()) < 2 ** 24
    d = slabs.to(DEV)
    out = torch.full(shape, 5.0, device=DEV)
    _native.ops().wgrad_f32_reduce(d, out)
    assert torch.equal(out.double().cpu(), ref)
    assert torch.equal(d.cpu(), slabs)


@pytest.mark.parametrize("K,N", [(128, 176), (256, 256)])
def test_acc_short_call_then_longer(K, N):
    """Through ``WgradAcc``: a short call (2 units) followed by a longer one (7 units), so
    ``fresh_from`` falls inside the second call's units. Exact, with the column sums."""
    g = gen("acc", K, N)
    acc = F32.WgradAcc(K, N, DEV, blocks=7, colsum=True)
    ref = torch.zeros(K, N, dtype=torch.float64)
    refc = torch.zeros(N, dtype=torch.float64)
    mag = torch.zeros(K, N, dtype=torch.float64)
    for M in (100, 1000, 40):
        A1, A2, G = ints((M, K // 2), g, -4, 4), ints((M, K // 2), g, -4, 4), ints((M, N), g, -4, 4)
        acc.add(A1.to(DEV), G.to(DEV), A2.to(DEV))
        a = torch.cat([A1, A2], 1).double()
        ref += a.t() @ G.double()
        refc += G.double().sum(0)
        mag += a.abs().t() @ G.double().abs()
    assert float(mag.max()) < 2 ** 24
    assert acc.tiles[0][2].used == 7
    assert torch.equal(acc.result().double().cpu(), ref)
    assert torch.equal(acc.col_result().double().cpu(), refc)


def assert_slabs_bound(got, c, ref=None, cols=True) -> None:
    """Full-mantissa comparison per slab: ``bound(fp64, fp32 matmul on the CPU)``."""
    ref = slabs_ref(c) if ref is None else ref
    ref32 = slabs_ref(c, torch.float32)
    worst = (0.0, 0.0, 0.0)
    for k in (0, 1):
        for u in range(c["P"] + EXTRA):
            err = float((got[k][u].double().cpu() - ref[k][u]).abs().max())
            lim = bound(ref[k][u], ref32[k][u])
            e32 = float((ref32[k][u].double() - ref[k][u]).abs().max())
            if err / lim >= worst[0] / max(worst[1], 1e-30):
                worst = (err, lim, e32)
            assert err <= lim, (("slab", "cols")[k], u, err, lim, e32)
    print(f"wgrad_f32 K={c['K']} N={c['N']} worst err {worst[0]:.3e} bound {worst[1]:.3e} "
          f"fp32-cpu err {worst[2]:.3e}")


@pytest.mark.parametrize("K,N", PAIRS)
def test_unit_normal(K, N):
    """Unit-normal operands, M = 1000 in 7 units, dual form with gathered A1: a
    bf16-truncated operand (2^-9 relative per term) lands far outside ``bound``."""
    c = make_case(K, N, K // 2, 1000, 7, 3, normal=True)
    both_schedules(c, check=assert_slabs_bound)
