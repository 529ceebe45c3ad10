"""The fused GATv2 kernels with edge features (csrc/kernels/gatv2_edge_f32.hip, called through
``_native.ops().gatv2_edge_*_f32`` directly), ``gatv2_attention(..., edge=)`` and
``CommAwareGATv2Conv(edge_dim=)`` on the GPU against the fp64 dense reference of
tests/test_gatv2_edge.py, at every ``(C, heads)`` instantiation and both column index types.

Bound per compared array: ``max(2e-5, 8 err32) max(1, max|fp64|)`` with ``err32`` the error of
the same formula evaluated in fp32 on the CPU (``test_gat_kernels.bound``); nothing is taken
from the kernels' own output. The backward kernels get ``c`` from the oracle, rounded to fp32.
Largest ``error / bound`` seen on an MI355X (a record, not an input; every test prints its
figures before asserting):

    gatv2_edge_fwd      out 0.126   stat_m 0.006   stat_l 0.131
    gatv2_edge_bwd_dst  dl 0.472    dee 0.227      w 0.126      da 0.449
    gatv2_edge_bwd_src  dr 0.178
    wide operands       0.027 or less
    the op              out 0.116   dl 0.169   dr 0.123   da 0.108   dee 0.143
    empty sides         0.032
    the layer           lin_dst.weight 0.023, everything else 0.013 or less
"""
from __future__ import annotations

import pytest
import torch

from test_gat_kernels import HS, LS, N, PAIRS, R, bound, pattern, transpose
from test_gatv2 import SCALES, SLOPE, case
from test_gatv2_edge import E, _layer_run, _op, edge_rows, oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.25e9  # what output buffers hold outside the slices the kernels may write
NAN = float("nan")
RATIOS: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _native_and_record():
    from dgraph_amd import _native

    assert _native.load(), "native library missing"
    yield
    print("".join(f"\n[gatv2-edge] largest error / bound, {k}: {v:.3f}"
                  for k, v in sorted(RATIOS.items())))


def _ops():
    from dgraph_amd import _native

    return _native.ops()


def _compare(tag, name, got, ref64, ref32):
    """|got - fp64| against :func:`bound`; prints the figures, records the ratio."""
    got = got.detach().double().cpu()
    assert got.shape == ref64.shape, (tag, name, got.shape, ref64.shape)
    assert torch.isfinite(got).all(), (tag, name)
    bd = bound(ref64, ref32)
    err = float((got - ref64.double()).abs().max()) if got.numel() else 0.0
    key = f"{tag.split()[0]}:{name}"
    RATIOS[key] = max(RATIOS.get(key, 0.0), err / bd)
    print(f"{tag} {name}: err {err:.3e} bound {bd:.3e} ratio {err / bd:.3f}")
    assert err <= bd, (tag, name, err, bd)


def _t_slot(col):
    """The forward slot of each entry of ``transpose(rowptr, col, N)``."""
    return torch.sort(col.long(), stable=True).indices


def _run(C, heads, s, idx, two, beta, wide=False):
    """One run of the three kernels on fresh buffers -> (results, untouched-check). ``wide``:
    every 2-D operand is the upper column half of a twice as wide buffer; inputs hold NaN
    outside their half, outputs ``SENT``. Outputs hold NaN inside on entry."""
    d, ee, c64 = case(C, heads, s), edge_rows(C, heads, s), oracle(C, heads, s)[0]["c"]
    rowptr, col, _ = pattern()
    t_rowptr, t_col = transpose(rowptr, col, N)
    held = []

    def buf(rows, cols, fill, src=None):
        whole = torch.full((rows, 2 * cols if wide else cols), fill, device=DEV)
        v = whole[:, cols:] if wide else whole
        if src is None:
            held.append(whole)
            v.fill_(NAN)
        else:
            v.copy_(src)
        return v

    ns = LS if two else N
    rp, cl, trp = rowptr.to(DEV), col.to(idx).to(DEV), t_rowptr.to(DEV)
    tcl, tsl = t_col.to(idx).to(DEV), _t_slot(col).to(idx).to(DEV)
    l, g, r = buf(R, C, NAN, d["l"]), buf(R, C, NAN, d["g"]), buf(ns, C, NAN, d["r"][:ns])
    r2 = buf(HS, C, NAN, d["r"][ns:]) if two else None
    eev, c, att = buf(E, C, NAN, ee), buf(R, heads, NAN, c64.float()), d["a"].to(DEV)
    out, m, lst = buf(R, C, SENT), buf(R, heads, SENT), buf(R, heads, SENT)
    if beta:
        out.copy_(d["out0"])
    dl, dee, w, dr = buf(R, C, SENT), buf(E, C, SENT), buf(E, heads, SENT), buf(ns, C, SENT)
    da_part = torch.full((_ops().gatv2_da_parts(R, C), C), NAN, device=DEV)
    ops = _ops()
    ops.gatv2_edge_fwd_f32(rp, cl, l, r, r2, ns, eev, att, out, beta, m, lst, heads, SLOPE)
    ops.gatv2_edge_bwd_dst_f32(rp, cl, l, r, r2, ns, eev, att, m, lst, g, c, dl, dee, w,
                               da_part, heads, SLOPE)
    # the source side: local rows, then the halo rows over the tail of the transposed row
    # pointer (as ops/gatv2.py calls it)
    ops.gatv2_edge_bwd_src_f32(trp[:ns + 1], tcl, tsl, g, w, dee, dr, heads)
    if two:
        dr2 = buf(HS, C, SENT)
        ops.gatv2_edge_bwd_src_f32(trp[LS:], tcl, tsl, g, w, dee, dr2, heads)
        dr = torch.cat([dr, dr2])
    torch.cuda.synchronize()
    assert torch.isfinite(da_part).all()  # every partial row written
    for whole in held if wide else ():
        rest = whole[:, :whole.shape[1] // 2]
        assert torch.equal(rest, torch.full_like(rest, SENT))
    return {"out": out, "stat_m": m, "stat_l": lst, "dl": dl, "dr": dr, "dee": dee,
            "alpha": w, "da": da_part.cpu().double().sum(0)}


def _check(tag, C, heads, s, idx, two, beta, wide=False):
    got, again = (_run(C, heads, s, idx, two, beta, wide) for _ in range(2))
    for k in got:  # fixed summation orders, no atomics
        assert torch.equal(got[k].view(torch.int64 if k == "da" else torch.int32),
                           again[k].view(torch.int64 if k == "da" else torch.int32)), k
    r64, r32 = (dict(r, out=beta * case(C, heads, s)["out0"].to(r["out"].dtype) + r["out"])
                for r in oracle(C, heads, s))
    rowptr = pattern()[0]
    full = rowptr[1:] > rowptr[:-1]
    empty = (~full).to(DEV)
    for k in got:  # (a slot of dee / w never written is still NaN: not finite)
        if k == "stat_m":  # (an empty row's maximum is not part of the contract)
            _compare(tag, k, got[k][full.to(DEV)], r64[k][full], r32[k][full])
        else:
            _compare(tag, k, got[k], r64[k], r32[k])
    assert (got["stat_l"][empty] == 0).all() and (got["dl"][empty] == 0).all()
    assert beta or (got["out"][empty] == 0).all()


@pytest.mark.parametrize("idx", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("C,heads", PAIRS)
def test_gatv2_edge_kernels_vs_fp64(C, heads, s, idx):
    for two in (True, False):
        for beta in (0.0, 0.5):
            _check(f"kernels C={C} heads={heads} s={s} beta={beta} two={two}", C, heads, s, idx,
                   two, beta)


@pytest.mark.parametrize("two", [True, False], ids=["two-source", "one-source"])
@pytest.mark.parametrize("C,heads", [(64, 1), (128, 4), (256, 2), (256, 8)])
def test_gatv2_edge_kernels_wide_operands(C, heads, two):
    _check(f"wide C={C} heads={heads}", C, heads, 0.5, torch.int32, two, 0.0, wide=True)


def _args(C, heads, R_=R, N_=N, E_=E, pat=True):
    """Valid arguments of the three ops (random values; zero row pointers without ``pat``)."""
    rowptr, col, _ = pattern()
    t_rowptr, t_col = transpose(rowptr, col, N)
    f = lambda *shape: torch.randn(*shape, device=DEV)  # noqa: E731
    z = lambda n: torch.zeros(n, dtype=torch.long, device=DEV)  # noqa: E731
    i32 = lambda t: t[:E_].to(torch.int32).to(DEV)  # noqa: E731
    P = _ops().gatv2_da_parts(R_, C) if C % 4 == 0 and C <= 256 else 1
    return dict(rowptr=rowptr.to(DEV) if pat else z(R_ + 1), col=i32(col), xd=f(R_, C),
                xs=f(N_, C), xs2=None, nsplit=N_, ee=f(E_, C), att=f(C), out=f(R_, C), beta=0.0,
                stat_m=f(R_, heads), stat_l=f(R_, heads), g=f(R_, C), c=f(R_, heads),
                dxd=f(R_, C), dee=f(E_, C), w=f(E_, heads), da_part=f(P, C),
                t_rowptr=t_rowptr.to(DEV) if pat else z(N_ + 1), t_col=i32(t_col),
                t_slot=i32(_t_slot(col)), dxs=f(N_, C), heads=heads, slope=SLOPE)


_CALLS = {
    "fwd": ("gatv2_edge_fwd_f32", "rowptr col xd xs xs2 nsplit ee att out beta stat_m stat_l "
            "heads slope", "out stat_m stat_l"),
    "dst": ("gatv2_edge_bwd_dst_f32", "rowptr col xd xs xs2 nsplit ee att stat_m stat_l g c dxd "
            "dee w da_part heads slope", "dxd dee w da_part"),
    "src": ("gatv2_edge_bwd_src_f32", "t_rowptr t_col t_slot g w dee dxs heads", "dxs"),
}


def _call(op, A):
    name, args, outs = _CALLS[op]
    before = {k: A[k].clone() for k in outs.split()}
    getattr(_ops(), name)(*[A[k] for k in args.split()])
    torch.cuda.synchronize()
    return before


@pytest.mark.parametrize("R_,N_", [(0, 5), (0, 0), (R, 5), (R, 0)])
def test_gatv2_edge_kernels_empty_shapes(R_, N_):
    """No rows; rows without entries (``E = 0``: nothing launched); source rows of in-degree
    0 with and without destination rows. Only the empty-row results are written."""
    A = _args(64, 2, R_, N_, 0, pat=False)
    for op, zeroed in (("fwd", ("out", "stat_l")), ("dst", ("dxd", "da_part")), ("src", ("dxs",))):
        before = _call(op, A)
        for k, t in before.items():
            nothing = (op != "src" and R_ == 0) or k not in zeroed
            assert torch.equal(A[k], t if nothing else torch.zeros_like(t)), (op, k)


@pytest.mark.parametrize("what,refused", [
    ("ee with E - 1 rows", "fwd dst"), ("ee offset by one float", "fwd dst"),
    ("dee short", "dst src"), ("w with the wrong column count", "dst src"),
    ("t_slot of the other integer dtype", "src"), ("t_slot one short", "src"),
    ("C=96", "fwd dst src"), ("heads=3", "fwd dst src")])
def test_gatv2_edge_contract_checks_raise_before_launch(what, refused):
    A = _args(96 if what == "C=96" else 64, 3 if what == "heads=3" else 2)
    if what == "ee with E - 1 rows":
        A["ee"] = A["ee"][:-1]
    elif what == "ee offset by one float":
        A["ee"] = torch.randn(E * 64 + 4, device=DEV)[1:1 + E * 64].view(E, 64)
        assert A["ee"].data_ptr() % 16 == 4
    elif what == "dee short":
        A["dee"] = A["dee"][:-1]
    elif what == "w with the wrong column count":
        A["w"] = torch.randn(E, 4, device=DEV)
    elif what == "t_slot of the other integer dtype":
        A["t_slot"] = A["t_slot"].long()
    elif what == "t_slot one short":
        A["t_slot"] = A["t_slot"][:-1]
    for op in refused.split():
        before = {k: A[k].clone() for k in _CALLS[op][2].split()}
        with pytest.raises(RuntimeError):
            _call(op, A)
        torch.cuda.synchronize()
        assert all(torch.equal(A[k], t) for k, t in before.items()), op


# -------------------------------------------------------------------------- the autograd op
@pytest.mark.parametrize("ns,nh", [(LS, HS), (N, 0)], ids=["halo", "no_halo"])
@pytest.mark.parametrize("C,heads,s", [(C, h, 0.5) for C, h in PAIRS] +
                         [(64, 8, 40.0), (128, 1, 40.0), (256, 4, 40.0)])
def test_gatv2_attention_edge_op_gpu_vs_cpu(C, heads, s, ns, nh):
    """Forward + the five gradients against the CPU fp64 op; ``xd`` / ``xs`` as the halves of
    one [N, 2C] buffer in one case; a repeated call is bitwise equal."""
    d, ee, r32 = case(C, heads, s), edge_rows(C, heads, s), oracle(C, heads, s)[1]
    kw = dict(halves=(C, heads, nh) == (128, 4, 0))
    ref64 = _op(d, ee, heads, ns, nh, **kw)
    got, again = (_op(d, ee, heads, ns, nh, torch.float32, DEV, **kw) for _ in range(2))
    for k in got:
        assert ref64[k].dtype == torch.float64 and torch.equal(got[k], again[k]), k
        _compare(f"op C={C} heads={heads} s={s} halo={nh}", k, got[k], ref64[k], r32[k])


@pytest.mark.parametrize("side", ["no destination rows", "no local sources", "no halo"])
def test_gatv2_attention_edge_op_empty_sides_and_dtypes(side):
    """The legal empty sides of a rank against the CPU op; bf16 rows and non-fp32 edges raise."""
    rowptr, col, _ = pattern()
    pat, ns, nh = {"no destination rows": ((rowptr[:1], col[:0]), 5, 3),
                   "no local sources": ((rowptr, col % HS), 0, HS),
                   "no halo": ((rowptr, col), N, 0)}[side]
    d, ee = case(64, 2, 0.5), edge_rows(64, 2, 0.5)
    got = _op(d, ee, 2, ns, nh, torch.float32, DEV, pat=pat)
    for k, b in _op(d, ee, 2, ns, nh, pat=pat).items():
        _compare(f"empty {side}", k, got[k], b, b.float())
    if side == "no destination rows":
        assert all(int(torch.count_nonzero(t)) == 0 for t in got.values())
        assert got["dee"].shape == (0, 64) and got["dr"].shape == (8, 64)
    from dgraph_amd.ops import gatv2_attention
    from dgraph_amd.ops.gat import GatPattern

    gp = GatPattern(rowptr.to(DEV), col.to(DEV), N, 0)
    for rows, edt in ((torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32)):
        with pytest.raises(ValueError, match="edge dtype"):
            gatv2_attention(d["l"].to(DEV, rows), d["r"].to(DEV, rows), d["a"].to(DEV), gp,
                            heads=2, allow_bf16=True, edge=ee.to(DEV, edt))


# --------------------------------------------------------------------------------- the layer
def test_gatv2_conv_edge_gpu_vs_cpu():
    """``CommAwareGATv2Conv(6, 64, heads=2, residual=True, hetero=True, edge_dim=7)`` forward +
    backward on the GPU against the same layer on the CPU at fp64, W = 1; ``err32`` is the
    dense per-edge formulation's at fp32. ``pre`` comes out of fp32 GEMMs, so its LeakyReLU
    branch could differ from fp64's where ``|pre|`` is within their rounding: the fp64 values
    have ``min |pre| >= 1e-5`` (asserted first; the seed of ``_layer_run`` makes it hold)."""
    layer, ref64, min_pre = _layer_run(2, cout=64)
    print(f"layer min |pre| {min_pre:.3e}")
    assert min_pre >= 1e-5
    ref32 = _layer_run(2, cout=64, dtype=torch.float32, dense=True)[1]
    got = _layer_run(2, cout=64, dtype=torch.float32, dev=DEV)[1]
    names = ["out", "dx", "dx_j", "dedge_attr"] + [n for n, _ in layer.named_parameters()]
    assert len(names) == len(got) == 12 and "lin_edge.weight" in names
    for n, a, b, c in zip(names, got, ref64, ref32):
        _compare("layer", n, a, b, c)
