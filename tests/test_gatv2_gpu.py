"""The fused GATv2 attention kernels (csrc/kernels/gatv2_f32.hip, called through
``_native.ops().gatv2_*_f32`` directly), the ``gatv2_attention`` op and the
``CommAwareGATv2Conv`` layer on the GPU against the fp64 evaluation of their contract
(tests/test_gatv2.py), at every ``(C, heads)`` instantiation and both column index types.

Pattern and inputs: see tests/test_gatv2.py (37 rows over 41 local + 19 halo sources with
rows of degree 0, 1, LPR +- 1 and a 301-entry hub; score scales 0.5 and 40). The backward
kernels get ``c`` from the fp64 oracle, rounded to fp32; ``da`` is the fp64 host sum of the
rows of ``da_part``.

Bound per compared array: ``max(2e-5, 8 err32) max(1, max|fp64|)`` with ``err32`` the error of
the same formula evaluated in fp32 on the CPU (``test_gat_kernels.bound``) — nothing is taken
from the kernels' own output. Largest ``error / bound`` seen on an MI355X (a record, not an
input to the bound; the tests print every figure before asserting):

    gatv2_fwd      out 0.174   stat_m 0.006   stat_l 0.159
    gatv2_bwd_dst  dl 0.692    da 0.405 (fp64 host sum of da_part)
    gatv2_bwd_src  dr 0.348
    the op         out 0.174   dl 0.262   dr 0.208   da 0.211
    empty sides    0.207
    the layer      out 0.005   dx 0.007   dx_j 0.008   att 0.027   parameters 0.038 or less
                   (min |pre| of the layer test's fp64 values: 2.9e-5)
"""
from __future__ import annotations

import pytest
import torch

from test_dot_attn import CIN, ND, NS, _edges
from test_gat_kernels import HS, LS, N, PAIRS, R, bound, pattern, transpose
from test_gatv2 import OUTPUTS, SCALES, SLOPE, _dense_gatv2, case, gatv2_contract, oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.25e9  # what output buffers hold outside the slices the kernels may write
RATIOS: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _native_and_record():
    from dgraph_amd import _native

    assert _native.load(), "native library missing"
    yield
    for k in sorted(RATIOS):
        print(f"\n[gatv2] largest error / bound, {k}: {RATIOS[k]:.3f}", end="")
    print()


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
    key = name if tag.startswith("kernels") else f"{tag.split()[0]}:{name}"
    RATIOS[key] = max(RATIOS.get(key, 0.0), err / bd)
    print(f"{tag} {name}: err {err:.3e} bound {bd:.3e} ratio {err / bd:.3f}")
    assert err <= bd, (tag, name, err, bd)


class _Buffers:
    """Device operands of one run of the three kernels. ``wide``: every feature array is
    the upper column half of a [rows, 2C] buffer and every per-head array the upper half of
    a [rows, 2 heads] buffer (one head: column 2 of a [rows, 4] buffer); inputs hold NaN
    outside their slice, outputs ``SENT``. Outputs hold NaN inside on entry. ``att`` and
    ``da_part`` are contiguous by contract (``da_part`` NaN on entry)."""

    def __init__(self, d, c64, idx, two, beta, wide=False):
        rowptr, col, _ = pattern()
        t_rowptr, t_col = transpose(rowptr, col, N)
        self.heads, self.two, self.beta, self.wide = d["heads"], two, beta, wide
        self.held = []  # (name, wide buffer, slice) of the outputs
        self.rowptr, self.col = rowptr.to(DEV), col.to(idx).to(DEV)
        self.t_rowptr, self.t_col = t_rowptr.to(DEV), t_col.to(idx).to(DEV)
        ns = LS if two else N
        self.ns = ns
        self.l, self.g = self._in(d["l"]), self._in(d["g"])
        self.r = self._in(d["r"][:ns])
        self.r2 = self._in(d["r"][ns:]) if two else None
        self.a = d["a"].to(DEV)
        self.c = self._in(c64.float())
        C, Hh = d["C"], d["heads"]
        self.out = self._out("out", R, C)
        if beta != 0:
            self.out.copy_(d["out0"])
        self.m, self.lin = self._out("stat_m", R, Hh), self._out("stat_l", R, Hh)
        self.dl = self._out("dl", R, C)
        self.dr = self._out("dr", ns, C)
        if two:
            self.dr2 = self._out("dr2", HS, C)
        self.P = _ops().gatv2_da_parts(R, C)
        assert 1 < self.P <= (R + 3) // 4  # more than one workgroup, far fewer rows than R
        self.da_part = torch.full((self.P, C), float("nan"), device=DEV)

    def _slice(self, rows, cols, fill):
        if not self.wide:
            return torch.full((rows, cols), fill, device=DEV), None, None
        if cols == 1:
            buf, sl = torch.full((rows, 4), fill, device=DEV), slice(2, 3)
        else:
            buf, sl = torch.full((rows, 2 * cols), fill, device=DEV), slice(cols, 2 * cols)
        return buf[:, sl], buf, sl

    def _in(self, t):
        v, _, _ = self._slice(t.shape[0], t.shape[1], float("nan"))
        v.copy_(t)
        return v

    def _out(self, name, rows, cols):
        v, buf, sl = self._slice(rows, cols, SENT)
        v.fill_(float("nan"))
        if buf is not None:
            self.held.append((name, buf, sl))
        return v

    def run(self):
        ops, h = _ops(), self.heads
        ops.gatv2_fwd_f32(self.rowptr, self.col, self.l, self.r, self.r2, self.ns, self.a,
                          self.out, self.beta, self.m, self.lin, h, SLOPE)
        ops.gatv2_bwd_dst_f32(self.rowptr, self.col, self.l, self.r, self.r2, self.ns, self.a,
                              self.m, self.lin, self.g, self.c, self.dl, self.da_part, h, SLOPE)
        # the source side: local rows, then the halo rows over the tail of the transposed
        # row pointer (as ops/gatv2.py calls it)
        ops.gatv2_bwd_src_f32(self.t_rowptr[:self.ns + 1], self.t_col, self.l, self.g, self.r,
                              self.a, self.m, self.lin, self.c, self.dr, h, SLOPE)
        if self.two:
            ops.gatv2_bwd_src_f32(self.t_rowptr[LS:], self.t_col, self.l, self.g, self.r2,
                                  self.a, self.m, self.lin, self.c, self.dr2, h, SLOPE)
        torch.cuda.synchronize()
        res = {"out": self.out, "stat_m": self.m, "stat_l": self.lin, "dl": self.dl,
               "dr": self.dr, "da_part": self.da_part}
        if self.two:
            res["dr"] = torch.cat([self.dr, self.dr2])
        return {k: v.clone() for k, v in res.items()}

    def assert_outside_untouched(self):
        for name, buf, sl in self.held:
            keep = torch.ones(buf.shape[1], dtype=torch.bool, device=DEV)
            keep[sl] = False
            rest = buf[:, keep]
            assert torch.equal(rest, torch.full_like(rest, SENT)), name


def _check(tag, got, C, heads, s, beta):
    r64, r32 = oracle(C, heads, s, beta)
    rowptr = pattern()[0]
    full = rowptr[1:] > rowptr[:-1]
    # every row of da_part is written (NaN on entry); da is its fp64 host sum
    assert torch.isfinite(got["da_part"]).all(), (tag, "da_part")
    got = dict(got, da=got["da_part"].double().sum(0))
    for k in OUTPUTS:
        if k == "stat_m":  # (an empty row's maximum is not part of the contract)
            _compare(tag, k, got[k][full.to(DEV)], r64[k][full], r32[k][full])
        else:
            _compare(tag, k, got[k], r64[k], r32[k])
    assert (got["stat_l"][(~full).to(DEV)] == 0).all()
    if beta == 0:
        assert (got["out"][(~full).to(DEV)] == 0).all()
    assert (got["dl"][(~full).to(DEV)] == 0).all()


def _run_twice(C, heads, s, idx, two, beta, wide=False):
    """Two runs on fresh buffers: bitwise equal (fixed summation orders, no atomics),
    ``da_part`` included."""
    d, c64 = case(C, heads, s), oracle(C, heads, s, beta)[0]["c"]
    a, b = _Buffers(d, c64, idx, two, beta, wide), _Buffers(d, c64, idx, two, beta, wide)
    ra, rb = a.run(), b.run()
    assert "da_part" in ra
    for k in ra:
        assert torch.equal(ra[k].view(torch.int32), rb[k].view(torch.int32)), k
    a.assert_outside_untouched()
    return ra


@pytest.mark.parametrize("idx", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("C,heads", PAIRS)
def test_gatv2_kernels_vs_fp64(C, heads, s, idx):
    """Forward, destination side, source side (local rows, halo rows) at one instantiation:
    with a second source split at 41 and with all 60 rows local; ``beta = 0`` into a
    NaN-filled ``out`` and ``beta = 0.5`` onto ``out`` on entry."""
    for two in (True, False):
        for beta in (0.0, 0.5):
            got = _run_twice(C, heads, s, idx, two, beta)
            _check(f"kernels C={C} heads={heads} s={s} beta={beta} "
                   f"{'two' if two else 'one'}-source", got, C, heads, s, beta)


@pytest.mark.parametrize("idx", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("C,heads", PAIRS)
def test_gatv2_kernels_wide_operands(C, heads, idx):
    """Every operand a column slice of a wider buffer (row strides 2C and 2 heads / 4):
    inputs hold NaN outside the slices; outputs keep their sentinel there bitwise. One and
    two sources, ``beta`` 0 and 0.5, both scales between them."""
    for two, beta, s in ((True, 0.0, 0.5), (False, 0.5, 40.0)):
        got = _run_twice(C, heads, s, idx, two, beta, wide=True)
        _check(f"kernels wide C={C} heads={heads} s={s} beta={beta}", got, C, heads, s, beta)


def test_gatv2_kernels_empty_shapes():
    ops = _ops()
    C, Hh = 64, 2
    f = lambda *shape: torch.randn(*shape, device=DEV)  # noqa: E731
    i32 = torch.empty(0, dtype=torch.int32, device=DEV)
    e = lambda n: torch.empty(0, n, device=DEV)  # noqa: E731
    l, g, r, a = f(3, C), f(3, C), f(5, C), f(C)
    assert ops.gatv2_da_parts(0, C) == 0
    # no destination rows: returns, writes nothing — also with every operand empty
    rp0 = torch.zeros(1, dtype=torch.long, device=DEV)
    outs = [torch.full((3, n), SENT, device=DEV) for n in (C, Hh, Hh, C, C)]
    out, m, li, dl, dr = outs
    ops.gatv2_fwd_f32(rp0, i32, l, r, None, 5, a, out, 0.0, m, li, Hh, SLOPE)
    ops.gatv2_bwd_dst_f32(rp0, i32, l, r, None, 5, a, f(3, Hh), f(3, Hh), g, f(3, Hh), dl,
                          e(C), Hh, SLOPE)
    ops.gatv2_bwd_src_f32(rp0, i32, l, g, r, a, f(3, Hh), f(3, Hh), f(3, Hh), dr, Hh, SLOPE)
    ops.gatv2_fwd_f32(rp0, i32, e(C), e(C), None, 0, a, e(C), 0.0, e(Hh), e(Hh), Hh, SLOPE)
    ops.gatv2_bwd_dst_f32(rp0, i32, e(C), e(C), e(C), 0, a, e(Hh), e(Hh), e(C), e(Hh), e(C),
                          e(C), Hh, SLOPE)
    ops.gatv2_bwd_src_f32(rp0, i32, e(C), e(C), e(C), a, e(Hh), e(Hh), e(Hh), e(C), Hh, SLOPE)
    torch.cuda.synchronize()
    for t in outs:
        assert torch.equal(t, torch.full_like(t, SENT))
    # 37 rows, no entries: with source rows (a launch) and without any (no launch)
    rp = torch.zeros(R + 1, dtype=torch.long, device=DEV)
    l, g, base = f(R, C), f(R, C), f(R, C)
    P = ops.gatv2_da_parts(R, C)
    for rr in (r, e(C)):
        for beta in (0.5, 0.0):
            out = base.clone() if beta else torch.full((R, C), float("nan"), device=DEV)
            m, li = f(R, Hh), torch.full((R, Hh), SENT, device=DEV)
            ops.gatv2_fwd_f32(rp, i32, l, rr, None, rr.shape[0], a, out, beta, m, li, Hh, SLOPE)
            assert torch.equal(out, base * beta if beta else torch.zeros_like(base))
            assert torch.equal(li, torch.zeros_like(li))
        dl = torch.full((R, C), SENT, device=DEV)
        dap = torch.full((P, C), float("nan"), device=DEV)
        ops.gatv2_bwd_dst_f32(rp, i32, l, rr, None, rr.shape[0], a, m, li, g, f(R, Hh), dl, dap,
                              Hh, SLOPE)
        assert torch.equal(dl, torch.zeros_like(dl)) and torch.equal(dap, torch.zeros_like(dap))
    # 5 source rows of in-degree 0: with destination rows (a launch) and without (no launch)
    rp5 = torch.zeros(6, dtype=torch.long, device=DEV)
    for ll, gg, n in ((l, g, R), (e(C), e(C), 0)):
        dr = torch.full((5, C), SENT, device=DEV)
        ops.gatv2_bwd_src_f32(rp5, i32, ll, gg, r, a, f(n, Hh), f(n, Hh), f(n, Hh), dr, Hh,
                              SLOPE)
        assert torch.equal(dr, torch.zeros_like(dr))


@pytest.mark.parametrize("side", ["no local sources", "0-row second source"])
def test_gatv2_kernels_empty_source_sides(side):
    """``nsplit = 0`` with a 0-row first source (every column, the padding slots' included,
    reads the second source) and a second source of 0 rows (treated as absent): the three
    kernels against the contract on the same pattern."""
    ops = _ops()
    C, heads, s = 64, 2, 0.5
    rowptr, col, _ = pattern()
    d = case(C, heads, s)
    if side == "no local sources":
        cl, ns, r1, r2 = col % HS, 0, d["r"][:0], d["r"][LS:]
    else:
        cl, ns, r1, r2 = col, N, d["r"], d["r"][:0]
    args = (rowptr, cl, d["l"], r1, r2, ns, d["a"], d["g"], heads, SLOPE, 0.0, None)
    r64, r32 = gatv2_contract(*args), gatv2_contract(*args, dtype=torch.float32)
    nsrc = r1.shape[0] + r2.shape[0]
    t_rowptr, t_col = transpose(rowptr, cl, nsrc)
    dv = lambda t: t.to(DEV)  # noqa: E731
    l, g, a, x1, x2 = dv(d["l"]), dv(d["g"]), dv(d["a"]), dv(r1), dv(r2)
    rp, ci = dv(rowptr), dv(cl.to(torch.int32))
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)  # noqa: E731
    out, m, li, dl = nan(R, C), nan(R, heads), nan(R, heads), nan(R, C)
    dap = nan(ops.gatv2_da_parts(R, C), C)
    c = dv(r64["c"].float())
    ops.gatv2_fwd_f32(rp, ci, l, x1, x2, ns, a, out, 0.0, m, li, heads, SLOPE)
    ops.gatv2_bwd_dst_f32(rp, ci, l, x1, x2, ns, a, m, li, g, c, dl, dap, heads, SLOPE)
    big = x2 if side == "no local sources" else x1
    dr = nan(nsrc, C)
    ops.gatv2_bwd_src_f32(dv(t_rowptr), dv(t_col.to(torch.int32)), l, g, big, a, m, li, c, dr,
                          heads, SLOPE)
    # the empty side's own source-side call: no rows, returns
    ops.gatv2_bwd_src_f32(dv(t_rowptr[:1]) if ns == 0 else dv(t_rowptr[N:]),
                          dv(t_col.to(torch.int32)), l, g, x1 if ns == 0 else x2, a, m, li, c,
                          torch.empty(0, C, device=DEV), heads, SLOPE)
    torch.cuda.synchronize()
    got = {"out": out, "stat_l": li, "dl": dl, "dr": dr, "da": dap.double().sum(0)}
    for k, v in got.items():
        _compare(f"empty {side}", k, v, r64[k], r32[k])


# ----------------------------------------------------- contract checks (bindings_gatv2.cpp)
def _valid_args(C, heads):
    rowptr, col, _ = pattern()
    f = lambda *shape: torch.randn(*shape, device=DEV)  # noqa: E731
    return dict(rowptr=rowptr.to(DEV), col=col.to(torch.int32).to(DEV), xd=f(R, C), xs=f(N, C),
                xs2=None, nsplit=N, att=f(C), out=f(R, C), beta=0.5, stat_m=f(R, heads),
                stat_l=f(R, heads), heads=heads, slope=SLOPE)


_FWD = ("rowptr", "col", "xd", "xs", "xs2", "nsplit", "att", "out", "beta", "stat_m", "stat_l",
        "heads", "slope")


def _violate(what):
    if what == "C=96":
        return _valid_args(96, 2)
    if what == "heads=3":
        return _valid_args(64, 3)
    if what == "(C,heads)=(64,16)":
        return _valid_args(64, 16)
    A = _valid_args(64, 2)
    if what == "xs offset by one float":
        flat = torch.empty(N * 64 + 4, device=DEV)
        A["xs"] = flat[1:1 + N * 64].view(N, 64).normal_()
        assert A["xs"].data_ptr() % 16 == 4
    elif what == "xs row stride not divisible by 4":
        A["xs"] = torch.randn(N, 66, device=DEV)[:, :64]
    elif what == "xs with a column stride":
        A["xs"] = torch.randn(N, 128, device=DEV)[:, ::2]
    elif what == "stat_l row stride differs from stat_m's":
        A["stat_l"] = torch.randn(R, 4, device=DEV)[:, :2]
    elif what == "nsplit larger than xs's row count":
        A.update(xs2=torch.randn(HS, 64, device=DEV), nsplit=N + 1)
    elif what == "float64 xd":
        A["xd"] = A["xd"].double()
    elif what == "att offset by one float":
        A["att"] = torch.randn(68, device=DEV)[1:65]
        assert A["att"].data_ptr() % 16 == 4
    elif what == "att strided":
        A["att"] = torch.randn(128, device=DEV)[::2]
    elif what == "att [heads, D]":
        A["att"] = A["att"].view(2, 32)
    elif what == "att on the CPU":
        A["att"] = A["att"].cpu()
    elif what == "xd with fewer rows than the pattern":
        A["xd"] = A["xd"][:R - 1]
    else:
        raise KeyError(what)
    return A


@pytest.mark.parametrize("what", [
    "C=96", "heads=3", "(C,heads)=(64,16)", "xs offset by one float",
    "xs row stride not divisible by 4", "xs with a column stride",
    "stat_l row stride differs from stat_m's", "nsplit larger than xs's row count",
    "float64 xd", "att offset by one float", "att strided", "att [heads, D]", "att on the CPU",
    "xd with fewer rows than the pattern"])
def test_gatv2_contract_checks_raise_before_launch(what):
    A = _violate(what)
    before = {k: A[k].clone() for k in ("out", "stat_m", "stat_l")}
    with pytest.raises(RuntimeError):
        _ops().gatv2_fwd_f32(*[A[k] for k in _FWD])
    torch.cuda.synchronize()
    for k, t in before.items():
        assert torch.equal(A[k], t), k


def test_gatv2_da_part_shape_is_checked():
    ops = _ops()
    C, Hh = 64, 2
    rowptr, col, _ = pattern()
    f = lambda *shape: torch.randn(*shape, device=DEV)  # noqa: E731
    P = ops.gatv2_da_parts(R, C)
    assert P == 3 and ops.gatv2_da_parts(R, 256) == 10  # ceil(ceil(R / rows per wave) / 4)
    assert ops.gatv2_da_parts(1 << 24, 128) == ops.gatv2_da_parts(1 << 30, 128) == 4096
    dl = f(R, C)
    before = dl.clone()
    for bad in (f(P + 1, C), f(P, C + 4), f(P, 2 * C)[:, :C]):
        with pytest.raises(RuntimeError):
            ops.gatv2_bwd_dst_f32(rowptr.to(DEV), col.to(torch.int32).to(DEV), f(R, C), f(N, C),
                                  None, N, f(C), f(R, Hh), f(R, Hh), f(R, C), f(R, Hh), dl, bad,
                                  Hh, SLOPE)
    torch.cuda.synchronize()
    assert torch.equal(dl, before)


# -------------------------------------------------------------------------- the autograd op
def _run_op(dev, dtype, C, heads, s, halo, one_buffer=False):
    """``gatv2_attention`` forward + backward. ``one_buffer``: xd and xs are the column
    halves of one [rows, 2C] buffer, as the layer hands them in."""
    from dgraph_amd.ops import gatv2_attention
    from dgraph_amd.ops.gat import GatPattern

    rowptr, col, _ = pattern()
    d = case(C, heads, s)
    ns, nh = (LS, HS) if halo else (N, 0)
    pat = GatPattern(rowptr.to(dev), col.to(dev), ns, nh)
    a = d["a"].view(heads, -1).to(dev, dtype).requires_grad_()
    rh = d["r"][ns:].to(dev, dtype).requires_grad_() if halo else None
    if one_buffer:
        buf = torch.zeros(ns, 2 * C)
        buf[:R, :C], buf[:, C:] = d["l"], d["r"][:ns]
        buf = buf.to(dev, dtype).requires_grad_()
        l, r = buf[:R, :C], buf[:, C:]
    else:
        l = d["l"].to(dev, dtype).requires_grad_()
        r = d["r"][:ns].to(dev, dtype).requires_grad_()
    out = gatv2_attention(l, r, a, pat, rh, heads=heads, negative_slope=SLOPE)
    if one_buffer and dev != "cpu":  # the kernels read the halves in place: no copy was made
        saved = out.grad_fn.saved_tensors
        assert saved[0].data_ptr() == l.data_ptr() and saved[1].data_ptr() == r.data_ptr()
        assert saved[0].stride(0) == 2 * C and saved[1].stride(0) == 2 * C
    ins = ([buf] if one_buffer else [l, r]) + [a] + ([rh] if halo else [])
    grads = list(torch.autograd.grad(out, ins, d["g"].to(dev, dtype)))
    if one_buffer:
        gb = grads.pop(0)
        assert int(torch.count_nonzero(gb[R:, :C])) == 0
        grads = [gb[:R, :C], gb[:, C:]] + grads
    dr = torch.cat([grads[1], grads[3]]) if halo else grads[1]
    return {"out": out.detach(), "dl": grads[0], "dr": dr, "da": grads[2].reshape(-1)}


@pytest.mark.parametrize("halo", [True, False], ids=["halo", "no_halo"])
@pytest.mark.parametrize("C,heads,s", [(C, h, 0.5) for C, h in PAIRS] +
                         [(64, 8, 40.0), (128, 1, 40.0), (256, 4, 40.0)])
def test_gatv2_attention_op_gpu_vs_contract(C, heads, s, halo):
    """Forward and all four gradients (``dxd``, ``dxs``, ``dxsh``, ``datt``)."""
    r64, r32 = oracle(C, heads, s, 0.0)
    got = _run_op(DEV, torch.float32, C, heads, s, halo)
    got2 = _run_op(DEV, torch.float32, C, heads, s, halo)
    tag = f"op C={C} heads={heads} s={s} halo={halo}"
    for k in got:
        assert torch.equal(got[k], got2[k]), k
        _compare(tag, k, got[k], r64[k], r32[k])


@pytest.mark.parametrize("halo", [True, False], ids=["halo", "no_halo"])
def test_gatv2_attention_op_reads_buffer_halves_in_place(halo):
    C, heads, s = 128, 4, 0.5
    r64, r32 = oracle(C, heads, s, 0.0)
    got = _run_op(DEV, torch.float32, C, heads, s, halo, one_buffer=True)
    for k in got:
        _compare(f"op one-buffer halo={halo}", k, got[k], r64[k], r32[k])


def test_gatv2_attention_op_rejects_unsupported_gpu_inputs():
    from dgraph_amd.ops import gatv2_attention
    from dgraph_amd.ops.gat import GatPattern

    rowptr, col, _ = pattern()
    pat = GatPattern(rowptr.to(DEV), col.to(DEV), N, 0)
    f = lambda n, C, dt=torch.float32: torch.randn(n, C, device=DEV, dtype=dt)  # noqa: E731
    for C, heads, dt in ((96, 2, torch.float32), (64, 16, torch.float32),
                         (64, 2, torch.float16), (64, 2, torch.float64),
                         (64, 2, torch.bfloat16)):
        with pytest.raises(ValueError, match="64, 128, 256"):
            gatv2_attention(f(R, C, dt), f(N, C, dt), f(1, C, dt)[0], pat, heads=heads)


@pytest.mark.parametrize("side", ["no destination rows", "no local sources", "no halo",
                                  "no entries"])
def test_gatv2_attention_op_empty_sides(side):
    """Legal empty sides of a rank's relation: forward + backward run, agree with the CPU op
    and give zero gradients where nothing is attended to."""
    from dgraph_amd.ops import gatv2_attention
    from dgraph_amd.ops.gat import GatPattern

    C, heads = 64, 2
    rowptr, col, _ = pattern()
    d = case(C, heads, 0.5)
    if side == "no destination rows":
        rp, cl, ns, nh, nq = torch.zeros(1, dtype=torch.long), col[:0], 5, 3, 0
    elif side == "no local sources":
        rp, cl, ns, nh, nq = rowptr, col % HS, 0, HS, R
    elif side == "no entries":
        rp, cl, ns, nh, nq = torch.zeros(R + 1, dtype=torch.long), col[:0], 0, 0, R
    else:
        rp, cl, ns, nh, nq = rowptr, col, N, 0, R

    def run(dev, dtype):
        pat = GatPattern(rp.to(dev), cl.to(dev), ns, nh)
        mk = lambda t: t.to(dev, dtype).clone().requires_grad_()  # noqa: E731
        l, r, a = mk(d["l"][:nq]), mk(d["r"][:ns]), mk(d["a"])
        rh = mk(d["r"][ns:ns + nh]) if nh else None
        out = gatv2_attention(l, r, a, pat, rh, heads=heads)
        ins = [t for t in (l, r, a, rh) if t is not None]
        return [out.detach()] + list(torch.autograd.grad(out, ins, d["g"][:nq].to(dev, dtype)))

    ref, got = run("cpu", torch.float64), run(DEV, torch.float32)
    for a, b in zip(got, ref):
        assert a.shape == b.shape
        _compare(f"empty {side}", "all", a, b, b.float())
    if side in ("no destination rows", "no entries"):
        assert all(int(torch.count_nonzero(t)) == 0 for t in got)
    if side == "no local sources":
        assert got[2].shape == (0, C)


# --------------------------------------------------------------------------------- the layer
LAYER_SEED = 1


def test_gatv2_conv_gpu_vs_cpu():
    """``CommAwareGATv2Conv`` (in 6, out 64, 2 heads, residual) forward + backward on the GPU
    against the same layer on the CPU at fp64, W = 1; the fp32 error of the bound is the
    dense per-edge formulation's at fp32.

    The layer's ``pre`` comes out of an fp32 GEMM, so its LeakyReLU branch could differ from
    fp64's where ``|pre|`` is within the GEMM's rounding: on the CPU fp64 values
    ``min |pre| >= 1e-5`` over every (edge, channel) is asserted first — about ten times the
    fp32 error of a K = 6 product of O(1) values (the seed is chosen so that it holds)."""
    import copy

    from dgraph_amd.data.hetero import build_relation_graph, get_vertex_offsets
    from dgraph_amd.models import CommAwareGATv2Conv

    edges = _edges()
    offs = {0: get_vertex_offsets(ND, 1), 1: get_vertex_offsets(NS, 1)}
    torch.manual_seed(0)
    base = CommAwareGATv2Conv(CIN, 64, heads=2, residual=True, hetero=True)
    with torch.no_grad():
        base.bias.normal_()
    gen = torch.Generator().manual_seed(LAYER_SEED)
    xd, xs, w = (torch.randn(n, c, generator=gen) for n, c in ((ND, CIN), (NS, CIN), (ND, 64)))
    l64 = copy.deepcopy(base).double()
    with torch.no_grad():
        pre = l64.lin_dst(xd.double())[edges[1]] + l64.lin_src(xs.double())[edges[0]]
    print(f"layer min |pre| {float(pre.abs().min()):.3e}")
    assert float(pre.abs().min()) >= 1e-5

    def run(dev, dtype, dense=False):
        layer = copy.deepcopy(base).to(dev, dtype)
        a, b = (t.to(dev, dtype).requires_grad_() for t in (xd, xs))
        if dense:
            out = _dense_gatv2(layer, a, b, edges)
        else:
            out = layer(a, build_relation_graph(edges, 1, 0, offs, 0, 1).to(dev), x_j=b)
        grads = torch.autograd.grad(out, [a, b] + list(layer.parameters()), w.to(dev, dtype))
        return [out.detach()] + list(grads)

    ref64, ref32 = run("cpu", torch.float64), run("cpu", torch.float32, dense=True)
    got = run(DEV, torch.float32)
    names = ["out", "dx", "dx_j"] + [n for n, _ in base.named_parameters()]
    assert len(names) == len(got) == 10 and "att" in names
    for n, a, b, c in zip(names, got, ref64, ref32):
        _compare("layer", n, a, b, c)


def test_gatv2_conv_gpu_one_gemm_for_both_projections():
    """One input, unshared weights: [l | r] is one [N, 2C] buffer and the op reads its halves
    in place; against the layer's CPU fp64 evaluation."""
    import copy

    from dgraph_amd.data.hetero import build_relation_graph, get_vertex_offsets
    from dgraph_amd.models import CommAwareGATv2Conv

    gen = torch.Generator().manual_seed(6)
    edges = torch.unique(torch.randint(0, NS, (2, 80), generator=gen), dim=1)
    offs = {0: get_vertex_offsets(NS, 1)}
    torch.manual_seed(0)
    base = CommAwareGATv2Conv(CIN, 64, heads=2)
    x, w = torch.randn(NS, CIN, generator=gen), torch.randn(NS, 64, generator=gen)
    l64 = copy.deepcopy(base).double()
    with torch.no_grad():
        pre = l64.lin_dst(x.double())[edges[1]] + l64.lin_src(x.double())[edges[0]]
    assert float(pre.abs().min()) >= 1e-5

    def run(dev, dtype, dense=False):
        layer = copy.deepcopy(base).to(dev, dtype)
        a = x.to(dev, dtype).requires_grad_()
        if dense:
            out = _dense_gatv2(layer, a, a, edges)
        else:
            out = layer(a, build_relation_graph(edges, 0, 0, offs, 0, 1).to(dev))
        grads = torch.autograd.grad(out, [a] + list(layer.parameters()), w.to(dev, dtype))
        return [out.detach()] + list(grads)

    ref64, ref32 = run("cpu", torch.float64), run("cpu", torch.float32, dense=True)
    got = run(DEV, torch.float32)
    names = ["out", "dx"] + [n for n, _ in base.named_parameters()]
    for n, a, b, c in zip(names, got, ref64, ref32):
        _compare("layer-one-gemm", n, a, b, c)
