"""The fused graph-attention kernels (csrc/kernels/gat_f32.hip, called through
``_native.ops().gat_*_f32`` directly) and the edge softmax (csrc/kernels/edge_softmax.hip)
against the fp64 evaluation of their contract (tests/test_gat_kernels.py), at every
``(C, heads)`` instantiation and both column index types.

The pattern (37 destination rows over 41 local + 19 halo sources, about 1300 entries) has
rows of degree 0, 1, LPR-1, LPR, LPR+1 and a 301-entry hub next to an empty row in one wave,
partial last row groups, and sources of in-degree 0, 1..15 and above 64 in both parts; the
CPU file asserts all of that. Scores at scale 0.5 (every edge carries at least 2e-4 of its
row: one dropped, doubled or misattributed edge shows at ten times the tolerance) and 30
(``exp`` overflows in fp32 without the max subtraction).

Bound per compared array: ``max(2e-5, 8 err32) max(1, max|fp64|)`` with ``err32`` the error of
the same formula evaluated in fp32 on the CPU (``test_gat_kernels.bound``) — nothing is taken
from the kernels' own output. Largest ``error / bound`` seen on an MI355X (a record, not an
input to the bound; the tests print every figure before asserting):

    gat_fwd      out 0.072   stat_m 0.003   stat_l 0.089
    gat_bwd_dst  c 0.055     gsd 0.472 (C=64, 2 heads, scale 30; 0.15 or less elsewhere)
    gat_bwd_src  gss 0.089   gz 0.082
    the op       out 0.041   gz 0.086   gzh 0.064   gsd 0.154   ga 0.087
    edge softmax ds 0.046 (alpha: atol = rtol = 1e-5, as tests/test_kernels_gpu.py)
"""
from __future__ import annotations

import pytest
import torch

from test_gat_kernels import (HS, LS, N, OUTPUTS, PAIRS, R, SCALES, SLOPE, bound, case,
                              edge_softmax_contract, oracle, pattern, row_degrees, transpose)

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
        print(f"\n[gat-kernels] largest error / bound, {k}: {RATIOS[k]:.3f}", end="")
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
    the upper column half of a [rows, 2C] buffer and every score / statistics array column
    2 of a [rows, 4] buffer (one-head calls: ``ld = 2C``, ``lds = 4``); inputs hold NaN
    outside their slice, outputs ``SENT``. Outputs hold NaN inside on entry."""

    def __init__(self, d, idx, two, beta, wide=False):
        rowptr, col, _ = pattern()
        t_rowptr, t_col = transpose(rowptr, col, N)
        self.heads, self.two, self.beta, self.wide = d["heads"], two, beta, wide
        self.held = []  # (name, wide buffer, slice) of the outputs
        self.rowptr, self.col = rowptr.to(DEV), col.to(idx).to(DEV)
        self.t_rowptr, self.t_col = t_rowptr.to(DEV), t_col.to(idx).to(DEV)
        ns = LS if two else N
        self.ns = ns
        self.x, self.ss = self._in(d["x"][:ns]), self._in(d["ss"][:ns])
        self.x2 = self._in(d["x"][ns:]) if two else None
        self.ss2 = self._in(d["ss"][ns:]) if two else None
        self.sd, self.g = self._in(d["sd"]), self._in(d["g"])
        self.a_src = d["a_src"].to(DEV)
        C, Hh = d["C"], d["heads"]
        self.out = self._out("out", R, C)
        if beta != 0:
            self.out.copy_(d["out0"])
        self.m, self.l = self._out("stat_m", R, Hh), self._out("stat_l", R, Hh)
        self.c, self.gsd = self._out("c", R, Hh), self._out("gsd", R, Hh)
        self.gz, self.gss = self._out("gz", ns, C), self._out("gss", ns, Hh)
        if two:
            self.gz2, self.gss2 = self._out("gz2", HS, C), self._out("gss2", HS, Hh)

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
        ops.gat_fwd_f32(self.rowptr, self.col, self.x, self.x2, self.ns, self.ss, self.ss2,
                        self.sd, self.out, self.beta, self.m, self.l, h, SLOPE)
        ops.gat_bwd_dst_f32(self.rowptr, self.col, self.x, self.x2, self.ns, self.ss,
                            self.ss2, self.sd, self.m, self.l, self.g, self.c, self.gsd, h,
                            SLOPE)
        # the source side: local rows, then the halo rows over the tail of the transposed
        # row pointer (as ops/gat.py calls it)
        ops.gat_bwd_src_f32(self.t_rowptr[:self.ns + 1], self.t_col, self.g, self.x, self.ss,
                            self.sd, self.m, self.l, self.c, self.a_src, self.gz, self.gss, h,
                            SLOPE)
        if self.two:
            ops.gat_bwd_src_f32(self.t_rowptr[LS:], self.t_col, self.g, self.x2, self.ss2,
                                self.sd, self.m, self.l, self.c, self.a_src, self.gz2,
                                self.gss2, h, SLOPE)
        torch.cuda.synchronize()
        res = {"out": self.out, "stat_m": self.m, "stat_l": self.l, "c": self.c,
               "gsd": self.gsd, "gz": self.gz, "gss": self.gss}
        if self.two:
            res["gz"] = torch.cat([self.gz, self.gz2])
            res["gss"] = torch.cat([self.gss, self.gss2])
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
    for k in OUTPUTS:
        if k == "stat_m":  # (an empty row's maximum is not part of the contract)
            _compare(tag, k, got[k][full.to(DEV)], r64[k][full], r32[k][full])
        else:
            _compare(tag, k, got[k], r64[k], r32[k])
    assert (got["stat_l"][(~full).to(DEV)] == 0).all()
    if beta == 0:
        assert (got["out"][(~full).to(DEV)] == 0).all()


def _run_twice(d, idx, two, beta, wide=False):
    """Two runs on fresh buffers: bitwise equal (fixed summation orders, no atomics)."""
    a, b = _Buffers(d, idx, two, beta, wide), _Buffers(d, idx, two, beta, wide)
    ra, rb = a.run(), b.run()
    for k in ra:
        assert torch.equal(ra[k].view(torch.int32), rb[k].view(torch.int32)), k
    a.assert_outside_untouched()
    return ra


@pytest.mark.parametrize("idx", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("C,heads", PAIRS)
def test_gat_kernels_vs_fp64(C, heads, s, idx):
    """Forward, destination side, source side (local rows, halo rows) at one instantiation:
    with a second source split at 41 and with all 60 rows local; ``beta = 0`` into a
    NaN-filled ``out``."""
    d = case(C, heads, s)
    for two in (True, False):
        got = _run_twice(d, idx, two, 0.0)
        _check(f"kernels C={C} heads={heads} s={s} {'two' if two else 'one'}-source", got, C,
               heads, s, 0.0)


@pytest.mark.parametrize("beta", [0.0, 1.0, 0.5])
@pytest.mark.parametrize("C,heads", [(64, 2), (128, 4), (256, 8)])
def test_gat_fwd_beta(C, heads, beta):
    """``out = beta out + ...``: 0 overwrites a NaN-filled ``out`` without reading it; 1
    and 0.5 against ``out`` on entry."""
    d = case(C, heads, 0.5)
    b = _Buffers(d, torch.int32, True, beta)
    if beta == 0:
        assert torch.isnan(b.out).all()
    got = b.run()
    r64, r32 = oracle(C, heads, 0.5, beta)
    _compare(f"kernels beta={beta} C={C}", "out", got["out"], r64["out"], r32["out"])


@pytest.mark.parametrize("two", [True, False], ids=["two-source", "one-source"])
@pytest.mark.parametrize("C", [64, 128, 256])
def test_gat_kernels_strided_one_head_slices(C, two):
    """The layout of the one-head column passes: features are column slices of [rows, 2C]
    buffers, scores and statistics one column of [rows, 4] arrays (``lds = 4``, one head).
    Inputs hold NaN outside the slices; outputs keep their sentinel there bitwise."""
    got = _run_twice(case(C, 1, 0.5), torch.int32, two, 0.0, wide=True)
    _check(f"kernels strided C={C}", got, C, 1, 0.5, 0.0)


def test_gat_kernels_empty_shapes():
    ops = _ops()
    C, Hh = 64, 2
    f = lambda *shape: torch.randn(*shape, device=DEV)  # noqa: E731
    i32 = torch.empty(0, dtype=torch.int32, device=DEV)
    x, ss, sd, g, a = f(5, C), f(5, Hh), f(3, Hh), f(3, C), f(C)
    # no rows: returns, writes nothing
    rp0 = torch.zeros(1, dtype=torch.long, device=DEV)
    outs = [torch.full((3, n), SENT, device=DEV) for n in (C, Hh, Hh, Hh, Hh, C, Hh)]
    out, m, l, c, gsd, gz, gss = outs
    ops.gat_fwd_f32(rp0, i32, x, None, 5, ss, None, sd, out, 0.0, m, l, Hh, SLOPE)
    ops.gat_bwd_dst_f32(rp0, i32, x, None, 5, ss, None, sd, f(3, Hh), f(3, Hh), g, c, gsd, Hh,
                        SLOPE)
    ops.gat_bwd_src_f32(rp0, i32, g, x, ss, sd, f(3, Hh), f(3, Hh), f(3, Hh), a, gz, gss, Hh,
                        SLOPE)
    torch.cuda.synchronize()
    for t in outs:
        assert torch.equal(t, torch.full_like(t, SENT))
    # 37 rows, no entries
    rp = torch.zeros(R + 1, dtype=torch.long, device=DEV)
    sd, g, base = f(R, Hh), f(R, C), f(R, C)
    for beta in (1.0, 0.0):
        out = base.clone() if beta else torch.full((R, C), float("nan"), device=DEV)
        m, l = f(R, Hh), torch.full((R, Hh), SENT, device=DEV)
        ops.gat_fwd_f32(rp, i32, x, None, 5, ss, None, sd, out, beta, m, l, Hh, SLOPE)
        assert torch.equal(out, base if beta else torch.zeros_like(base))
        assert torch.equal(l, torch.zeros_like(l))
    c, gsd = (torch.full((R, Hh), SENT, device=DEV) for _ in range(2))
    ops.gat_bwd_dst_f32(rp, i32, x, None, 5, ss, None, sd, m, l, g, c, gsd, Hh, SLOPE)
    assert torch.equal(c, torch.zeros_like(c)) and torch.equal(gsd, torch.zeros_like(gsd))
    # no entries seen from the source side: 5 source rows of in-degree 0
    gz, gss = torch.full((5, C), SENT, device=DEV), torch.full((5, Hh), SENT, device=DEV)
    ops.gat_bwd_src_f32(torch.zeros(6, dtype=torch.long, device=DEV), i32, g, x, ss, sd, m, l,
                        c, a, gz, gss, Hh, SLOPE)
    assert torch.equal(gz, torch.zeros_like(gz)) and torch.equal(gss, torch.zeros_like(gss))


# ------------------------------------------------------- contract checks (bindings_gat.cpp)
_ORDER = {
    "fwd": ("rowptr", "col", "x", "x2", "nsplit", "ss", "ss2", "sd", "out", "beta", "stat_m",
            "stat_l", "heads", "slope"),
    "bwd_dst": ("rowptr", "col", "x", "x2", "nsplit", "ss", "ss2", "sd", "stat_m", "stat_l",
                "g", "c", "gsd", "heads", "slope"),
    "bwd_src": ("t_rowptr", "t_col", "g", "x", "ss", "sd", "stat_m", "stat_l", "c", "a_src",
                "gz", "gss", "heads", "slope"),
}
_WRITTEN = {"fwd": ("out", "stat_m", "stat_l"), "bwd_dst": ("c", "gsd"),
            "bwd_src": ("gz", "gss")}


def _valid_args(C, heads):
    """Every operand of the three ops at (C, heads), valid for the test pattern."""
    rowptr, col, _ = pattern()
    t_rowptr, t_col = transpose(rowptr, col, N)
    f = lambda *shape: torch.randn(*shape, device=DEV)  # noqa: E731
    return dict(rowptr=rowptr.to(DEV), col=col.to(torch.int32).to(DEV),
                t_rowptr=t_rowptr.to(DEV), t_col=t_col.to(torch.int32).to(DEV),
                x=f(N, C), x2=None, nsplit=N, ss=f(N, heads), ss2=None, sd=f(R, heads),
                out=f(R, C), beta=1.0, stat_m=f(R, heads), stat_l=f(R, heads).abs(),
                g=f(R, C), c=f(R, heads), gsd=f(R, heads), a_src=f(C), gz=f(N, C),
                gss=f(N, heads), heads=heads, slope=SLOPE)


def _offset_by_one_float(t):
    flat = torch.empty(t.numel() + 4, device=DEV)
    v = flat[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _violate(what, op):
    if what == "C=96":
        return _valid_args(96, 2)
    if what == "heads=3":
        return _valid_args(64, 3)
    if what == "(C,heads)=(64,16)":
        return _valid_args(64, 16)
    A = _valid_args(64, 2)
    if what == "x offset by one float":
        key = "g" if op == "bwd_src" else "x"
        A[key] = _offset_by_one_float(A[key])
    elif what == "sd row stride differs from ss's":
        A["sd"] = torch.randn(R, 4, device=DEV)[:, :2]
    elif what == "x2 without ss2":
        A.update(x2=A["x"][LS:].clone(), nsplit=LS)
    elif what == "nsplit larger than x's row count":
        A.update(x2=torch.randn(HS, 64, device=DEV), ss2=torch.randn(HS, 2, device=DEV),
                 nsplit=N + 1)
    else:
        raise KeyError(what)
    return A


_SHARED = ["C=96", "heads=3", "(C,heads)=(64,16)", "x offset by one float",
           "sd row stride differs from ss's"]
_TWO_SOURCE = ["x2 without ss2", "nsplit larger than x's row count"]


@pytest.mark.parametrize("op,what", [(op, w) for op in ("fwd", "bwd_dst") for w in
                                     _SHARED + _TWO_SOURCE] + [("bwd_src", w) for w in _SHARED])
def test_gat_contract_checks_raise_before_launch(op, what):
    fn = getattr(_ops(), f"gat_{op}_f32")
    A = _violate(what, op)
    before = {k: A[k].clone() for k in _WRITTEN[op]}
    with pytest.raises(RuntimeError):
        fn(*[A[k] for k in _ORDER[op]])
    torch.cuda.synchronize()
    for k, t in before.items():
        assert torch.equal(A[k], t), k
    # the stream is still good: a valid call gives the right answer
    got = _Buffers(case(64, 2, 0.5), torch.int32, True, 0.0).run()
    _check("contract valid-call", got, 64, 2, 0.5, 0.0)


# -------------------------------------------------------------------------- the autograd op
@pytest.mark.parametrize("halo", [True, False], ids=["zh_static", "no_halo"])
@pytest.mark.parametrize("C,heads,hp", [(C, h, False) for C, h in PAIRS] +
                         [(128, 2, True), (256, 2, True), (256, 4, True)])
def test_gat_relation_op_gpu_vs_cpu(monkeypatch, C, heads, hp, halo):
    """``ops.gat.gat_relation_into`` on the GPU (whole rows; one pass per head where
    D = C / heads is a kernel width) against its CPU path in fp64: forward and the
    gradients with respect to z, zh_static, sd and a_src."""
    import dgraph_amd.ops.gat as G

    monkeypatch.setattr(G, "HEAD_PASSES", hp)
    rowptr, col, _ = pattern()
    d = case(C, heads, 0.5)
    nsplit, nh = (LS, HS) if halo else (N, 0)

    def run(dev, dtype, fn):
        pat = G.GatPattern(rowptr.to(dev), col.to(dev), nsplit, nh)
        mk = lambda t: t.to(dev, dtype).clone().requires_grad_()  # noqa: E731
        z, sd, a = mk(d["x"][:nsplit]), mk(d["sd"] * 2), mk(d["a_src"].view(heads, C // heads))
        zh = mk(d["x"][nsplit:]) if halo else None
        out = fn(z, zh, sd, a, d["out0"].to(dev, dtype), pat)
        ins = [t for t in (z, zh, sd, a) if t is not None]
        grads = torch.autograd.grad(out, ins, d["g"].to(dev, dtype))
        names = [n for n, t in zip(("gz", "gzh", "gsd", "ga"), (z, zh, sd, a)) if t is not None]
        return {"out": out.detach(), **dict(zip(names, grads))}

    def op(z, zh, sd, a, base, pat):
        return G.gat_relation_into(z, sd, a, base.clone(), pat, zh_static=zh)

    ref64 = run("cpu", torch.float64, op)
    ref32 = run("cpu", torch.float32, lambda z, zh, sd, a, base, pat:
                base + G._reference(z, zh, sd, a, pat))
    got = run(DEV, torch.float32, op)
    got2 = run(DEV, torch.float32, op)
    tag = f"op C={C} heads={heads} head_passes={hp} halo={halo}"
    assert got.keys() == ref64.keys()
    for k in got:
        assert ref64[k].dtype == torch.float64
        assert torch.equal(got[k], got2[k]), k
        _compare(tag, k, got[k], ref64[k], ref32[k])


# ------------------------------------------------------------------------- the edge softmax
@pytest.mark.parametrize("H", [1, 2, 3, 5, 8, 16, 33, 64])
def test_edge_softmax_vs_fp64(H):
    """Every lanes-per-edge instantiation (1 .. 64), rows of several wave steps at each,
    empty rows, and three entries raised by 80 inside long rows."""
    from dgraph_amd.ops import kernels as K

    rowptr = torch.zeros(R + 1, dtype=torch.long)
    rowptr[1:] = torch.cumsum(row_degrees(), 0)
    gen = torch.Generator().manual_seed(H)
    s = torch.randn(int(rowptr[-1]), H, generator=gen) * 5
    for r, k in ((17, 5), (14, 100), (11, 62)):
        s[rowptr[r] + k] += 80.0  # large scores: the max subtraction must keep this finite
    g = torch.randn(s.shape, generator=gen)
    rp = rowptr.to(DEV)
    a = K.edge_softmax_fwd(rp, s.to(DEV))
    assert torch.equal(a, K.edge_softmax_fwd(rp, s.to(DEV)))
    a64, d64 = edge_softmax_contract(rowptr, s, g)
    _, d32 = edge_softmax_contract(rowptr, s, g, dtype=torch.float32)
    assert torch.isfinite(a).all()
    torch.testing.assert_close(a.double().cpu(), a64, atol=1e-5, rtol=1e-5)
    ds = K.edge_softmax_bwd(rp, a, g.to(DEV))
    assert torch.equal(ds, K.edge_softmax_bwd(rp, a, g.to(DEV)))
    _compare(f"edge_softmax H={H}", "ds", ds, d64, d32)
