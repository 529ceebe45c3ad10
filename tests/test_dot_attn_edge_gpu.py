"""The fused dot-product attention kernels with edge features
(csrc/kernels/dot_attn_edge_f32.hip, called through ``_native.ops().dot_attn_edge_*_f32``
directly), ``dot_attention(..., edge=)`` and ``CommAwareTransformerConv(edge_dim=)`` on the
GPU against the fp64 evaluation of their contract (tests/test_dot_attn_edge.py), at every
``(C, heads)`` instantiation and both column index types.

Pattern and inputs: see tests/test_dot_attn_edge.py (37 rows over 41 local + 19 halo sources
with rows of degree 0, 1, LPR +- 1 and a 301-entry hub; score scales 0.5 and 40; one edge row
per CSR slot). The backward kernels get ``c`` from the fp64 oracle, rounded to fp32.

Bound per compared array: ``max(2e-5, 8 err32) max(1, max|fp64|)`` with ``err32`` the error of
the same formula evaluated in fp32 on the CPU (``test_gat_kernels.bound``) — nothing is taken
from the kernels' own output. Largest ``error / bound`` seen on an MI355X (a record, not an
input to the bound; the tests print every figure before asserting):

    dot_attn_edge_fwd      out 0.135   stat_m 0.007   stat_l 0.172
    dot_attn_edge_bwd_dst  dq 0.393    dee 0.401      w 0.399
    dot_attn_edge_bwd_src  dk 0.718    dv 0.200
    the op                 out 0.099   dq 0.103   dk 0.098   dv 0.200   dee 0.093
    empty sides            0.030
    the layer              out 0.005   dx 0.012   dx_j 0.008   dedge_attr 0.013
                           parameters 0.010 or less

The largest figure, dk 0.718, is C = 256 with 8 heads at scale 40 (error 3.6e-4, bound
5.1e-4); every other dk ratio is below 0.5.
"""
from __future__ import annotations

import pytest
import torch

from test_dot_attn import ND, NS, SCALES, _edges, case
from test_dot_attn_edge import (E, OUTPUTS, _dense_edge_transformer, _edge_attr, edge_rows,
                                oracle)
from test_gat_kernels import HS, LS, N, PAIRS, R, bound, pattern, transpose

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
        print(f"\n[dot-attn-edge] largest error / bound, {k}: {RATIOS[k]:.3f}", end="")
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


def _t_slot(col):
    """The forward slot of each entry of ``transpose(rowptr, col, N)``."""
    return torch.sort(col.long(), stable=True).indices


class _Buffers:
    """Device operands of one run of the three kernels. ``wide``: every feature array (``ee``
    and ``dee`` included) is the upper column half of a [rows, 2C] buffer, ``w`` the upper half
    of a [E, 4 heads] buffer and every per-head array the upper half of a [rows, 2 heads]
    buffer (one head: column 2 of a [rows, 4] buffer); inputs hold NaN outside their slice,
    outputs ``SENT``. Outputs hold NaN inside on entry."""

    def __init__(self, d, ee, c64, idx, two, beta, wide=False):
        rowptr, col, _ = pattern()
        t_rowptr, t_col = transpose(rowptr, col, N)
        self.heads, self.two, self.beta, self.wide = d["heads"], two, beta, wide
        self.scale = d["scale"]
        self.held = []  # (name, wide buffer, slice) of the outputs
        self.rowptr, self.col = rowptr.to(DEV), col.to(idx).to(DEV)
        self.t_rowptr, self.t_col = t_rowptr.to(DEV), t_col.to(idx).to(DEV)
        self.t_slot = _t_slot(col).to(idx).to(DEV)
        ns = LS if two else N
        self.ns = ns
        self.q, self.g = self._in(d["q"]), self._in(d["g"])
        self.k, self.v = self._in(d["k"][:ns]), self._in(d["v"][:ns])
        self.k2 = self._in(d["k"][ns:]) if two else None
        self.v2 = self._in(d["v"][ns:]) if two else None
        self.ee = self._in(ee)
        self.c = self._in(c64.float())
        C, Hh = d["C"], d["heads"]
        self.out = self._out("out", R, C)
        if beta != 0:
            self.out.copy_(d["out0"])
        self.m, self.l = self._out("stat_m", R, Hh), self._out("stat_l", R, Hh)
        self.dq = self._out("dq", R, C)
        self.dee, self.w = self._out("dee", E, C), self._out("w", E, 2 * Hh)
        self.dk, self.dv = self._out("dk", ns, C), self._out("dv", ns, C)
        if two:
            self.dk2, self.dv2 = self._out("dk2", HS, C), self._out("dv2", HS, C)

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
        ops, h, sc = _ops(), self.heads, self.scale
        ops.dot_attn_edge_fwd_f32(self.rowptr, self.col, self.q, self.k, self.v, self.k2,
                                  self.v2, self.ns, self.ee, self.out, self.beta, self.m,
                                  self.l, h, sc)
        ops.dot_attn_edge_bwd_dst_f32(self.rowptr, self.col, self.q, self.k, self.v, self.k2,
                                      self.v2, self.ns, self.ee, self.m, self.l, self.g,
                                      self.c, self.dq, self.dee, self.w, h, sc)
        # the source side: local rows, then the halo rows over the tail of the transposed
        # row pointer (as ops/dot_attn.py calls it)
        ops.dot_attn_edge_bwd_src_f32(self.t_rowptr[:self.ns + 1], self.t_col, self.t_slot,
                                      self.q, self.g, self.w, self.dk, self.dv, h, sc)
        if self.two:
            ops.dot_attn_edge_bwd_src_f32(self.t_rowptr[LS:], self.t_col, self.t_slot, self.q,
                                          self.g, self.w, self.dk2, self.dv2, h, sc)
        torch.cuda.synchronize()
        res = {"out": self.out, "stat_m": self.m, "stat_l": self.l, "dq": self.dq,
               "dk": self.dk, "dv": self.dv, "dee": self.dee, "w": self.w}
        if self.two:
            res["dk"] = torch.cat([self.dk, self.dk2])
            res["dv"] = torch.cat([self.dv, self.dv2])
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
        else:  # (a slot of dee / w that was never written is still NaN: not finite)
            _compare(tag, k, got[k], r64[k], r32[k])
    assert (got["stat_l"][(~full).to(DEV)] == 0).all()
    if beta == 0:
        assert (got["out"][(~full).to(DEV)] == 0).all()
    assert (got["dq"][(~full).to(DEV)] == 0).all()


def _run_twice(C, heads, s, idx, two, beta, wide=False):
    """Two runs on fresh buffers: bitwise equal (fixed summation orders, no atomics)."""
    d, ee, c64 = case(C, heads, s), edge_rows(C, heads, s), oracle(C, heads, s, beta)[0]["c"]
    a = _Buffers(d, ee, c64, idx, two, beta, wide)
    b = _Buffers(d, ee, c64, idx, two, beta, wide)
    ra, rb = a.run(), b.run()
    for k in ra:
        assert torch.equal(ra[k].view(torch.int32), rb[k].view(torch.int32)), k
    a.assert_outside_untouched()
    return ra


@pytest.mark.parametrize("idx", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("C,heads", PAIRS)
def test_dot_attn_edge_kernels_vs_fp64(C, heads, s, idx):
    """Forward, destination side, source side (local rows, halo rows) at one instantiation:
    with a second source split at 41 and with all 60 rows local; ``beta = 0`` into a
    NaN-filled ``out`` and ``beta = 0.5`` onto ``out`` on entry."""
    for two in (True, False):
        for beta in (0.0, 0.5):
            got = _run_twice(C, heads, s, idx, two, beta)
            _check(f"kernels C={C} heads={heads} s={s} beta={beta} "
                   f"{'two' if two else 'one'}-source", got, C, heads, s, beta)


@pytest.mark.parametrize("two", [True, False], ids=["two-source", "one-source"])
@pytest.mark.parametrize("C,heads", [(64, 1), (128, 4), (256, 2), (256, 8)])
def test_dot_attn_edge_kernels_wide_operands(C, heads, two):
    """Every operand a column slice of a wider buffer (row strides 2C, 4 heads and 2 heads /
    4): inputs hold NaN outside the slices; outputs keep their sentinel there bitwise."""
    got = _run_twice(C, heads, 0.5, torch.int32, two, 0.0, wide=True)
    _check(f"kernels wide C={C} heads={heads}", got, C, heads, 0.5, 0.0)


def test_dot_attn_edge_kernels_empty_shapes():
    ops = _ops()
    C, Hh, sc = 64, 2, 0.25
    f = lambda *shape: torch.randn(*shape, device=DEV)  # noqa: E731
    e = lambda n: torch.empty(0, n, device=DEV)  # noqa: E731
    i32 = torch.empty(0, dtype=torch.int32, device=DEV)
    q, g, k, v = f(3, C), f(3, C), f(5, C), f(5, C)
    # no rows: returns, writes nothing — also with every operand empty
    rp0 = torch.zeros(1, dtype=torch.long, device=DEV)
    outs = [torch.full((3, n), SENT, device=DEV) for n in (C, Hh, Hh, C, C, C)]
    out, m, l, dq, dk, dv = outs
    ops.dot_attn_edge_fwd_f32(rp0, i32, q, k, v, None, None, 5, e(C), out, 0.0, m, l, Hh, sc)
    ops.dot_attn_edge_bwd_dst_f32(rp0, i32, q, k, v, None, None, 5, e(C), f(3, Hh), f(3, Hh), g,
                                  f(3, Hh), dq, e(C), e(2 * Hh), Hh, sc)
    ops.dot_attn_edge_bwd_src_f32(rp0, i32, i32, q, g, e(2 * Hh), dk, dv, Hh, sc)
    ops.dot_attn_edge_fwd_f32(rp0, i32, e(C), e(C), e(C), None, None, 0, e(C), e(C), 0.0, e(Hh),
                              e(Hh), Hh, sc)
    ops.dot_attn_edge_bwd_dst_f32(rp0, i32, e(C), e(C), e(C), e(C), e(C), 0, e(C), e(Hh), e(Hh),
                                  e(C), e(Hh), e(C), e(C), e(2 * Hh), Hh, sc)
    ops.dot_attn_edge_bwd_src_f32(rp0, i32, i32, e(C), e(C), e(2 * Hh), e(C), e(C), Hh, sc)
    torch.cuda.synchronize()
    for t in outs:
        assert torch.equal(t, torch.full_like(t, SENT))
    # 37 rows, no entries (ee is empty: nothing is launched), with and without source rows
    rp = torch.zeros(R + 1, dtype=torch.long, device=DEV)
    q, g, base = f(R, C), f(R, C), f(R, C)
    for kk, vv in ((k, v), (e(C), e(C))):
        for beta in (0.5, 0.0):
            out = base.clone() if beta else torch.full((R, C), float("nan"), device=DEV)
            m, l = torch.full((R, Hh), SENT, device=DEV), torch.full((R, Hh), SENT, device=DEV)
            ops.dot_attn_edge_fwd_f32(rp, i32, q, kk, vv, None, None, kk.shape[0], e(C), out,
                                      beta, m, l, Hh, sc)
            assert torch.equal(out, base * beta if beta else torch.zeros_like(base))
            assert torch.equal(l, torch.zeros_like(l))
            assert torch.equal(m, torch.full_like(m, SENT))  # filled, not launched
        dq = torch.full((R, C), SENT, device=DEV)
        ops.dot_attn_edge_bwd_dst_f32(rp, i32, q, kk, vv, None, None, kk.shape[0], e(C), f(R, Hh),
                                      l, g, f(R, Hh), dq, e(C), e(2 * Hh), Hh, sc)
        assert torch.equal(dq, torch.zeros_like(dq))
    # 5 source rows of in-degree 0: with destination rows and without
    rp5 = torch.zeros(6, dtype=torch.long, device=DEV)
    for qq, gg in ((q, g), (e(C), e(C))):
        dk, dv = torch.full((5, C), SENT, device=DEV), torch.full((5, C), SENT, device=DEV)
        ops.dot_attn_edge_bwd_src_f32(rp5, i32, i32, qq, gg, e(2 * Hh), dk, dv, Hh, sc)
        assert torch.equal(dk, torch.zeros_like(dk)) and torch.equal(dv, torch.zeros_like(dv))


# --------------------------------------------------- contract checks (bindings_dot_attn.cpp)
def _valid_args(C, heads):
    rowptr, col, _ = pattern()
    t_rowptr, t_col = transpose(rowptr, col, N)
    f = lambda *shape: torch.randn(*shape, device=DEV)  # noqa: E731
    return dict(rowptr=rowptr.to(DEV), col=col.to(torch.int32).to(DEV), q=f(R, C), k=f(N, C),
                v=f(N, C), k2=None, v2=None, nsplit=N, ee=f(E, C), out=f(R, C), beta=0.5,
                stat_m=f(R, heads), stat_l=f(R, heads), g=f(R, C), c=f(R, heads), dq=f(R, C),
                dee=f(E, C), w=f(E, 2 * heads), t_rowptr=t_rowptr.to(DEV),
                t_col=t_col.to(torch.int32).to(DEV),
                t_slot=_t_slot(col).to(torch.int32).to(DEV), dk=f(N, C), dv=f(N, C),
                heads=heads, scale=0.125)


_CALLS = {
    "fwd": ("dot_attn_edge_fwd_f32",
            ("rowptr", "col", "q", "k", "v", "k2", "v2", "nsplit", "ee", "out", "beta",
             "stat_m", "stat_l", "heads", "scale"), ("out", "stat_m", "stat_l")),
    "dst": ("dot_attn_edge_bwd_dst_f32",
            ("rowptr", "col", "q", "k", "v", "k2", "v2", "nsplit", "ee", "stat_m", "stat_l",
             "g", "c", "dq", "dee", "w", "heads", "scale"), ("dq", "dee", "w")),
    "src": ("dot_attn_edge_bwd_src_f32",
            ("t_rowptr", "t_col", "t_slot", "q", "g", "w", "dk", "dv", "heads", "scale"),
            ("dk", "dv")),
}


def _violate(what):
    """(the arguments, the ops that must refuse them)."""
    if what == "C=96":
        return _valid_args(96, 2), ("fwd", "dst", "src")
    if what == "heads=3":
        return _valid_args(64, 3), ("fwd", "dst", "src")
    A = _valid_args(64, 2)
    if what == "ee with E - 1 rows":
        A["ee"] = A["ee"][:-1]
        return A, ("fwd", "dst")
    if what == "dee with E - 1 rows":
        A["dee"] = A["dee"][:-1]
        return A, ("dst",)
    if what == "ee offset by one float":
        flat = torch.empty(E * 64 + 4, device=DEV)
        A["ee"] = flat[1:1 + E * 64].view(E, 64).normal_()
        assert A["ee"].data_ptr() % 16 == 4
        return A, ("fwd", "dst")
    if what == "w with heads columns":
        A["w"] = A["w"][:, :2].contiguous()
        return A, ("dst", "src")
    if what == "t_slot of the other integer dtype":
        A["t_slot"] = A["t_slot"].long()
        return A, ("src",)
    if what == "t_slot one entry short":
        A["t_slot"] = A["t_slot"][:-1]
        return A, ("src",)
    raise KeyError(what)


@pytest.mark.parametrize("what", ["ee with E - 1 rows", "dee with E - 1 rows",
                                  "ee offset by one float", "w with heads columns",
                                  "t_slot of the other integer dtype", "t_slot one entry short",
                                  "C=96", "heads=3"])
def test_dot_attn_edge_contract_checks_raise_before_launch(what):
    A, refused = _violate(what)
    for op in refused:
        name, args, outs = _CALLS[op]
        before = {k: A[k].clone() for k in outs}
        with pytest.raises(RuntimeError):
            getattr(_ops(), name)(*[A[k] for k in args])
        torch.cuda.synchronize()
        for k, t in before.items():
            assert torch.equal(A[k], t), (op, k)


# -------------------------------------------------------------------------- the autograd op
def _run_op(dev, dtype, C, heads, s, halo):
    """``dot_attention(..., edge=)`` forward + backward; k / v (and kh / vh) are the column
    halves of one [rows, 2C] buffer, as the layer hands them in."""
    from dgraph_amd.ops import dot_attention
    from dgraph_amd.ops.gat import GatPattern

    rowptr, col, _ = pattern()
    d = case(C, heads, s)
    ns, nh = (LS, HS) if halo else (N, 0)
    pat = GatPattern(rowptr.to(dev), col.to(dev), ns, nh)
    q = d["q"].to(dev, dtype).requires_grad_()
    ee = edge_rows(C, heads, s).to(dev, dtype).requires_grad_()
    kv = torch.cat([d["k"], d["v"]], 1).to(dev, dtype)
    kvl = kv[:ns].clone().requires_grad_()
    kvh = kv[ns:].clone().requires_grad_() if halo else None
    out = dot_attention(q, kvl[:, :C], kvl[:, C:], pat,
                        None if kvh is None else kvh[:, :C],
                        None if kvh is None else kvh[:, C:], heads=heads, edge=ee)
    ins = [q, ee, kvl] + ([kvh] if halo else [])
    grads = torch.autograd.grad(out, ins, d["g"].to(dev, dtype))
    gkv = torch.cat(grads[2:], 0)
    return {"out": out.detach(), "dq": grads[0], "dee": grads[1], "dk": gkv[:, :C],
            "dv": gkv[:, C:]}


@pytest.mark.parametrize("halo", [True, False], ids=["halo", "no_halo"])
@pytest.mark.parametrize("C,heads,s", [(C, h, 0.5) for C, h in PAIRS] +
                         [(64, 8, 40.0), (128, 1, 40.0), (256, 4, 40.0)])
def test_dot_attention_edge_op_gpu_vs_cpu(C, heads, s, halo):
    ref64 = _run_op("cpu", torch.float64, C, heads, s, halo)
    _, r32 = oracle(C, heads, s, 0.0)
    got = _run_op(DEV, torch.float32, C, heads, s, halo)
    got2 = _run_op(DEV, torch.float32, C, heads, s, halo)
    tag = f"op C={C} heads={heads} s={s} halo={halo}"
    for k in got:
        assert ref64[k].dtype == torch.float64
        assert torch.equal(got[k], got2[k]), k
        _compare(tag, k, got[k], ref64[k], r32[k])


def test_dot_attention_edge_op_rejects_unsupported_edge_dtypes():
    from dgraph_amd.ops import dot_attention
    from dgraph_amd.ops.gat import GatPattern

    rowptr, col, _ = pattern()
    pat = GatPattern(rowptr.to(DEV), col.to(DEV), N, 0)
    f = lambda n, C, dt=torch.float32: torch.randn(n, C, device=DEV, dtype=dt)  # noqa: E731
    for dt in (torch.bfloat16, torch.float64):
        with pytest.raises(ValueError, match="edge dtype"):
            dot_attention(f(R, 64), f(N, 64), f(N, 64), pat, heads=2, edge=f(E, 64, dt))
    with pytest.raises(ValueError):
        dot_attention(f(R, 64), f(N, 64), f(N, 64), pat, heads=2, edge=f(E - 1, 64))


@pytest.mark.parametrize("side", ["no destination rows", "no local sources", "no halo"])
def test_dot_attention_edge_op_empty_sides(side):
    """Legal empty sides of a rank's relation with an ``edge`` of matching (possibly zero)
    rows: forward + backward run, agree with the CPU op and give zero gradients where
    nothing is attended to."""
    from dgraph_amd.ops import dot_attention
    from dgraph_amd.ops.gat import GatPattern

    C, heads = 64, 2
    rowptr, col, _ = pattern()
    d = case(C, heads, 0.5)
    if side == "no destination rows":
        rp, cl, ns, nh, nq = torch.zeros(1, dtype=torch.long), col[:0], 5, 3, 0
    elif side == "no local sources":
        rp, cl, ns, nh, nq = rowptr, col % HS, 0, HS, R
    else:
        rp, cl, ns, nh, nq = rowptr, col, N, 0, R
    ee0 = edge_rows(C, heads, 0.5)[:cl.numel()]

    def run(dev, dtype):
        pat = GatPattern(rp.to(dev), cl.to(dev), ns, nh)
        mk = lambda t: t.to(dev, dtype).clone().requires_grad_()  # noqa: E731
        q, k, v, ee = mk(d["q"][:nq]), mk(d["k"][:ns]), mk(d["v"][:ns]), mk(ee0)
        kh, vh = (mk(d["k"][ns:ns + nh]), mk(d["v"][ns:ns + nh])) if nh else (None, None)
        out = dot_attention(q, k, v, pat, kh, vh, heads=heads, edge=ee)
        ins = [t for t in (q, k, v, ee, kh, vh) if t is not None]
        return [out.detach()] + list(torch.autograd.grad(out, ins, d["g"][:nq].to(dev, dtype)))

    ref, got = run("cpu", torch.float64), run(DEV, torch.float32)
    for a, b in zip(got, ref):
        assert a.shape == b.shape
        _compare(f"empty {side}", "all", a, b, b.float())
    if side == "no destination rows":
        assert all(int(torch.count_nonzero(t)) == 0 for t in got)
        assert got[4].shape == (0, C)
    if side == "no local sources":
        assert got[2].shape == (0, C) and got[3].shape == (0, C)


# --------------------------------------------------------------------------------- the layer
def test_transformer_conv_edge_gpu_vs_cpu():
    """``CommAwareTransformerConv`` (in 32, out 64, 2 heads, ``edge_dim=7``) forward +
    backward on the GPU against the same layer on the CPU at fp64, W = 1; the fp32 error of
    the bound is the dense per-edge formulation's at fp32."""
    import copy

    from dgraph_amd.data.hetero import (build_relation_graph, get_vertex_offsets,
                                        relation_edge_order)
    from dgraph_amd.models.transformer_conv import CommAwareTransformerConv

    edges = _edges()
    offs = {0: get_vertex_offsets(ND, 1), 1: get_vertex_offsets(NS, 1)}
    order = relation_edge_order(edges, offs, 0, 0)
    torch.manual_seed(0)
    base = CommAwareTransformerConv(32, 64, heads=2, hetero=True, edge_dim=7)
    with torch.no_grad():
        base.bias.normal_()
    gen = torch.Generator().manual_seed(1)
    xd, xs, w = (torch.randn(n, c, generator=gen) for n, c in ((ND, 32), (NS, 32), (ND, 64)))
    ea = _edge_attr(edges, 7, torch.float32)

    def run(dev, dtype, dense=False):
        layer = copy.deepcopy(base).to(dev, dtype)
        a, b, e = (t.to(dev, dtype).requires_grad_() for t in (xd, xs, ea))
        if dense:
            out = _dense_edge_transformer(layer, a, b, edges.to(dev), e)
        else:
            out = layer(a, build_relation_graph(edges, 1, 0, offs, 0, 1).to(dev), x_j=b,
                        edge_attr=e[order.to(dev)])
        grads = torch.autograd.grad(out, [a, b, e] + list(layer.parameters()), w.to(dev, dtype))
        return [out.detach()] + list(grads)

    ref64, ref32 = run("cpu", torch.float64), run("cpu", torch.float32, dense=True)
    got = run(DEV, torch.float32)
    names = ["out", "dx", "dx_j", "dedge_attr"] + [n for n, _ in base.named_parameters()]
    assert len(names) == len(got) == 11
    for n, a, b, c in zip(names, got, ref64, ref32):
        _compare("layer", n, a, b, c)
