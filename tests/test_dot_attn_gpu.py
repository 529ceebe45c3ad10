"""The fused dot-product attention kernels (csrc/kernels/dot_attn_f32.hip, called through
``_native.ops().dot_attn_*_f32`` directly), the ``dot_attention`` op and the
``CommAwareTransformerConv`` layer on the GPU against the fp64 evaluation of their contract
(tests/test_dot_attn.py), at every ``(C, heads)`` instantiation and both column index types.

Pattern and inputs: see tests/test_dot_attn.py (37 rows over 41 local + 19 halo sources with
rows of degree 0, 1, LPR +- 1 and a 301-entry hub; score scales 0.5 and 40). The backward
kernels get ``c`` from the fp64 oracle, rounded to fp32.

Bound per compared array: ``max(2e-5, 8 err32) max(1, max|fp64|)`` with ``err32`` the error of
the same formula evaluated in fp32 on the CPU (``test_gat_kernels.bound``) — nothing is taken
from the kernels' own output. Largest ``error / bound`` seen on an MI355X (a record, not an
input to the bound; the tests print every figure before asserting):

    dot_attn_fwd      out 0.107   stat_m 0.007   stat_l 0.207
    dot_attn_bwd_dst  dq 0.228
    dot_attn_bwd_src  dk 0.264    dv 0.236
    the op            out 0.081   dq 0.162   dk 0.165   dv 0.236
    empty sides       0.095
    the layer         out 0.006   dx 0.012   dx_j 0.010   parameters 0.015 or less

No array came near the bound at scale 40, so ``err32`` is the plain fp32 evaluation's; the
ratio against the larger error of two D-sum orders is printed next to it for the record.
"""
from __future__ import annotations

import pytest
import torch

from test_dot_attn import (CIN, ND, NS, OUTPUTS, SCALES, _dense_transformer, _edges, case,
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
        print(f"\n[dot-attn] largest error / bound, {k}: {RATIOS[k]:.3f}", end="")
    print()


def _ops():
    from dgraph_amd import _native

    return _native.ops()


def _compare(tag, name, got, ref64, ref32, ref32p=None):
    """|got - fp64| against :func:`bound`; prints the figures, records the ratio. With
    ``ref32p`` (the fp32 evaluation with the D-sum in a second order) the ratio against the
    larger of the two fp32 errors is printed next to it, for the record only."""
    got = got.detach().double().cpu()
    assert got.shape == ref64.shape, (tag, name, got.shape, ref64.shape)
    assert torch.isfinite(got).all(), (tag, name)
    bd = bound(ref64, ref32)
    err = float((got - ref64.double()).abs().max()) if got.numel() else 0.0
    key = name if tag.startswith("kernels") else f"{tag.split()[0]}:{name}"
    RATIOS[key] = max(RATIOS.get(key, 0.0), err / bd)
    extra = ""
    if ref32p is not None:
        extra = f" (ratio with both D-sum orders {err / max(bd, bound(ref64, ref32p)):.3f})"
    print(f"{tag} {name}: err {err:.3e} bound {bd:.3e} ratio {err / bd:.3f}{extra}")
    assert err <= bd, (tag, name, err, bd)


class _Buffers:
    """Device operands of one run of the three kernels. ``wide``: every feature array is
    the upper column half of a [rows, 2C] buffer and every per-head array the upper half of
    a [rows, 2 heads] buffer (one head: column 2 of a [rows, 4] buffer); inputs hold NaN
    outside their slice, outputs ``SENT``. Outputs hold NaN inside on entry."""

    def __init__(self, d, c64, idx, two, beta, wide=False):
        rowptr, col, _ = pattern()
        t_rowptr, t_col = transpose(rowptr, col, N)
        self.heads, self.two, self.beta, self.wide = d["heads"], two, beta, wide
        self.scale = d["scale"]
        self.held = []  # (name, wide buffer, slice) of the outputs
        self.rowptr, self.col = rowptr.to(DEV), col.to(idx).to(DEV)
        self.t_rowptr, self.t_col = t_rowptr.to(DEV), t_col.to(idx).to(DEV)
        ns = LS if two else N
        self.ns = ns
        self.q, self.g = self._in(d["q"]), self._in(d["g"])
        self.k, self.v = self._in(d["k"][:ns]), self._in(d["v"][:ns])
        self.k2 = self._in(d["k"][ns:]) if two else None
        self.v2 = self._in(d["v"][ns:]) if two else None
        self.c = self._in(c64.float())
        C, Hh = d["C"], d["heads"]
        self.out = self._out("out", R, C)
        if beta != 0:
            self.out.copy_(d["out0"])
        self.m, self.l = self._out("stat_m", R, Hh), self._out("stat_l", R, Hh)
        self.dq = self._out("dq", R, C)
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
        ops.dot_attn_fwd_f32(self.rowptr, self.col, self.q, self.k, self.v, self.k2, self.v2,
                             self.ns, self.out, self.beta, self.m, self.l, h, sc)
        ops.dot_attn_bwd_dst_f32(self.rowptr, self.col, self.q, self.k, self.v, self.k2,
                                 self.v2, self.ns, self.m, self.l, self.g, self.c, self.dq, h,
                                 sc)
        # the source side: local rows, then the halo rows over the tail of the transposed
        # row pointer (as ops/dot_attn.py calls it)
        ops.dot_attn_bwd_src_f32(self.t_rowptr[:self.ns + 1], self.t_col, self.q, self.g,
                                 self.k, self.v, self.m, self.l, self.c, self.dk, self.dv, h,
                                 sc)
        if self.two:
            ops.dot_attn_bwd_src_f32(self.t_rowptr[LS:], self.t_col, self.q, self.g, self.k2,
                                     self.v2, self.m, self.l, self.c, self.dk2, self.dv2, h,
                                     sc)
        torch.cuda.synchronize()
        res = {"out": self.out, "stat_m": self.m, "stat_l": self.l, "dq": self.dq,
               "dk": self.dk, "dv": self.dv}
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
    r64, r32, r32p = oracle(C, heads, s, beta)
    rowptr = pattern()[0]
    full = rowptr[1:] > rowptr[:-1]
    for k in OUTPUTS:
        if k == "stat_m":  # (an empty row's maximum is not part of the contract)
            _compare(tag, k, got[k][full.to(DEV)], r64[k][full], r32[k][full], r32p[k][full])
        else:
            _compare(tag, k, got[k], r64[k], r32[k], r32p[k])
    assert (got["stat_l"][(~full).to(DEV)] == 0).all()
    if beta == 0:
        assert (got["out"][(~full).to(DEV)] == 0).all()
    assert (got["dq"][(~full).to(DEV)] == 0).all()


def _run_twice(C, heads, s, idx, two, beta, wide=False):
    """Two runs on fresh buffers: bitwise equal (fixed summation orders, no atomics)."""
    d, c64 = case(C, heads, s), oracle(C, heads, s, beta)[0]["c"]
    a, b = _Buffers(d, c64, idx, two, beta, wide), _Buffers(d, c64, idx, two, beta, wide)
    ra, rb = a.run(), b.run()
    for k in ra:
        assert torch.equal(ra[k].view(torch.int32), rb[k].view(torch.int32)), k
    a.assert_outside_untouched()
    return ra


@pytest.mark.parametrize("idx", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("C,heads", PAIRS)
def test_dot_attn_kernels_vs_fp64(C, heads, s, idx):
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
def test_dot_attn_kernels_wide_operands(C, heads, two):
    """Every operand a column slice of a wider buffer (row strides 2C and 2 heads / 4):
    inputs hold NaN outside the slices; outputs keep their sentinel there bitwise."""
    got = _run_twice(C, heads, 0.5, torch.int32, two, 0.0, wide=True)
    _check(f"kernels wide C={C} heads={heads}", got, C, heads, 0.5, 0.0)


def test_dot_attn_kernels_empty_shapes():
    ops = _ops()
    C, Hh, sc = 64, 2, 0.25
    f = lambda *shape: torch.randn(*shape, device=DEV)  # noqa: E731
    i32 = torch.empty(0, dtype=torch.int32, device=DEV)
    q, g, k, v = f(3, C), f(3, C), f(5, C), f(5, C)
    # no rows: returns, writes nothing — also with every operand empty
    rp0 = torch.zeros(1, dtype=torch.long, device=DEV)
    outs = [torch.full((3, n), SENT, device=DEV) for n in (C, Hh, Hh, C, C, C)]
    out, m, l, dq, dk, dv = outs
    ops.dot_attn_fwd_f32(rp0, i32, q, k, v, None, None, 5, out, 0.0, m, l, Hh, sc)
    ops.dot_attn_bwd_dst_f32(rp0, i32, q, k, v, None, None, 5, f(3, Hh), f(3, Hh), g, f(3, Hh),
                             dq, Hh, sc)
    ops.dot_attn_bwd_src_f32(rp0, i32, q, g, k, v, f(3, Hh), f(3, Hh), f(3, Hh), dk, dv, Hh, sc)
    e = lambda n: torch.empty(0, n, device=DEV)  # noqa: E731
    ops.dot_attn_fwd_f32(rp0, i32, e(C), e(C), e(C), None, None, 0, e(C), 0.0, e(Hh), e(Hh),
                         Hh, sc)
    ops.dot_attn_bwd_dst_f32(rp0, i32, e(C), e(C), e(C), e(C), e(C), 0, e(Hh), e(Hh), e(C),
                             e(Hh), e(C), Hh, sc)
    ops.dot_attn_bwd_src_f32(rp0, i32, e(C), e(C), e(C), e(C), e(Hh), e(Hh), e(Hh), e(C), e(C),
                             Hh, sc)
    torch.cuda.synchronize()
    for t in outs:
        assert torch.equal(t, torch.full_like(t, SENT))
    # 37 rows, no entries: with source rows (a launch) and without any (no launch)
    rp = torch.zeros(R + 1, dtype=torch.long, device=DEV)
    q, g, base = f(R, C), f(R, C), f(R, C)
    for kk, vv in ((k, v), (e(C), e(C))):
        for beta in (0.5, 0.0):
            out = base.clone() if beta else torch.full((R, C), float("nan"), device=DEV)
            m, l = f(R, Hh), torch.full((R, Hh), SENT, device=DEV)
            ops.dot_attn_fwd_f32(rp, i32, q, kk, vv, None, None, kk.shape[0], out, beta, m, l,
                                 Hh, sc)
            assert torch.equal(out, base * beta if beta else torch.zeros_like(base))
            assert torch.equal(l, torch.zeros_like(l))
        dq = torch.full((R, C), SENT, device=DEV)
        ops.dot_attn_bwd_dst_f32(rp, i32, q, kk, vv, None, None, kk.shape[0], m, l, g,
                                 f(R, Hh), dq, Hh, sc)
        assert torch.equal(dq, torch.zeros_like(dq))
    # 5 source rows of in-degree 0: with destination rows (a launch) and without (no launch)
    rp5 = torch.zeros(6, dtype=torch.long, device=DEV)
    for qq, gg, n in ((q, g, R), (e(C), e(C), 0)):
        dk, dv = torch.full((5, C), SENT, device=DEV), torch.full((5, C), SENT, device=DEV)
        ops.dot_attn_bwd_src_f32(rp5, i32, qq, gg, k, v, f(n, Hh), f(n, Hh), f(n, Hh), dk, dv,
                                 Hh, sc)
        assert torch.equal(dk, torch.zeros_like(dk)) and torch.equal(dv, torch.zeros_like(dv))


# --------------------------------------------------- contract checks (bindings_dot_attn.cpp)
def _valid_args(C, heads):
    rowptr, col, _ = pattern()
    f = lambda *shape: torch.randn(*shape, device=DEV)  # noqa: E731
    return dict(rowptr=rowptr.to(DEV), col=col.to(torch.int32).to(DEV), q=f(R, C), k=f(N, C),
                v=f(N, C), k2=None, v2=None, nsplit=N, out=f(R, C), beta=0.5,
                stat_m=f(R, heads), stat_l=f(R, heads), heads=heads, scale=0.125)


_FWD = ("rowptr", "col", "q", "k", "v", "k2", "v2", "nsplit", "out", "beta", "stat_m", "stat_l",
        "heads", "scale")


def _violate(what):
    if what == "C=96":
        return _valid_args(96, 2)
    if what == "heads=3":
        return _valid_args(64, 3)
    if what == "(C,heads)=(64,16)":
        return _valid_args(64, 16)
    A = _valid_args(64, 2)
    if what == "k offset by one float":
        flat = torch.empty(N * 64 + 4, device=DEV)
        A["k"] = flat[1:1 + N * 64].view(N, 64).normal_()
        assert A["k"].data_ptr() % 16 == 4
    elif what == "stat_l row stride differs from stat_m's":
        A["stat_l"] = torch.randn(R, 4, device=DEV)[:, :2]
    elif what == "k2 without v2":
        A.update(k2=A["k"][LS:].clone(), nsplit=LS)
    elif what == "nsplit larger than k's row count":
        A.update(k2=torch.randn(HS, 64, device=DEV), v2=torch.randn(HS, 64, device=DEV),
                 nsplit=N + 1)
    elif what == "float64 q":
        A["q"] = A["q"].double()
    else:
        raise KeyError(what)
    return A


@pytest.mark.parametrize("what", ["C=96", "heads=3", "(C,heads)=(64,16)", "k offset by one float",
                                  "stat_l row stride differs from stat_m's", "k2 without v2",
                                  "nsplit larger than k's row count", "float64 q"])
def test_dot_attn_contract_checks_raise_before_launch(what):
    A = _violate(what)
    before = {k: A[k].clone() for k in ("out", "stat_m", "stat_l")}
    with pytest.raises(RuntimeError):
        _ops().dot_attn_fwd_f32(*[A[k] for k in _FWD])
    torch.cuda.synchronize()
    for k, t in before.items():
        assert torch.equal(A[k], t), k


# -------------------------------------------------------------------------- the autograd op
def _run_op(dev, dtype, C, heads, s, halo):
    """``dot_attention`` forward + backward; k / v (and kh / vh) are the column halves of
    one [rows, 2C] buffer, as the layer hands them in."""
    from dgraph_amd.ops import dot_attention
    from dgraph_amd.ops.gat import GatPattern

    rowptr, col, _ = pattern()
    d = case(C, heads, s)
    ns, nh = (LS, HS) if halo else (N, 0)
    pat = GatPattern(rowptr.to(dev), col.to(dev), ns, nh)
    q = d["q"].to(dev, dtype).requires_grad_()
    kv = torch.cat([d["k"], d["v"]], 1).to(dev, dtype)
    kvl = kv[:ns].clone().requires_grad_()
    kvh = kv[ns:].clone().requires_grad_() if halo else None
    out = dot_attention(q, kvl[:, :C], kvl[:, C:], pat,
                        None if kvh is None else kvh[:, :C],
                        None if kvh is None else kvh[:, C:], heads=heads)
    ins = [q, kvl] + ([kvh] if halo else [])
    grads = torch.autograd.grad(out, ins, d["g"].to(dev, dtype))
    gkv = torch.cat(grads[1:], 0)
    return {"out": out.detach(), "dq": grads[0], "dk": gkv[:, :C], "dv": gkv[:, C:]}


@pytest.mark.parametrize("halo", [True, False], ids=["halo", "no_halo"])
@pytest.mark.parametrize("C,heads,s", [(C, h, 0.5) for C, h in PAIRS] +
                         [(64, 8, 40.0), (128, 1, 40.0), (256, 4, 40.0)])
def test_dot_attention_op_gpu_vs_cpu(C, heads, s, halo):
    ref64 = _run_op("cpu", torch.float64, C, heads, s, halo)
    _, r32, _ = oracle(C, heads, s, 0.0)
    got = _run_op(DEV, torch.float32, C, heads, s, halo)
    got2 = _run_op(DEV, torch.float32, C, heads, s, halo)
    tag = f"op C={C} heads={heads} s={s} halo={halo}"
    for k in got:
        assert ref64[k].dtype == torch.float64
        assert torch.equal(got[k], got2[k]), k
        _compare(tag, k, got[k], ref64[k], r32[k])


def test_dot_attention_op_rejects_unsupported_gpu_inputs():
    from dgraph_amd.ops import dot_attention
    from dgraph_amd.ops.gat import GatPattern

    rowptr, col, _ = pattern()
    pat = GatPattern(rowptr.to(DEV), col.to(DEV), N, 0)
    f = lambda n, C, dt=torch.float32: torch.randn(n, C, device=DEV, dtype=dt)  # noqa: E731
    for C, heads, dt in ((96, 2, torch.float32), (64, 16, torch.float32),
                         (64, 2, torch.float64), (64, 2, torch.bfloat16)):
        with pytest.raises(ValueError, match="64, 128, 256"):
            dot_attention(f(R, C, dt), f(N, C, dt), f(N, C, dt), pat, heads=heads)


@pytest.mark.parametrize("side", ["no destination rows", "no local sources", "no halo"])
def test_dot_attention_op_empty_sides(side):
    """Legal empty sides of a rank's relation: forward + backward run, agree with the CPU op
    and give zero gradients where nothing is attended to."""
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

    def run(dev, dtype):
        pat = GatPattern(rp.to(dev), cl.to(dev), ns, nh)
        mk = lambda t: t.to(dev, dtype).clone().requires_grad_()  # noqa: E731
        q, k, v = mk(d["q"][:nq]), mk(d["k"][:ns]), mk(d["v"][:ns])
        kh, vh = (mk(d["k"][ns:ns + nh]), mk(d["v"][ns:ns + nh])) if nh else (None, None)
        out = dot_attention(q, k, v, pat, kh, vh, heads=heads)
        ins = [t for t in (q, k, v, kh, vh) if t is not None]
        return [out.detach()] + list(torch.autograd.grad(out, ins, d["g"][:nq].to(dev, dtype)))

    ref, got = run("cpu", torch.float64), run(DEV, torch.float32)
    for a, b in zip(got, ref):
        assert a.shape == b.shape
        _compare(f"empty {side}", "all", a, b, b.float())
    if side == "no destination rows":
        assert all(int(torch.count_nonzero(t)) == 0 for t in got)
    if side == "no local sources":
        assert got[2].shape == (0, C) and got[3].shape == (0, C)


# --------------------------------------------------------------------------------- the layer
def test_transformer_conv_gpu_vs_cpu():
    """``CommAwareTransformerConv`` (in 32, out 64, 2 heads) forward + backward on the GPU
    against the same layer on the CPU at fp64, W = 1; the fp32 error of the bound is the
    dense per-edge formulation's at fp32."""
    import copy

    from dgraph_amd.data.hetero import build_relation_graph, get_vertex_offsets
    from dgraph_amd.models.transformer_conv import CommAwareTransformerConv

    edges = _edges()
    offs = {0: get_vertex_offsets(ND, 1), 1: get_vertex_offsets(NS, 1)}
    torch.manual_seed(0)
    base = CommAwareTransformerConv(32, 64, heads=2, hetero=True)
    with torch.no_grad():
        base.bias.normal_()
    gen = torch.Generator().manual_seed(1)
    xd, xs, w = (torch.randn(n, c, generator=gen) for n, c in ((ND, 32), (NS, 32), (ND, 64)))

    def run(dev, dtype, dense=False):
        layer = copy.deepcopy(base).to(dev, dtype)
        a, b = (t.to(dev, dtype).requires_grad_() for t in (xd, xs))
        if dense:
            out = _dense_transformer(layer, a, b, edges)
        else:
            out = layer(a, build_relation_graph(edges, 1, 0, offs, 0, 1).to(dev), x_j=b)
        grads = torch.autograd.grad(out, [a, b] + list(layer.parameters()), w.to(dev, dtype))
        return [out.detach()] + list(grads)

    ref64, ref32 = run("cpu", torch.float64), run("cpu", torch.float32, dense=True)
    got = run(DEV, torch.float32)
    names = ["out", "dx", "dx_j"] + [n for n, _ in base.named_parameters()]
    assert len(names) == len(got) == 9
    for n, a, b, c in zip(names, got, ref64, ref32):
        _compare("layer", n, a, b, c)
