"""The dot-product attention kernels with bf16 storage (csrc/kernels/dot_attn_bf16.hip): the
op ``ops.dot_attention`` on bf16 rows, the three kernels called directly, the empty sides and a
bf16 ``CommAwareTransformerConv``. Reference and bounds: tests/test_dot_attn_bf16.py; nothing
is taken from the kernels' own output. The degree-1 rows (reference dq exactly 0) at score
scale 40 are what a ``c`` taken from the rounded output fails. Largest error / bound seen on an
MI355X (a record, not an input to the bounds; the tests print every figure before asserting;
a bf16 array comes close to 1 because one rounding errs by up to 2^-8 of the value):

    the op       out 0.977   dq 0.978   dk 0.968   dv 0.976
    the kernels  out 0.977   dq 0.978   dk 0.968   dv 0.976
                 stat_m 0.005   stat_l 0.094   c 0.085
    the layer    largest |GPU - CPU| / max|CPU| over the output and the 8 gradients: 0
                 (equal bits in all nine arrays; the margin is 2^-6 = 0.0156)
"""
from __future__ import annotations

import pytest
import torch

from test_dot_attn import ND, NS, _edges
from test_dot_attn_bf16 import SCALES, bounds, inputs, reference
from test_gat_kernels import HS, LS, N, PAIRS, R, pattern, transpose

pytestmark = pytest.mark.gpu
DEV, BF = "cuda", torch.bfloat16
SENT = -7.25e9


@pytest.fixture(scope="module", autouse=True)
def _native():
    from dgraph_amd import _native

    assert _native.load(), "native library missing"


def check(tag, got, C, heads, s):
    ref64, ref32 = (reference(C, heads, s, t) for t in (torch.float64, torch.float32))
    deg = pattern()[0].diff()
    for k, t in got.items():
        t, r64, r32 = t.detach().double().cpu(), ref64[k], ref32[k]
        assert t.shape == r64.shape, (tag, k, t.shape, r64.shape)
        if k == "stat_m":  # (an empty row's maximum is unspecified)
            t, r64, r32 = t[deg > 0], r64[deg > 0], r32[deg > 0]
        assert torch.isfinite(t).all(), (tag, k)
        b, bd = bounds(k, r64, r32)
        ratio = float(((t - r64).abs() / bd).max())
        print(f"{tag} {k}: bound {b:.3e} largest err / bound {ratio:.3f}")
        assert ratio <= 1.0, (tag, k, ratio)


def run_op(d, pat, ns, nh, heads, nq=R):
    """out and the gradients of ``dot_attention`` on bf16 rows: k, v the first ``ns`` sources,
    kh, vh the next ``nh`` (``None`` without any: one source)."""
    from dgraph_amd.ops import dot_attention

    mk = lambda t: t.to(DEV, BF).requires_grad_()  # noqa: E731
    q, k, v = mk(d["q"][:nq]), mk(d["k"][:ns]), mk(d["v"][:ns])
    kh, vh = (None, None) if nh is None else (mk(d["k"][ns:ns + nh]), mk(d["v"][ns:ns + nh]))
    out = dot_attention(q, k, v, pat, kh, vh, d["scale"], heads=heads, allow_bf16=True)
    ins = [t for t in (q, k, v, kh, vh) if t is not None]
    grads = torch.autograd.grad(out, ins, d["g"][:nq].to(DEV, BF))
    for t, gr in zip([q] + ins, (out,) + grads):
        assert gr.dtype == BF and gr.shape == t.shape
    return [out.detach()] + list(grads)


@pytest.mark.parametrize("two", [False, True], ids=["one_source", "two_sources"])
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("C,heads", PAIRS)
def test_op_against_fp64(C, heads, s, two):
    from dgraph_amd.ops.gat import GatPattern

    rowptr, col, _ = pattern()
    ns, nh = (LS, HS) if two else (N, None)
    pat = GatPattern(rowptr.to(DEV), col.to(DEV), ns, nh or 0)
    d = inputs(C, heads, s)
    got, again = run_op(d, pat, ns, nh, heads), run_op(d, pat, ns, nh, heads)
    for a, b in zip(got, again):
        assert torch.equal(a, b)
    out, dq, dk, dv, *halo = got
    if two:
        dk, dv = torch.cat([dk, halo[0]]), torch.cat([dv, halo[1]])
    check(f"op C={C} heads={heads} s={s} two={two}", dict(out=out, dq=dq, dk=dk, dv=dv), C,
          heads, s)


def _wide(t, fill):
    """``t`` as the upper column half of a [rows, 2C] bf16 buffer holding ``fill`` elsewhere."""
    buf = torch.full((t.shape[0], 2 * t.shape[1]), fill, dtype=BF, device=DEV)
    buf[:, t.shape[1]:] = t.to(DEV)
    return buf, buf[:, t.shape[1]:]


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("C,heads", PAIRS)
def test_kernels_directly(C, heads, s):
    from dgraph_amd import _native

    ops = _native.ops()
    rowptr, col, _ = pattern()
    t_rowptr, t_col = transpose(rowptr, col, N)
    d = inputs(C, heads, s)
    nan = float("nan")
    rp, cl = rowptr.to(DEV), col.int().to(DEV)
    trp, tcl = t_rowptr.to(DEV), t_col.int().to(DEV)
    q, g, k, kh, v, vh = (_wide(t, nan)[1] for t in (d["q"], d["g"], d["k"][:LS], d["k"][LS:],
                                                     d["v"][:LS], d["v"][LS:]))

    def run():
        held = {}  # name -> (whole buffer, the part the kernels may write: NaN on entry)

        def out(name, rows, cols=None):
            if cols is None:  # bf16, the upper half of a sentinel buffer
                buf, view = _wide(torch.full((rows, C), nan), SENT)
            else:  # fp32 with one sentinel row past the end
                buf = torch.full((rows + 1, cols), SENT, device=DEV)
                view = buf[:rows].fill_(nan)
            held[name] = (buf, view)
            return view

        o, m, l, c = out("out", R), out("stat_m", R, heads), out("stat_l", R, heads), \
            out("c", R, heads)
        ops.dot_attn_fwd_bf16(rp, cl, q, k, v, kh, vh, LS, o, m, l, heads, d["scale"])
        ops.dot_attn_bwd_dst_bf16(rp, cl, q, k, v, kh, vh, LS, m, l, g, c, out("dq", R), heads,
                                  d["scale"])
        for nm, ks, vs, n, tr in (("", k, v, LS, trp[:LS + 1]), ("h", kh, vh, HS, trp[LS:])):
            ops.dot_attn_bwd_src_bf16(tr, tcl, q, g, ks, vs, m, l, c, out("dk" + nm, n),
                                      out("dv" + nm, n), heads, d["scale"])
        torch.cuda.synchronize()
        return held

    held, again = run(), run()
    for name, (buf, view) in held.items():
        assert torch.equal(buf, again[name][0]), name  # two calls, equal bits (no NaN is left)
        outside = torch.ones_like(buf, dtype=torch.bool)
        outside[:view.shape[0], buf.shape[1] - view.shape[1]:] = False
        assert (buf[outside] == torch.tensor(SENT, dtype=buf.dtype)).all(), name
    got = {n: held[n][1] for n in ("out", "stat_m", "stat_l", "c", "dq")}
    got["dk"] = torch.cat([held["dk"][1], held["dkh"][1]])
    got["dv"] = torch.cat([held["dv"][1], held["dvh"][1]])
    deg = rowptr.diff()
    assert (got["stat_l"][deg == 0] == 0).all() and (got["out"][deg == 0] == 0).all()
    check(f"kernels C={C} heads={heads} s={s}", got, C, heads, s)


@pytest.mark.parametrize("side", ["no destination rows", "no entries", "halo sources only",
                                  "kh of 0 rows"])
def test_empty_sides(side):
    """Nothing attended to gives zeros (or empty gradients); an empty first or second source
    gives the bits of the same attention with the other source as the only one."""
    from dgraph_amd.ops.gat import GatPattern

    C, heads = 64, 2
    rowptr, col, _ = pattern()
    d = inputs(C, heads, 0.5)
    pat = lambda rp, cl, ns, nh: GatPattern(rp.to(DEV), cl.to(DEV), ns, nh)  # noqa: E731
    if side == "no destination rows":
        got = run_op(d, pat(rowptr[:1], col[:0], 5, 3), 5, 3, heads, nq=0)
        assert got[0].shape == (0, C) and all(int(t.count_nonzero()) == 0 for t in got)
    elif side == "no entries":
        got = run_op(d, pat(torch.zeros_like(rowptr), col[:0], LS, HS), LS, HS, heads)
        assert all(int(t.count_nonzero()) == 0 for t in got)
    elif side == "halo sources only":
        out, dq, dk, dv, dkh, dvh = run_op(d, pat(rowptr, col % HS, 0, HS), 0, HS, heads)
        one = run_op(d, pat(rowptr, col % HS, HS, 0), HS, None, heads)
        assert dk.shape == dv.shape == (0, C)
        for a, b in zip((out, dq, dkh, dvh), one):
            assert torch.equal(a, b) and torch.isfinite(a).all()
    else:
        *got, dkh, dvh = run_op(d, pat(rowptr, col, N, 0), N, 0, heads)
        assert dkh.shape == dvh.shape == (0, C)
        for a, b in zip(got, run_op(d, pat(rowptr, col, N, 0), N, None, heads)):
            assert torch.equal(a, b) and torch.isfinite(a).all()


def test_unsupported_bf16_combinations_raise():
    from dgraph_amd import _native
    from dgraph_amd.ops import dot_attention
    from dgraph_amd.ops.gat import GatPattern

    rowptr, col, _ = pattern()
    pat = GatPattern(rowptr.to(DEV), col.to(DEV), N, 0)
    f = lambda n, dt=BF: torch.randn(n, 64, device=DEV).to(dt)  # noqa: E731
    for kw in (dict(v=f(N, torch.float32)), dict(edge=f(col.numel())), dict(dropout_p=0.1),
               dict(allow_bf16=False)):  # (the last: bf16 stays opt-in)
        with pytest.raises(ValueError, match="64, 128, 256"):
            dot_attention(f(R), f(N), kw.pop("v", f(N)), pat, heads=2,
                          **{"allow_bf16": True, **kw})
    m = torch.empty(R, 2, device=DEV)
    with pytest.raises(RuntimeError, match="int32"):  # the binding: no int64 columns
        _native.ops().dot_attn_fwd_bf16(rowptr.to(DEV), col.to(DEV), f(R), f(N), f(N), None,
                                        None, N, f(R), m, torch.empty_like(m), 2, 0.125)


def test_transformer_conv_bf16_gpu_vs_cpu():
    """The bf16 layer on the GPU against the same bf16 layer on the CPU (whose op path evaluates
    in fp64 and returns bf16), W = 1. Margin 2^-6 of the array's largest magnitude, four bf16
    ulps: the layer rounds four times (q, kv, the attention output, the final sum) and a GPU
    and a CPU GEMM may sum in different orders and flip each rounding by one ulp."""
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

    def run(dev):
        layer = copy.deepcopy(base).to(dev).bfloat16()
        a, b = (t.to(dev, BF).requires_grad_() for t in (xd, xs))
        out = layer(a, build_relation_graph(edges, 1, 0, offs, 0, 1).to(dev), x_j=b)
        assert out.dtype == BF and out.device.type == torch.device(dev).type
        grads = torch.autograd.grad(out, [a, b] + list(layer.parameters()), w.to(dev, BF))
        return [out.detach()] + list(grads)

    names = ["out", "dx", "dx_j"] + [n for n, _ in base.named_parameters()]
    for n, a, b in zip(names, run(DEV), run("cpu")):
        a, b = a.double().cpu(), b.double()
        rel = float((a - b).abs().max() / b.abs().max())
        print(f"layer {n}: largest |GPU - CPU| / max|CPU| {rel:.2e} (margin {2.0 ** -6:.2e})")
        assert a.shape == b.shape and rel <= 2.0 ** -6, (n, rel)
