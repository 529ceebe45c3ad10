"""The GATv2 attention kernels with bf16 storage (csrc/kernels/gatv2_bf16.hip): the op
``ops.gatv2_attention`` on bf16 rows, the three kernels called directly, the empty sides, the
refusals and a bf16 ``CommAwareGATv2Conv``. Reference and bounds: tests/test_gatv2_bf16.py;
nothing is taken from the kernels' own output. The degree-1 rows (reference dl exactly 0) are
what a ``c`` taken from the rounded output, or a contracted ``T1 - c T2``, fails. Largest
error / bound seen on an MI355X (a record, not an input to the bounds; the tests print every
figure before asserting; a bf16 array comes close to 1 because one rounding errs by up to 2^-8
of the value):

    the op       out 0.981   dl 0.975   dr 0.966   datt 0.185
    the kernels  out 0.981   dl 0.975   dr 0.966   da 0.185 (fp64 host sum of da_part)
                 stat_m 0.009   stat_l 0.121   c 0.111
    the layer    largest |GPU - CPU| / max|CPU| over the output and the 9 gradients: 9.8e-4
                 (lin_dst.bias; equal bits in eight of the ten; the margin is 2^-6 = 0.0156)
"""
from __future__ import annotations

import pytest
import torch

from test_dot_attn import CIN, ND, NS, _edges
from test_gat_kernels import HS, LS, N, PAIRS, R, pattern, transpose
from test_gatv2_bf16 import SCALES, SLOPE, bounds, inputs, reference

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


def run_op(d, pat, ns, nh, heads, nq=R, **kw):
    """out and the gradients of ``gatv2_attention`` on bf16 rows: xs the first ``ns`` sources,
    xsh the next ``nh`` (``None`` without any: one source); att fp32."""
    from dgraph_amd.ops import gatv2_attention

    mk = lambda t: t.to(DEV, BF).requires_grad_()  # noqa: E731
    l, r, a = mk(d["l"][:nq]), mk(d["r"][:ns]), d["a"].to(DEV).requires_grad_()
    rh = None if nh is None else mk(d["r"][ns:ns + nh])
    out = gatv2_attention(l, r, a, pat, rh, heads=heads, negative_slope=SLOPE,
                          **{"allow_bf16": True, **kw})
    ins = [t for t in (l, r, a, rh) if t is not None]
    grads = torch.autograd.grad(out, ins, d["g"][:nq].to(DEV, BF))
    for t, gr in zip([l] + ins, (out,) + grads):
        assert gr.dtype == t.dtype and gr.shape == t.shape  # (bf16 rows, fp32 datt)
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
    out, dl, dr, da, *halo = got
    check(f"op C={C} heads={heads} s={s} two={two}",
          dict(out=out, dl=dl, dr=torch.cat([dr] + halo), da=da), C, heads, s)


def _wide(t, fill, dtype=BF):
    """``t`` as the upper column half of a [rows, 2 cols] buffer holding ``fill`` elsewhere."""
    buf = torch.full((t.shape[0], 2 * t.shape[1]), fill, dtype=dtype, device=DEV)
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
    l, g, r, rh = (_wide(t, nan)[1] for t in (d["l"], d["g"], d["r"][:LS], d["r"][LS:]))
    att = d["a"].to(DEV)
    P = ops.gatv2_bf16_da_parts(R, C)
    assert P == (-(-R // (512 // C)) + 3) // 4 > 1  # ceil(ceil(R / rows per wave) / 4)

    def run():
        held = {}  # name -> (whole buffer, the part the kernels may write: NaN on entry)

        def out(name, rows, cols=None):  # bf16 [rows, C], or fp32 [rows, cols]
            held[name] = _wide(torch.full((rows, cols or C), nan), SENT,
                               torch.float32 if cols else BF)
            return held[name][1]

        o, m, li, c = out("out", R), out("stat_m", R, heads), out("stat_l", R, heads), \
            out("c", R, heads)
        dap = torch.full((P, C), nan, device=DEV)
        held["da_part"] = (dap, dap)
        ops.gatv2_fwd_bf16(rp, cl, l, r, rh, LS, att, o, m, li, heads, SLOPE)
        ops.gatv2_bwd_dst_bf16(rp, cl, l, r, rh, LS, att, m, li, g, c, out("dl", R), dap, heads,
                               SLOPE)
        for nm, rs, n, tr in (("dr", r, LS, trp[:LS + 1]), ("drh", rh, HS, trp[LS:])):
            ops.gatv2_bwd_src_bf16(tr, tcl, l, g, rs, att, m, li, c, out(nm, n), heads, SLOPE)
        torch.cuda.synchronize()
        return held

    held, again = run(), run()
    for name, (buf, view) in held.items():
        assert torch.equal(buf, again[name][0]), name  # two calls, equal bits (no NaN is left)
        outside = torch.ones_like(buf, dtype=torch.bool)
        outside[:, buf.shape[1] - view.shape[1]:] = False
        assert (buf[outside] == torch.tensor(SENT, dtype=buf.dtype)).all(), name
    got = {n: held[n][1] for n in ("out", "stat_m", "stat_l", "c", "dl")}
    got["dr"] = torch.cat([held["dr"][1], held["drh"][1]])
    got["da"] = held["da_part"][1].double().sum(0)  # (finite: every row of da_part is written)
    deg = rowptr.diff()
    for n in ("stat_l", "out", "dl"):
        assert (got[n][deg == 0] == 0).all(), n
    assert (got["dl"][deg == 1] == 0).all()  # alpha = 1, c = ga: T1 = fl(c T2) exactly
    check(f"kernels C={C} heads={heads} s={s}", got, C, heads, s)


@pytest.mark.parametrize("side", ["no destination rows", "no entries", "halo sources only",
                                  "xsh of 0 rows"])
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
        out, dl, dr, da, drh = run_op(d, pat(rowptr, col % HS, 0, HS), 0, HS, heads)
        assert dr.shape == (0, C)
        for a, b in zip((out, dl, drh, da), run_op(d, pat(rowptr, col % HS, HS, 0), HS, None,
                                                   heads)):
            assert torch.equal(a, b) and torch.isfinite(a).all()
    else:
        *got, drh = run_op(d, pat(rowptr, col, N, 0), N, 0, heads)
        assert drh.shape == (0, C)
        for a, b in zip(got, run_op(d, pat(rowptr, col, N, 0), N, None, heads)):
            assert torch.equal(a, b) and torch.isfinite(a).all()


def test_refusals():
    from dgraph_amd import _native
    from dgraph_amd.ops import gatv2_attention
    from dgraph_amd.ops.gat import GatPattern

    ops = _native.ops()
    rowptr, col, _ = pattern()
    pat = GatPattern(rowptr.to(DEV), col.to(DEV), N, 0)
    f = lambda n, dt=BF, w=64: torch.randn(n, w, device=DEV).to(dt)  # noqa: E731
    att = torch.randn(64, device=DEV)
    for xs, kw in ((f(N, torch.float32), {}), (f(N), dict(allow_bf16=False))):
        with pytest.raises(ValueError, match="64, 128, 256"):  # (bf16 stays opt-in)
            gatv2_attention(f(R), xs, att, pat, heads=2, **{"allow_bf16": True, **kw})
    rp, ci = rowptr.to(DEV), col.int().to(DEV)
    odd = torch.empty(N * 64 + 8, dtype=BF, device=DEV)[1:1 + N * 64].view(N, 64)
    for cl, xs, msg in ((col.to(DEV), f(N), "int32"), (ci, odd, "alignment"),
                        (ci, f(N, w=68)[:, :64], "stride")):
        outs = [f(R), torch.randn(R, 2, device=DEV), torch.randn(R, 2, device=DEV)]
        before = [t.clone() for t in outs]
        with pytest.raises(RuntimeError, match=msg):
            ops.gatv2_fwd_bf16(rp, cl, f(R), xs, None, N, att, *outs, 2, SLOPE)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(outs, before))


@pytest.mark.parametrize("autocast", [False, True], ids=["bf16_layer", "autocast"])
def test_gatv2_conv_bf16_gpu_vs_cpu(autocast):
    """The bf16 layer on the GPU against the same bf16 layer on the CPU (whose op path evaluates
    in fp64 and returns bf16), W = 1. Margin 2^-6 of the array's largest magnitude, four bf16
    ulps, as test_transformer_conv_bf16_gpu_vs_cpu argues: this layer also rounds four times (l,
    r, the attention output, the final sum) and a GPU and a CPU GEMM may sum in different orders
    and flip each rounding by one ulp. Under autocast (fp32 parameters) only that it runs on the
    bf16 kernels and returns bf16."""
    import copy

    from dgraph_amd.data.hetero import build_relation_graph, get_vertex_offsets
    from dgraph_amd.models import CommAwareGATv2Conv

    edges = _edges()
    offs = {0: get_vertex_offsets(ND, 1), 1: get_vertex_offsets(NS, 1)}
    torch.manual_seed(0)
    base = CommAwareGATv2Conv(CIN, 64, heads=2, residual=True, hetero=True)
    with torch.no_grad():
        base.bias.normal_()
    gen = torch.Generator().manual_seed(1)
    xd, xs, w = (torch.randn(n, c, generator=gen) for n, c in ((ND, CIN), (NS, CIN), (ND, 64)))
    rel = lambda dev: build_relation_graph(edges, 1, 0, offs, 0, 1).to(dev)  # noqa: E731
    if autocast:
        layer = copy.deepcopy(base).to(DEV)
        with torch.autocast("cuda", torch.bfloat16):
            out = layer(xd.to(DEV).requires_grad_(), rel(DEV), x_j=xs.to(DEV))
        assert out.dtype == BF
        out.backward(w.to(DEV, BF))
        assert all(p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all()
                   for p in layer.parameters())
        return

    def run(dev):
        layer = copy.deepcopy(base).to(dev).bfloat16()
        a, b = (t.to(dev, BF).requires_grad_() for t in (xd, xs))
        out = layer(a, rel(dev), x_j=b)
        assert out.dtype == BF and out.device.type == torch.device(dev).type
        grads = torch.autograd.grad(out, [a, b] + list(layer.parameters()), w.to(dev, BF))
        return [out.detach()] + list(grads)

    names = ["out", "dx", "dx_j"] + [n for n, _ in base.named_parameters()]
    for n, a, b in zip(names, run(DEV), run("cpu")):
        a, b = a.double().cpu(), b.double()
        rel_err = float((a - b).abs().max() / b.abs().max())
        print(f"layer {n}: largest |GPU - CPU| / max|CPU| {rel_err:.2e} (margin {2.0 ** -6:.2e})")
        assert a.shape == b.shape and rel_err <= 2.0 ** -6, (n, rel_err)
