"""The relation-attention kernels with bf16 storage (csrc/kernels/gat_bf16.hip): the autograd
op ``ops.gat.gat_relation_into`` on bf16 rows, the three kernels called directly, and the
bf16 lean RGAT model.

Reference: ``ops/gat.py::_reference`` under autograd in fp64 on the bf16-rounded inputs
widened exactly (the ``into`` prefill is one of them); the same in fp32 on the CPU gives
``ref32``. With ``b = test_gat_kernels.bound(ref64, ref32)``: fp32 outputs (stat_m, stat_l,
gsd, ga) err <= b; bf16 outputs (out, gz, gzh) err <= b + 2^-8 (|ref64| + b) elementwise —
one round-to-nearest-even of the fp32 result at 7 stored mantissa bits. Nothing is taken from
the kernels' own output. Largest error / bound seen on an MI355X (a record, not an input to
the bounds; the tests print every figure before asserting):

    the op       out 0.990   gz 0.973   gzh 0.982   gsd 0.217   ga 0.240
    the kernels  out 0.990   gz 0.973   gzh 0.982   gsd 0.217   ga 0.231
                 stat_m 0.007   stat_l 0.137
    the model    largest |loss16 - loss32| / loss32 over 6 steps: 0.0005

(The bf16 arrays come close to 1: a round-to-nearest-even of a value just above a power of
two errs by up to 2^-8 of it, which is the bound's second term.)
"""
from __future__ import annotations

import pytest
import torch

from test_gat_bf16 import bounds, inputs, reference
from test_gat_kernels import HS, LS, N, PAIRS, R, SLOPE, pattern, transpose

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.25e9
RATIOS: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _native_and_record():
    from dgraph_amd import _native

    assert _native.load(), "native library missing"
    yield
    for k in sorted(RATIOS):
        print(f"\n[gat-bf16] largest error / bound, {k}: {RATIOS[k]:.3f}", end="")
    print()


def check(tag, got, C, heads, s, two):
    ref64 = reference(C, heads, s, two, torch.float64)
    ref32 = reference(C, heads, s, two, torch.float32)
    deg = pattern()[0].diff()
    for k, t in got.items():
        t, r64, r32 = t.detach().double().cpu(), ref64[k], ref32[k]
        assert t.shape == r64.shape, (tag, k, t.shape, r64.shape)
        if k == "stat_m":  # (an empty row's maximum is unspecified)
            t, r64, r32 = t[deg > 0], r64[deg > 0], r32[deg > 0]
        assert torch.isfinite(t).all(), (tag, k)
        b, bd = bounds(k, r64, r32)
        ratio = float(((t - r64).abs() / bd).max())
        key = f"{tag.split()[0]}:{k}"
        RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
        print(f"{tag} {k}: bound {b:.3e} largest err / bound {ratio:.3f}")
        assert ratio <= 1.0, (tag, k, ratio)


@pytest.mark.parametrize("two", [False, True], ids=["one_source", "zh_static"])
@pytest.mark.parametrize("s", [0.5, 30.0])
@pytest.mark.parametrize("C,heads", PAIRS)
def test_op_against_fp64(C, heads, s, two):
    import dgraph_amd.ops.gat as G

    rowptr, col, _ = pattern()
    d = inputs(C, heads, s)
    ns, nh = (LS, HS) if two else (N, 0)
    pat = G.GatPattern(rowptr.to(DEV), col.to(DEV), ns, nh)

    def run():
        mk = lambda t, dt: t.to(DEV, dt).requires_grad_()  # noqa: E731
        z, sd, a = mk(d["z"][:ns], torch.bfloat16), mk(d["sd"], torch.float32), \
            mk(d["a"], torch.float32)
        zh = mk(d["z"][ns:], torch.bfloat16) if two else None
        out = G.gat_relation_into(z, sd, a, d["into"].to(DEV, torch.bfloat16), pat,
                                  zh_static=zh)
        assert out.dtype == torch.bfloat16
        ins = [t for t in (z, zh, sd, a) if t is not None]
        grads = torch.autograd.grad(out, ins, d["g"].to(DEV, torch.bfloat16))
        for t, gr in zip(ins, grads):
            assert gr.dtype == t.dtype and gr.shape == t.shape
        names = [n for n, t in zip(("gz", "gzh", "gsd", "ga"), (z, zh, sd, a)) if t is not None]
        return dict(zip(names, grads), out=out.detach())

    got, again = run(), run()
    for k in got:
        assert torch.equal(got[k], again[k]), k
    check(f"op C={C} heads={heads} s={s} two={two}", got, C, heads, s, two)


def _wide(t, fill):
    """``t`` as the upper column half of a [rows, 2C] bf16 buffer holding ``fill`` elsewhere."""
    buf = torch.full((t.shape[0], 2 * t.shape[1]), fill, dtype=torch.bfloat16, device=DEV)
    buf[:, t.shape[1]:] = t.to(DEV)
    return buf, buf[:, t.shape[1]:]


@pytest.mark.parametrize("s", [0.5, 30.0])
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
    z, zh, g = (_wide(t, nan)[1] for t in (d["z"][:LS], d["z"][LS:], d["g"]))
    sd, a = d["sd"].to(DEV), d["a"].reshape(-1).to(DEV)
    parts = {n: ops.gat_bf16_da_parts(n, C) for n in (LS, HS)}
    for n, P in parts.items():  # one row per wave of 512 / C row groups
        assert P == -(-n // (512 // C))

    def run():
        held = {}  # name -> (whole buffer, the part the kernels may write)

        def out(name, rows, cols, dtype, wide=False):
            if wide:
                buf, view = _wide(torch.full((rows, cols), nan), SENT)
            else:  # one sentinel row past the end
                buf = torch.full((rows + 1, cols), SENT, dtype=dtype, device=DEV)
                view = buf[:rows]
            held[name] = (buf, view)
            return view

        f32 = torch.float32
        o = out("out", R, C, None, wide=True)
        o.copy_(d["into"])
        m, l = out("stat_m", R, heads, f32), out("stat_l", R, heads, f32)
        c, gsd = out("c", R, heads, f32), out("gsd", R, heads, f32)
        ops.gat_fwd_bf16(rp, cl, z, zh, LS, a, sd, o, 1.0, m, l, heads, SLOPE)
        ops.gat_bwd_dst_bf16(rp, cl, z, zh, LS, a, sd, m, l, g, c, gsd, heads, SLOPE)
        for nm, rows, n, tr in (("", z, LS, trp[:LS + 1]), ("h", zh, HS, trp[LS:])):
            ops.gat_bwd_src_bf16(tr, tcl, g, rows, a, sd, m, l, c,
                                 out("gz" + nm, n, C, None, wide=True),
                                 out("gss" + nm, n, heads, f32),
                                 out("da" + nm, parts[n], C, f32), heads, SLOPE)
        torch.cuda.synchronize()
        return held

    held, again = run(), run()
    for k, (buf, view) in held.items():
        assert torch.equal(buf, again[k][0]), k  # two calls, equal bits (no NaN is left)
        outside = torch.ones_like(buf, dtype=torch.bool)
        outside[:view.shape[0], buf.shape[1] - view.shape[1]:] = False
        assert (buf[outside] == torch.tensor(SENT, dtype=buf.dtype)).all(), k
        assert not (view == torch.tensor(SENT, dtype=buf.dtype)).any(), k  # every slot written
    got = {k: held[k][1] for k in ("out", "stat_m", "stat_l", "gsd", "gz", "gzh")}
    got["ga"] = (held["da"][1].double().sum(0) + held["dah"][1].double().sum(0)).view(heads, -1)
    deg = rowptr.diff()
    assert (got["stat_l"][deg == 0] == 0).all() and (got["gsd"][deg == 0] == 0).all()
    check(f"kernels C={C} heads={heads} s={s}", got, C, heads, s, True)


def test_binding_rejects_int64_columns():
    from dgraph_amd import _native

    ops = _native.ops()
    rowptr, col, _ = pattern()
    d = inputs(64, 2, 0.5)
    z = d["z"].to(DEV, torch.bfloat16)
    m = torch.empty(R, 2, device=DEV)
    with pytest.raises(RuntimeError, match="int32"):
        ops.gat_fwd_bf16(rowptr.to(DEV), col.to(DEV), z, None, N, d["a"].reshape(-1).to(DEV),
                         d["sd"].to(DEV), d["into"].to(DEV, torch.bfloat16), 1.0, m,
                         torch.empty_like(m), 2, SLOPE)


def test_model_bf16_follows_fp32():
    """CommAwareRGAT on a tiny HeteroGraph: bf16 features (fp32 parameters) against fp32 from
    equal weights; the 5 % of tests/test_precision_gpu.py's bf16 SAGE stack."""
    import torch.nn.functional as F

    from dgraph_amd.data.mag import (EDGE_TYPES, HETERO_SHAPES, build_hetero_partition,
                                     hetero_node_data)
    from dgraph_amd.models.rgat import CommAwareRGAT
    from dgraph_amd.models.rgcn import HeteroGraph

    shape = HETERO_SHAPES["mag240m"].scaled(1e-4)
    part = build_hetero_partition(shape, 0, 1, "cpu", global_frac=0.2, window=256)
    feats, y, tr = hetero_node_data(shape, 0, part["offsets"], "cpu", dtype=torch.float32)
    part = {"offsets": part["offsets"], "sources": {
        s: {k: (v.to(DEV) if hasattr(v, "to") else v) for k, v in d.items()}
        for s, d in part["sources"].items()}}
    g = HeteroGraph.from_partition(part, EDGE_TYPES)
    y, idx = y.to(DEV), torch.nonzero(tr).squeeze(1).to(DEV)
    losses = {}
    for dtype in (torch.float32, torch.bfloat16):
        torch.manual_seed(0)
        m = CommAwareRGAT(64, shape.num_classes, 64, 5, 2, 4, dropout=0.0).to(DEV)
        xs = {t: v[:, :64].to(DEV, dtype).contiguous() for t, v in feats.items()}
        opt = torch.optim.Adam(m.parameters(), lr=2e-3)
        losses[dtype] = []
        for _ in range(6):
            loss = F.cross_entropy(m(xs, g)[idx].float(), y[idx])
            loss.backward()
            opt.step()
            opt.zero_grad()
            losses[dtype].append(float(loss.detach()))
    l32, l16 = (torch.tensor(losses[k]) for k in (torch.float32, torch.bfloat16))
    rel = (l16 - l32).abs() / l32
    print(f"model fp32 {l32.tolist()} bf16 {l16.tolist()} largest rel {float(rel.max()):.4f}")
    assert torch.isfinite(l16).all() and torch.isfinite(l32).all()
    assert float(rel.max()) < 0.05, rel.tolist()
