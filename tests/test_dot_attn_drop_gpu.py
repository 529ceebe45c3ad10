"""The fused dot-product attention kernels with attention dropout
(csrc/kernels/dot_attn_drop_f32.hip, called through ``_native.ops().dot_attn_drop_*_f32``
directly), ``dot_attention(..., dropout_p=, dropout_seed=)`` and
``CommAwareTransformerConv(dropout=)`` on the GPU against the fp64 evaluation of their contract
(tests/test_dot_attn_drop.py), at every ``(C, heads)`` instantiation and both index types.

Pattern and inputs: see tests/test_dot_attn.py (37 rows over 41 local + 19 halo sources with
rows of degree 0, 1, LPR +- 1 and a 301-entry hub; score scales 0.5 and 40), p = 0.1 and 0.5
with the seed of tests/test_dot_attn_drop.py. The keep mask is regenerated bit for bit on the
CPU (``ops/philox.py``), so these are exact comparisons, not statistical ones. The backward
kernels get ``c`` from the fp64 oracle, rounded to fp32.

Bound per compared array: ``max(2e-5, 8 err32) max(1, max|fp64|)`` with ``err32`` the error of
the same formula evaluated in fp32 on the CPU (``test_gat_kernels.bound``) — nothing is taken
from the kernels' own output. ``stat_m`` / ``stat_l`` are also compared with the PLAIN forward
kernel's on the same inputs under the same bound (dropout does not enter the softmax
statistics). Largest ``error / bound`` seen on an MI355X (a record, not an input to the bound;
the tests print every figure before asserting):

    dot_attn_drop_fwd      out 0.085   stat_m 0.007   stat_l 0.207
                           (stat_m / stat_l against the plain forward's: error 0 everywhere)
    dot_attn_drop_bwd_dst  dq 0.233
    dot_attn_drop_bwd_src  dk 0.267    dv 0.261
    the op                 out 0.085   dq 0.135   dk 0.156   dv 0.261
    the layer              out 0.005   dx 0.010   dx_j 0.010   parameters 0.015 or less
"""
from __future__ import annotations

import pytest
import torch

from test_dot_attn import ND, NS, SCALES, _edges, case
from test_dot_attn_drop import (DROP_OUTPUTS, PS, SEED, drop_oracle, keep_mask,
                                layer_pieces_dense)
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
        print(f"\n[dot-attn-drop] largest error / bound, {k}: {RATIOS[k]:.3f}", end="")
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


def _seed(value=SEED):
    return torch.tensor([value], dtype=torch.int64, device=DEV)


class _Buffers:
    """Device operands of one run of the three kernels. ``wide``: every feature array is
    the upper column half of a [rows, 2C] buffer and every per-head array the upper half of
    a [rows, 2 heads] buffer (one head: column 2 of a [rows, 4] buffer); inputs hold NaN
    outside their slice, outputs ``SENT``. Outputs hold NaN inside on entry."""

    def __init__(self, d, c64, idx, two, p, wide=False):
        rowptr, col, _ = pattern()
        t_rowptr, t_col = transpose(rowptr, col, N)
        self.heads, self.two, self.p, self.wide = d["heads"], two, p, wide
        self.scale = d["scale"]
        self.seed = _seed()
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
        self.c = self._in(c64.float())
        C, Hh = d["C"], d["heads"]
        self.out = self._out("out", R, C)
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
        ops, h, sc, p, sd = _ops(), self.heads, self.scale, self.p, self.seed
        ops.dot_attn_drop_fwd_f32(self.rowptr, self.col, self.q, self.k, self.v, self.k2,
                                  self.v2, self.ns, self.out, self.m, self.l, sd, p, h, sc)
        ops.dot_attn_drop_bwd_dst_f32(self.rowptr, self.col, self.q, self.k, self.v, self.k2,
                                      self.v2, self.ns, self.m, self.l, self.g, self.c,
                                      self.dq, sd, p, h, sc)
        # the source side: local rows, then the halo rows over the tail of the transposed
        # row pointer (as ops/dot_attn.py calls it)
        ops.dot_attn_drop_bwd_src_f32(self.t_rowptr[:self.ns + 1], self.t_col, self.t_slot,
                                      self.q, self.g, self.k, self.v, self.m, self.l, self.c,
                                      self.dk, self.dv, sd, p, h, sc)
        if self.two:
            ops.dot_attn_drop_bwd_src_f32(self.t_rowptr[LS:], self.t_col, self.t_slot, self.q,
                                          self.g, self.k2, self.v2, self.m, self.l, self.c,
                                          self.dk2, self.dv2, sd, p, h, sc)
        torch.cuda.synchronize()
        res = {"out": self.out, "stat_m": self.m, "stat_l": self.l, "dq": self.dq,
               "dk": self.dk, "dv": self.dv}
        if self.two:
            res["dk"] = torch.cat([self.dk, self.dk2])
            res["dv"] = torch.cat([self.dv, self.dv2])
        return {k: v.clone() for k, v in res.items()}

    def plain_stats(self):
        """stat_m, stat_l of the plain forward kernel (dot_attn_fwd_f32) on these inputs."""
        out, m, l = torch.empty_like(self.out), torch.empty_like(self.m), \
            torch.empty_like(self.l)
        _ops().dot_attn_fwd_f32(self.rowptr, self.col, self.q, self.k, self.v, self.k2, self.v2,
                                self.ns, out, 0.0, m, l, self.heads, self.scale)
        return m, l

    def assert_outside_untouched(self):
        for name, buf, sl in self.held:
            keep = torch.ones(buf.shape[1], dtype=torch.bool, device=DEV)
            keep[sl] = False
            rest = buf[:, keep]
            assert torch.equal(rest, torch.full_like(rest, SENT)), name


def _check(tag, got, C, heads, s, p):
    r64, r32 = drop_oracle(C, heads, s, p)
    rowptr, _, rows = pattern()
    full = rowptr[1:] > rowptr[:-1]
    for k in DROP_OUTPUTS:
        if k == "stat_m":  # (an empty row's maximum is not part of the contract)
            _compare(tag, k, got[k][full.to(DEV)], r64[k][full], r32[k][full])
        else:
            _compare(tag, k, got[k], r64[k], r32[k])
    assert (got["stat_l"][(~full).to(DEV)] == 0).all()
    # rows (per head) with no kept edge, the empty rows among them: exact zeros
    kept = torch.zeros(R, heads).index_add(0, rows, keep_mask(heads, p).float())
    dead = (kept == 0).repeat_interleave(C // heads, 1).to(DEV)
    assert dead.any()
    assert (got["out"][dead] == 0).all()
    assert (got["dq"][dead] == 0).all()  # (c, an input, is the oracle's: 0 there)


def _run_twice(C, heads, s, idx, two, p, wide=False):
    """Two runs on fresh buffers: bitwise equal (fixed summation orders, no atomics, a fixed
    seed). The statistics against the plain forward's under the oracle's bound."""
    d, r = case(C, heads, s), drop_oracle(C, heads, s, p)
    a, b = _Buffers(d, r[0]["c"], idx, two, p, wide), _Buffers(d, r[0]["c"], idx, two, p, wide)
    ra, rb = a.run(), b.run()
    for k in ra:
        assert torch.equal(ra[k].view(torch.int32), rb[k].view(torch.int32)), k
    a.assert_outside_untouched()
    m, l = a.plain_stats()
    full = (pattern()[0][1:] > pattern()[0][:-1])
    for name, mine, plain in (("stat_m", ra["stat_m"], m), ("stat_l", ra["stat_l"], l)):
        bd = bound(r[0][name][full], r[1][name][full])
        err = float((mine[full.to(DEV)] - plain[full.to(DEV)]).abs().max())
        print(f"C={C} heads={heads} s={s} p={p} {name} against the plain forward: err {err:.3e} "
              f"bound {bd:.3e}")
        assert err <= bd, (name, err, bd)
    return ra


@pytest.mark.parametrize("idx", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("C,heads", PAIRS)
def test_dot_attn_drop_kernels_vs_fp64(C, heads, s, idx):
    """Forward, destination side, source side (local rows, halo rows) at one instantiation:
    with a second source split at 41 and with all 60 rows local, at p = 0.1 and 0.5."""
    for two in (True, False):
        for p in PS:
            got = _run_twice(C, heads, s, idx, two, p)
            _check(f"kernels C={C} heads={heads} s={s} p={p} "
                   f"{'two' if two else 'one'}-source", got, C, heads, s, p)


@pytest.mark.parametrize("two", [True, False], ids=["two-source", "one-source"])
@pytest.mark.parametrize("C,heads", [(64, 1), (128, 4), (256, 2), (256, 8)])
def test_dot_attn_drop_kernels_wide_operands(C, heads, two):
    """Every operand a column slice of a wider buffer (row strides 2C and 2 heads / 4):
    inputs hold NaN outside the slices; outputs keep their sentinel there bitwise."""
    for p in PS:
        got = _run_twice(C, heads, 0.5, torch.int32, two, p, wide=True)
        _check(f"kernels wide C={C} heads={heads} p={p}", got, C, heads, 0.5, p)


# --------------------------------------------------- contract checks (bindings_dot_attn.cpp)
def _valid_args(C, heads):
    rowptr, col, _ = pattern()
    t_rowptr, t_col = transpose(rowptr, col, N)
    f = lambda *shape: torch.randn(*shape, device=DEV)  # noqa: E731
    return dict(rowptr=rowptr.to(DEV), col=col.to(torch.int32).to(DEV), q=f(R, C), k=f(N, C),
                v=f(N, C), k2=None, v2=None, nsplit=N, out=f(R, C), stat_m=f(R, heads),
                stat_l=f(R, heads), g=f(R, C), c=f(R, heads), dq=f(R, C),
                t_rowptr=t_rowptr.to(DEV), t_col=t_col.to(torch.int32).to(DEV),
                t_slot=_t_slot(col).to(torch.int32).to(DEV), dk=f(N, C), dv=f(N, C),
                seed=_seed(), p=0.5, heads=heads, scale=0.125)


_CALLS = {
    "fwd": ("dot_attn_drop_fwd_f32",
            ("rowptr", "col", "q", "k", "v", "k2", "v2", "nsplit", "out", "stat_m", "stat_l",
             "seed", "p", "heads", "scale"), ("out", "stat_m", "stat_l")),
    "dst": ("dot_attn_drop_bwd_dst_f32",
            ("rowptr", "col", "q", "k", "v", "k2", "v2", "nsplit", "stat_m", "stat_l", "g", "c",
             "dq", "seed", "p", "heads", "scale"), ("dq",)),
    "src": ("dot_attn_drop_bwd_src_f32",
            ("t_rowptr", "t_col", "t_slot", "q", "g", "k", "v", "stat_m", "stat_l", "c", "dk",
             "dv", "seed", "p", "heads", "scale"), ("dk", "dv")),
}
_ALL = ("fwd", "dst", "src")


def _violate(what):
    """(the arguments, the ops that must refuse them)."""
    if what == "C=96":
        return _valid_args(96, 2), _ALL
    if what == "heads=3":
        return _valid_args(64, 3), _ALL
    A = _valid_args(64, 2)
    if what == "seed on the CPU":
        A["seed"] = torch.tensor([SEED])
    elif what == "seed int32":
        A["seed"] = _seed().to(torch.int32)
    elif what == "seed with two elements":
        A["seed"] = torch.tensor([SEED, SEED], device=DEV)
    elif what == "p = 1":
        A["p"] = 1.0
    elif what == "p < 0":
        A["p"] = -0.5
    elif what == "k offset by one float":
        flat = torch.empty(N * 64 + 4, device=DEV)
        A["k"] = flat[1:1 + N * 64].view(N, 64).normal_()
        assert A["k"].data_ptr() % 16 == 4
    elif what == "t_slot of the other integer dtype":
        A["t_slot"] = A["t_slot"].long()
        return A, ("src",)
    elif what == "t_slot one entry short":
        A["t_slot"] = A["t_slot"][:-1]
        return A, ("src",)
    else:
        raise KeyError(what)
    return A, _ALL


@pytest.mark.parametrize("what", ["seed on the CPU", "seed int32", "seed with two elements",
                                  "t_slot of the other integer dtype", "t_slot one entry short",
                                  "p = 1", "p < 0", "k offset by one float", "C=96", "heads=3"])
def test_dot_attn_drop_contract_checks_raise_before_launch(what):
    A, refused = _violate(what)
    for op in refused:
        name, args, outs = _CALLS[op]
        before = {k: A[k].clone() for k in outs}
        with pytest.raises(RuntimeError):
            getattr(_ops(), name)(*[A[k] for k in args])
        torch.cuda.synchronize()
        for k, t in before.items():
            assert torch.equal(A[k], t), (op, k)
    if what == "p = 1":  # the valid arguments run
        A["p"] = 0.5
        for name, args, _ in _CALLS.values():
            getattr(_ops(), name)(*[A[k] for k in args])
        torch.cuda.synchronize()


# -------------------------------------------------------------------------- the autograd op
def _run_op(dev, dtype, C, heads, s, halo, p, seed=SEED):
    """``dot_attention(..., dropout_p=)`` forward + backward; k / v (and kh / vh) are the
    column halves of one [rows, 2C] buffer, as the layer hands them in."""
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
                        None if kvh is None else kvh[:, C:], heads=heads, dropout_p=p,
                        dropout_seed=torch.tensor([seed], device=dev))
    ins = [q, kvl] + ([kvh] if halo else [])
    grads = torch.autograd.grad(out, ins, d["g"].to(dev, dtype))
    gkv = torch.cat(grads[1:], 0)
    return {"out": out.detach(), "dq": grads[0], "dk": gkv[:, :C], "dv": gkv[:, C:]}


@pytest.mark.parametrize("halo", [True, False], ids=["halo", "no_halo"])
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("C,heads,s", [(C, h, 0.5) for C, h in PAIRS] +
                         [(64, 8, 40.0), (128, 1, 40.0), (256, 4, 40.0)])
def test_dot_attention_drop_op_gpu_vs_cpu(C, heads, s, p, halo):
    """out, dq, dk, dv, dkh, dvh of the op against its CPU path at fp64 (which
    tests/test_dot_attn_drop.py ties to the dense evaluation); two runs with one seed are
    bitwise identical, another seed gives another output."""
    ref64 = _run_op("cpu", torch.float64, C, heads, s, halo, p)
    r32 = drop_oracle(C, heads, s, p)[1]
    got = _run_op(DEV, torch.float32, C, heads, s, halo, p)
    got2 = _run_op(DEV, torch.float32, C, heads, s, halo, p)
    tag = f"op C={C} heads={heads} s={s} p={p} halo={halo}"
    for k in got:
        assert ref64[k].dtype == torch.float64
        assert torch.equal(got[k], got2[k]), k
        _compare(tag, k, got[k], ref64[k], r32[k])
    other = _run_op(DEV, torch.float32, C, heads, s, halo, p, seed=SEED + 1)
    assert not torch.equal(other["out"], got["out"])


@pytest.mark.parametrize("p", PS)
def test_gpu_keep_mask_equals_cpu_mask(p):
    """Which edges the kernels keep, read off the output: C = 64, one head, 64 sources with
    one-hot ``v`` rows and rows of distinct columns, so ``out[i, j] = alpha_ij keep_ij /
    (1 - p)`` is positive exactly for the kept entries (alpha >= e^-16 / 64 here). Rows of
    degree 0, 1, 15..17, 33 and 64: padding lanes, a chunk tail and full chunks."""
    from dgraph_amd.ops import dot_attention
    from dgraph_amd.ops.gat import GatPattern
    from dgraph_amd.ops.philox import attn_keep_mask

    C = 64
    gen = torch.Generator().manual_seed(9)
    deg = torch.tensor([0, 1, 15, 16, 17, 33, 64, 1, 64, 5, 0, 64, 2])
    rowptr = torch.zeros(deg.numel() + 1, dtype=torch.long)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.cat([torch.randperm(C, generator=gen)[:int(n)] for n in deg])
    rows = torch.repeat_interleave(torch.arange(deg.numel()), deg)
    q = torch.randn(deg.numel(), C, generator=gen).clamp_(-1, 1)
    k = torch.randn(C, C, generator=gen).clamp_(-1, 1)       # |score| <= 64 / 8 = 8
    pat = GatPattern(rowptr.to(DEV), col.to(DEV), C, 0)
    for seed in (SEED, 2 ** 62 - 1):
        out = dot_attention(q.to(DEV), k.to(DEV), torch.eye(C, device=DEV), pat, heads=1,
                            dropout_p=p, dropout_seed=_seed(seed)).cpu()
        kept_gpu = out[rows, col] > 0
        want = attn_keep_mask(seed, col.numel(), 1, p)[:, 0]
        assert torch.equal(kept_gpu, want), seed
        assert 0 < int(want.sum()) < want.numel()
        # and nothing outside the pattern's entries
        member = torch.zeros(deg.numel(), C, dtype=torch.bool)
        member[rows, col] = True
        assert (out[~member] == 0).all()
    gpu_mask = attn_keep_mask(_seed(), col.numel(), 1, p)  # the torch generator on the GPU
    assert gpu_mask.is_cuda and torch.equal(gpu_mask.cpu()[:, 0],
                                            attn_keep_mask(SEED, col.numel(), 1, p)[:, 0])


def test_dot_attention_drop_replay_reads_the_seed_tensor():
    """Forward + backward captured once (``GraphedStep``); the seed tensor is rewritten
    between replays: each replay equals the eager result for its seed bitwise, and two seeds
    give different outputs."""
    from dgraph_amd.ops import dot_attention
    from dgraph_amd.ops.gat import GatPattern
    from dgraph_amd.utils.graphed import GraphedStep

    C, heads, p = 128, 4, 0.5
    rowptr, col, _ = pattern()
    d = case(C, heads, 0.5)
    pat = GatPattern(rowptr.to(DEV), col.to(DEV), LS, HS)
    q, g = d["q"].to(DEV).requires_grad_(), d["g"].to(DEV)
    k, v = (d[n][:LS].to(DEV).requires_grad_() for n in ("k", "v"))
    kh, vh = (d[n][LS:].to(DEV).requires_grad_() for n in ("k", "v"))
    seed = _seed(1)

    def step():
        out = dot_attention(q, k, v, pat, kh, vh, heads=heads, dropout_p=p, dropout_seed=seed)
        grads = torch.autograd.grad(out, (q, k, v, kh, vh), g)
        # detached: a result that kept its autograd graph would keep the leaves' gradient
        # accumulators alive, and those stay bound to the stream of the eager calls below, so
        # a later capture would pull that stream in through autograd's stream syncs
        return torch.cat([out.detach().reshape(-1)] + [t.reshape(-1) for t in grads])

    eager = {}
    for value in (SEED, SEED + 1):
        seed.fill_(value)
        eager[value] = step().clone()
    assert not torch.equal(eager[SEED], eager[SEED + 1])
    run = GraphedStep(step, warmup=1)
    seed.fill_(7)
    run()            # warm-up, eager
    run()            # capture and first replay
    assert run.captured
    for value in (SEED, SEED + 1, SEED):
        seed.fill_(value)
        got = run().clone()
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), eager[value].view(torch.int32)), value
    assert run.replays == 4


# --------------------------------------------------------------------------------- the layer
def test_transformer_conv_dropout_gpu_vs_cpu():
    """``CommAwareTransformerConv`` (in 32, out 64, 2 heads, ``dropout=0.5``) in training,
    forward + backward on the GPU against the same layer on the CPU at fp64 with the same
    seed, W = 1; the fp32 error of the bound is the dense evaluation's at fp32. In evaluation
    mode the layer is the one without dropout, bitwise."""
    import copy

    from dgraph_amd.data.hetero import build_relation_graph, get_vertex_offsets
    from dgraph_amd.models.transformer_conv import CommAwareTransformerConv

    edges = _edges()
    offs = {0: get_vertex_offsets(ND, 1), 1: get_vertex_offsets(NS, 1)}
    torch.manual_seed(0)
    base = CommAwareTransformerConv(32, 64, heads=2, hetero=True, dropout=0.5)
    with torch.no_grad():
        base.bias.normal_()
    gen = torch.Generator().manual_seed(1)
    xd, xs, w = (torch.randn(n, c, generator=gen) for n, c in ((ND, 32), (NS, 32), (ND, 64)))

    def run(dev, dtype, dense=False):
        layer = copy.deepcopy(base).to(dev, dtype)
        a, b = (t.to(dev, dtype).requires_grad_() for t in (xd, xs))
        rel = build_relation_graph(edges, 1, 0, offs, 0, 1).to(dev)
        if dense:
            out = layer_pieces_dense(layer, a, b, layer._pattern(rel), SEED)
        else:
            out = layer(a, rel, x_j=b, dropout_seed=torch.tensor([SEED], device=dev))
        grads = torch.autograd.grad(out, [a, b] + list(layer.parameters()), w.to(dev, dtype))
        return [out.detach()] + list(grads)

    ref64, ref32 = run("cpu", torch.float64), run("cpu", torch.float32, dense=True)
    got = run(DEV, torch.float32)
    names = ["out", "dx", "dx_j"] + [n for n, _ in base.named_parameters()]
    assert len(names) == len(got) == 9
    for n, a, b, c in zip(names, got, ref64, ref32):
        _compare("layer", n, a, b, c)
    # evaluation mode: the plain kernels, bitwise the layer without dropout
    rel = build_relation_graph(edges, 1, 0, offs, 0, 1).to(DEV)
    layer = copy.deepcopy(base).to(DEV).eval()
    plain = CommAwareTransformerConv(32, 64, heads=2, hetero=True).to(DEV)
    plain.load_state_dict(layer.state_dict())
    with torch.no_grad():
        assert torch.equal(layer(xd.to(DEV), rel, x_j=xs.to(DEV)),
                           plain(xd.to(DEV), rel, x_j=xs.to(DEV)))
        # training without a given seed: drawn on the device, reproducible under manual_seed
        layer.train()
        torch.manual_seed(3)
        a = layer(xd.to(DEV), rel, x_j=xs.to(DEV))
        b = layer(xd.to(DEV), rel, x_j=xs.to(DEV))
        torch.manual_seed(3)
        assert torch.equal(layer(xd.to(DEV), rel, x_j=xs.to(DEV)), a) and not torch.equal(a, b)
