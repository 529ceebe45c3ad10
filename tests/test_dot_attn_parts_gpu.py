"""The carry-in forward ``dot_attn_fwd_carry_f32`` (csrc/kernels/dot_attn_f32.hip, called
through ``_native.ops()`` directly), ``dot_attention_parts``, ``dot_attention_halo`` over the
loopback all-to-all-v and ``CommAwareTransformerConv(overlap=True)`` over RCCL, on the GPU
against the fp64 single-pass oracle of tests/test_dot_attn.py.

Pattern, inputs, the four edge partitions P1-P4 and how a chained forward is run (plain
forward, NaN wherever ``stat_l == 0``, one carry pass per further part): see
tests/test_dot_attn_parts.py. The backward kernels get ``c`` from the fp64 oracle, rounded to
fp32, and the chained forward's own ``stat_m`` / ``stat_l``.

Bound per compared array: ``max(2e-5, 8 err32) max(1, max|fp64|)`` with ``err32`` the error of
the same formula evaluated in fp32 on the CPU (``test_gat_kernels.bound``) — nothing is taken
from the kernels' own output. Largest ``error / bound`` seen on an MI355X (a record, not an
input to the bound; the tests print every figure before asserting):

    carry forward (P1-P4)        out 0.108   stat_m 0.007   stat_l 0.207
    backward on its statistics   dq 0.228    dk 0.264       dv 0.236
    wide operands                out 0.020   stat_m 0.005   stat_l 0.003
    two sources per pass         out 0.108   stat_m 0.005   stat_l 0.207
    dot_attention_parts          out 0.020   dq 0.040   dk 0.053   dv 0.060
    dot_attention_halo           out 0.024   dq 0.034   dkv 0.074
    the layer over RCCL, W = 2   out 0.004   dx 0.006   dx_j 0.009   parameters 0.011 or less
"""
from __future__ import annotations

import types

import pytest
import torch

from conftest import rank_device, run_ranks
from test_dot_attn import (ND, NS, SCALES, _dense_transformer, _edges, case, dot_attn_contract,
                           oracle)
from test_dot_attn_parts import PARTITIONS, chain, check_chain_vs_single_pass, \
    check_idle_rows_untouched, partition, run_parts
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
        print(f"\n[dot-attn-parts] largest error / bound, {k}: {RATIOS[k]:.3f}", end="")
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
    key = f"{tag.split()[0]}:{name}"
    RATIOS[key] = max(RATIOS.get(key, 0.0), err / bd)
    print(f"{tag} {name}: err {err:.3e} bound {bd:.3e} ratio {err / bd:.3f}")
    assert err <= bd, (tag, name, err, bd)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


class _Wide:
    """Operands as column slices of wider buffers: ``k`` / ``v`` the halves of one
    ``[rows, 2C]`` block inside a NaN-filled ``[rows, 2C + 8]`` buffer, ``q`` the upper half
    of a NaN-filled ``[R, 2C]`` one; ``out`` the upper half of a ``[R, 2C]`` buffer and
    ``stat_m`` / ``stat_l`` the upper halves of ``[R, 2 heads]`` ones (one head: column 2
    of ``[R, 4]``), all holding ``SENT`` outside."""

    def __init__(self):
        self.held = []

    def kv(self, k, v):
        C = k.shape[1]
        buf = torch.full((k.shape[0], 2 * C + 8), float("nan"), device=DEV)
        buf[:, 4:4 + C] = k.to(DEV)
        buf[:, 4 + C:4 + 2 * C] = v.to(DEV)
        return buf[:, 4:4 + C], buf[:, 4 + C:4 + 2 * C]

    def q(self, q):
        C = q.shape[1]
        buf = torch.full((q.shape[0], 2 * C), float("nan"), device=DEV)
        buf[:, C:] = q.to(DEV)
        return buf[:, C:]

    def out(self, rows, cols):
        if cols == 1:
            buf, sl = torch.full((rows, 4), SENT, device=DEV), slice(2, 3)
        else:
            buf, sl = torch.full((rows, 2 * cols), SENT, device=DEV), slice(cols, 2 * cols)
        buf[:, sl] = float("nan")
        self.held.append((buf, sl))
        return buf[:, sl]

    def assert_outside_untouched(self):
        for buf, sl in self.held:
            keep = torch.ones(buf.shape[1], dtype=torch.bool, device=DEV)
            keep[sl] = False
            rest = buf[:, keep]
            assert torch.equal(rest, torch.full_like(rest, SENT))


def _run_chain(name, C, heads, s, idx, wide=None, two=False):
    """The chained forward of partition ``name`` on the device, on fresh NaN-filled state
    buffers: ``((out, stat_m, stat_l), [state before each carry pass])``. ``two``: every pass
    reads its sources as two, split at ``LS`` (parts over all ``N`` columns only)."""
    ops = _ops()
    d = case(C, heads, s)
    q = wide.q(d["q"]) if wide else d["q"].to(DEV)
    sc = d["scale"]

    def operands(rp, cl, k, v):
        kd, vd = wide.kv(k, v) if wide else (k.to(DEV).contiguous(), v.to(DEV).contiguous())
        src = (kd, vd, None, None, kd.shape[0])
        if two:
            assert k.shape[0] == N
            src = (kd[:LS], vd[:LS], kd[LS:], vd[LS:], LS)
        return rp.to(DEV), cl.to(idx).to(DEV), src

    def first(rp, cl, k, v):
        rp, cl, src = operands(rp, cl, k, v)
        if wide:
            out, m, l = wide.out(R, C), wide.out(R, heads), wide.out(R, heads)
        else:
            out, m, l = (torch.full((R, n), float("nan"), device=DEV) for n in (C, heads, heads))
        ops.dot_attn_fwd_f32(rp, cl, q, *src, out, 0.0, m, l, heads, sc)
        return out, m, l

    def carry(rp, cl, k, v, out, m, l):
        rp, cl, src = operands(rp, cl, k, v)
        ops.dot_attn_fwd_carry_f32(rp, cl, q, *src, out, m, l, heads, sc)
        return out, m, l

    state, before = chain(name, first, carry, C, heads, s)
    torch.cuda.synchronize()
    return state, before


def _check_chain(tag, name, state, before, C, heads, s):
    r64, r32, _ = oracle(C, heads, s, 0.0)
    check_chain_vs_single_pass(
        state, lambda n, got, rows: _compare(tag, n, got, r64[n][rows], r32[n][rows]))
    check_idle_rows_untouched(name, before, state)


def _backward_from(state, C, heads, s, idx):
    """dq / dk / dv of the existing backward kernels over the merged pattern, fed the chained
    forward's statistics."""
    ops = _ops()
    rowptr, col, _ = pattern()
    t_rowptr, t_col = transpose(rowptr, col, N)
    d = case(C, heads, s)
    c = oracle(C, heads, s, 0.0)[0]["c"].float().to(DEV)
    _, m, l = state
    m, l = m.contiguous(), l.contiguous()
    q, k, v, g = (d[n].to(DEV) for n in ("q", "k", "v", "g"))
    dq = torch.full((R, C), float("nan"), device=DEV)
    dk, dv = torch.full((N, C), float("nan"), device=DEV), torch.full((N, C), float("nan"),
                                                                      device=DEV)
    ops.dot_attn_bwd_dst_f32(rowptr.to(DEV), col.to(idx).to(DEV), q, k, v, None, None, N, m, l,
                             g, c, dq, heads, d["scale"])
    ops.dot_attn_bwd_src_f32(t_rowptr.to(DEV), t_col.to(idx).to(DEV), q, g, k, v, m, l, c, dk,
                             dv, heads, d["scale"])
    torch.cuda.synchronize()
    return {"dq": dq, "dk": dk, "dv": dv}


@pytest.mark.parametrize("idx", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("C,heads", PAIRS)
def test_carry_kernel_vs_fp64(C, heads, s, idx):
    """P1-P4 at one instantiation: the final state against the single-pass oracle, two runs
    bitwise equal, idle rows untouched, no NaN of an unset state in a result, and the
    backward kernels on the chained statistics."""
    r64, r32, _ = oracle(C, heads, s, 0.0)
    for name in PARTITIONS:
        state, before = _run_chain(name, C, heads, s, idx)
        again, _ = _run_chain(name, C, heads, s, idx)
        for a, b in zip(state, again):
            assert torch.equal(_bits(a), _bits(b)), name
        tag = f"carry {name} C={C} heads={heads} s={s}"
        _check_chain(tag, name, state, before, C, heads, s)
        got = _backward_from(state, C, heads, s, idx)
        for n in got:
            _compare(f"carry-bwd {name} C={C} heads={heads} s={s}", n, got[n], r64[n], r32[n])


@pytest.mark.parametrize("name", ["P1", "P3"])
@pytest.mark.parametrize("C,heads", [(64, 1), (128, 4), (256, 2), (256, 8)])
def test_carry_kernel_wide_operands(C, heads, name):
    """Every part's k / v the halves of one [rows, 2C] block with NaN around it, q and the
    state inside wider buffers: nothing outside the slices is read into a result or
    written."""
    wide = _Wide()
    state, before = _run_chain(name, C, heads, 0.5, torch.int32, wide)
    assert state[0].stride(0) == 2 * C and state[1].stride(0) == state[2].stride(0)
    _check_chain(f"carry-wide {name} C={C} heads={heads}", name, state, before, C, heads, 0.5)
    wide.assert_outside_untouched()
    plain, _ = _run_chain(name, C, heads, 0.5, torch.int32)
    for a, b in zip(state, plain):
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("name", ["P2", "P3", "P4"])
@pytest.mark.parametrize("C,heads", [(64, 2), (128, 1), (256, 8)])
def test_carry_kernel_two_sources(C, heads, name):
    """Every pass, the carry passes included, with its columns over two sources split at 41:
    bitwise the one-source result (the same rows in the same order)."""
    state, before = _run_chain(name, C, heads, 40.0, torch.int32, two=True)
    _check_chain(f"carry-two {name} C={C} heads={heads}", name, state, before, C, heads, 40.0)
    plain, _ = _run_chain(name, C, heads, 40.0, torch.int32)
    for a, b in zip(state, plain):
        assert torch.equal(_bits(a), _bits(b))


def test_carry_kernel_empty_shapes():
    ops = _ops()
    C, Hh, sc = 64, 2, 0.25
    f = lambda *shape: torch.randn(*shape, device=DEV)  # noqa: E731
    e = lambda n: torch.empty(0, n, device=DEV)  # noqa: E731
    i32 = torch.empty(0, dtype=torch.int32, device=DEV)
    q, k, v = f(R, C), f(5, C), f(5, C)
    state = [f(R, C), f(R, Hh), f(R, Hh).abs()]
    state[0][3], state[1][3], state[2][3] = float("nan"), float("nan"), 0.0
    keep = [t.clone() for t in state]
    rp0 = torch.zeros(1, dtype=torch.long, device=DEV)
    rp = torch.zeros(R + 1, dtype=torch.long, device=DEV)
    # no destination rows (also with every operand empty); no source rows; rows and sources
    # but no entries (the one launch): the carried state is the result
    ops.dot_attn_fwd_carry_f32(rp0, i32, q, k, v, None, None, 5, *state, Hh, sc)
    ops.dot_attn_fwd_carry_f32(rp0, i32, e(C), e(C), e(C), None, None, 0, e(C), e(Hh), e(Hh),
                               Hh, sc)
    ops.dot_attn_fwd_carry_f32(rp, i32, q, e(C), e(C), None, None, 0, *state, Hh, sc)
    ops.dot_attn_fwd_carry_f32(rp, i32, q, k, v, e(C), e(C), 5, *state, Hh, sc)
    ops.dot_attn_fwd_carry_f32(rp, i32, q, k, v, None, None, 5, *state, Hh, sc)
    torch.cuda.synchronize()
    for a, b in zip(state, keep):
        assert torch.equal(_bits(a), _bits(b))
    with pytest.raises(RuntimeError):  # entries, but nothing to gather from
        ops.dot_attn_fwd_carry_f32(pattern()[0].to(DEV), pattern()[1].to(torch.int32).to(DEV),
                                   q, e(C), e(C), None, None, 0, *state, Hh, sc)


# ---------------------------------------------------- contract checks (bindings_dot_attn.cpp)
_CARRY = ("rowptr", "col", "q", "k", "v", "k2", "v2", "nsplit", "out", "stat_m", "stat_l",
          "heads", "scale")


def _valid_args(C, heads):
    rowptr, col, _ = pattern()
    f = lambda *shape: torch.randn(*shape, device=DEV)  # noqa: E731
    return dict(rowptr=rowptr.to(DEV), col=col.to(torch.int32).to(DEV), q=f(R, C), k=f(N, C),
                v=f(N, C), k2=None, v2=None, nsplit=N, out=f(R, C), stat_m=f(R, heads),
                stat_l=f(R, heads).abs(), heads=heads, scale=0.125)


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
    elif what == "v with column stride 2":
        A["v"] = torch.randn(N, 128, device=DEV)[:, ::2]
    elif what == "out with a row stride that is no multiple of 4":
        A["out"] = torch.randn(R, 66, device=DEV)[:, :64]
    elif what == "stat_l row stride differs from stat_m's":
        A["stat_l"] = torch.randn(R, 4, device=DEV).abs()[:, :2]
    elif what == "stat_m with column stride 2":
        A["stat_m"] = torch.randn(R, 4, device=DEV)[:, ::2]
    elif what == "k2 without v2":
        A.update(k2=A["k"][LS:].clone(), nsplit=LS)
    elif what == "float64 q":
        A["q"] = A["q"].double()
    elif what == "too few state rows":
        A["stat_l"] = A["stat_l"][:R - 1]
    else:
        raise KeyError(what)
    return A


@pytest.mark.parametrize("what", ["C=96", "heads=3", "(C,heads)=(64,16)", "k offset by one float",
                                  "v with column stride 2",
                                  "out with a row stride that is no multiple of 4",
                                  "stat_l row stride differs from stat_m's",
                                  "stat_m with column stride 2", "k2 without v2", "float64 q",
                                  "too few state rows"])
def test_carry_contract_checks_raise_before_launch(what):
    A = _violate(what)
    before = {k: A[k].clone() for k in ("out", "stat_m", "stat_l")}
    with pytest.raises(RuntimeError):
        _ops().dot_attn_fwd_carry_f32(*[A[k] for k in _CARRY])
    torch.cuda.synchronize()
    for k, t in before.items():
        assert torch.equal(A[k], t), k


# ---------------------------------------------------------------------- dot_attention_parts
@pytest.mark.parametrize("name", ["P1", "P3"])
@pytest.mark.parametrize("C,heads", [(64, 1), (128, 4), (256, 2), (256, 8)])
def test_dot_attention_parts_gpu_vs_cpu(C, heads, name):
    ref64 = run_parts(name, "cpu", torch.float64, C, heads, 0.5)
    r32 = oracle(C, heads, 0.5, 0.0)[1]
    got = run_parts(name, DEV, torch.float32, C, heads, 0.5)
    got2 = run_parts(name, DEV, torch.float32, C, heads, 0.5)
    for k in got:
        assert ref64[k].dtype == torch.float64
        assert torch.equal(got[k], got2[k]), k
        _compare(f"parts {name} C={C} heads={heads}", k, got[k], ref64[k], r32[k])


def test_dot_attention_parts_single_part_is_dot_attention():
    from dgraph_amd.ops import dot_attention, dot_attention_parts
    from dgraph_amd.ops.gat import GatPattern

    rowptr, col, _ = pattern()
    d = case(128, 4, 0.5)
    pat = GatPattern(rowptr.to(DEV), col.to(DEV), N, 0)
    res = []
    for fn in (lambda q, k, v: dot_attention_parts([(q, k, v, pat)], heads=4),
               lambda q, k, v: dot_attention(q, k, v, pat, heads=4)):
        q, k, v = (d[n].to(DEV).requires_grad_() for n in ("q", "k", "v"))
        out = fn(q, k, v)
        res.append([out.detach()] + list(torch.autograd.grad(out, (q, k, v), d["g"].to(DEV))))
    for a, b in zip(*res):
        assert torch.equal(_bits(a), _bits(b))


def test_dot_attention_parts_rejects_unsupported_gpu_inputs():
    from dgraph_amd.ops import dot_attention_parts
    from dgraph_amd.ops.gat import GatPattern

    rowptr, col, _ = pattern()
    pat = GatPattern(rowptr.to(DEV), col.to(DEV), N, 0)
    f = lambda n, C, dt=torch.float32: torch.randn(n, C, device=DEV, dtype=dt)  # noqa: E731
    for C, heads, dt in ((96, 2, torch.float32), (64, 16, torch.float32),
                         (64, 2, torch.float64), (64, 2, torch.bfloat16)):
        with pytest.raises(ValueError, match="64, 128, 256"):
            dot_attention_parts([(f(R, C, dt), f(N, C, dt), f(N, C, dt), pat)] * 2, heads=heads)


# ----------------------------------------------------------------------- dot_attention_halo
@pytest.mark.parametrize("receives", [True, False], ids=["halo", "sends-only"])
@pytest.mark.parametrize("C,heads", [(64, 2), (256, 4)])
def test_dot_attention_halo_loopback(C, heads, receives):
    """One process over the loopback all-to-all-v: halo row ``h`` is a copy of local row
    ``send_idx[h]`` (some rows are sent twice), so the reference is ``dot_attention`` at fp64
    on the CPU over the pattern with its halo columns remapped to those rows — the returned
    gradients' segment sum included. ``sends-only``: rows go out, none come in."""
    from dgraph_amd.comm.alltoallv import AllToAllV, CommStats
    from dgraph_amd.ops import HaloPlan, dot_attention, dot_attention_halo
    from dgraph_amd.ops.gat import GatPattern

    rowptr, col, _ = pattern()
    d = case(C, heads, 0.5)
    gen = torch.Generator().manual_seed(9)
    if receives:
        send_idx = torch.randint(0, LS, (HS,), generator=gen)
        send_idx[1] = send_idx[0]
        cols, H = col, HS
        local = torch.where(col >= LS, send_idx[(col - LS).clamp(min=0)], col)
    else:
        send_idx = torch.randint(0, LS, (7,), generator=gen)
        cols, H = col % LS, 0
        local = cols
    kv0 = torch.cat([d["k"][:LS], d["v"][:LS]], 1)
    # the reference: everything local
    q64, kv64 = d["q"].double().requires_grad_(), kv0.double().requires_grad_()
    ref = dot_attention(q64, kv64[:, :C], kv64[:, C:], GatPattern(rowptr, local, LS, 0),
                        heads=heads)
    gq, gkv = torch.autograd.grad(ref, (q64, kv64), d["g"].double())
    r32 = dot_attn_contract(rowptr, local, d["q"], d["k"][:LS], d["v"][:LS], None, None, LS,
                            d["g"], heads, d["scale"], 0.0, None, dtype=torch.float32)
    ref64 = {"out": ref.detach(), "dq": gq, "dkv": gkv}
    ref32 = {"out": r32["out"], "dq": r32["dq"], "dkv": torch.cat([r32["dk"], r32["dv"]], 1)}

    pat = GatPattern(rowptr.to(DEV), cols.to(DEV), LS, H)

    def run():
        plan = HaloPlan(AllToAllV([0, send_idx.numel()], [0, H]), send_idx.to(DEV), LS)
        q, kv = d["q"].to(DEV).requires_grad_(), kv0.to(DEV).requires_grad_()
        CommStats.reset()
        out = dot_attention_halo(q, kv, pat, plan, heads=heads)
        assert CommStats.calls == 1, CommStats.calls
        a, b = torch.autograd.grad(out, (q, kv), d["g"].to(DEV))
        assert CommStats.calls == 2, CommStats.calls
        torch.cuda.synchronize()
        return {"out": out.detach(), "dq": a, "dkv": b}

    got, got2 = run(), run()
    for k in got:
        assert torch.equal(_bits(got[k]), _bits(got2[k])), k
        _compare(f"halo-op C={C} heads={heads} receives={receives}", k, got[k], ref64[k],
                 ref32[k])


# ------------------------------------------------------------ the layer over RCCL, W = 2
def _mk_layer(comm, overlap):
    from dgraph_amd.models.transformer_conv import CommAwareTransformerConv

    torch.manual_seed(0)
    layer = CommAwareTransformerConv(32, 64, comm=comm, heads=2, hetero=True, overlap=overlap)
    with torch.no_grad():
        layer.bias.normal_()
    return layer


def _overlap_rccl_body(rank, world):
    import torch.distributed as dist

    from dgraph_amd import Communicator
    from dgraph_amd.comm.alltoallv import CommStats
    from dgraph_amd.data.hetero import build_relation_graph, get_vertex_offsets

    assert dist.get_backend() == "nccl"
    dev = rank_device()
    comm = Communicator.init_process_group("nccl")
    try:
        edges = _edges(world)  # skewed: the last rank sends rows and receives none
        offs = {0: get_vertex_offsets(ND, world), 1: get_vertex_offsets(NS, world)}
        rel = build_relation_graph(edges, 1, 0, offs, rank, world)
        if rank == world - 1:
            assert rel.num_halo == 0 and sum(rel.pattern.send_splits()) > 0
        else:
            assert rel.num_halo > 0
        rel = rel.to(dev)
        gen = torch.Generator().manual_seed(1)
        xd, xs, w = (torch.randn(n, c, generator=gen) for n, c in ((ND, 32), (NS, 32), (ND, 64)))
        d0, d1 = int(offs[0][rank]), int(offs[0][rank + 1])
        s0, s1 = int(offs[1][rank]), int(offs[1][rank + 1])
        layer = _mk_layer(comm, True).to(dev)
        xdl = xd[d0:d1].to(dev).requires_grad_()
        xsl = xs[s0:s1].to(dev).requires_grad_()
        CommStats.reset()
        out = layer(xdl, rel, x_j=xsl)
        assert CommStats.calls == 1, CommStats.calls
        (out * w[d0:d1].to(dev)).sum().backward()
        assert CommStats.calls == 2, CommStats.calls
        pg = [p.grad.clone() for p in layer.parameters()]
        for t in pg:
            dist.all_reduce(t)
        torch.cuda.synchronize()
        # W = 1 on the CPU: the layer at fp64 (the oracle), its dense formulation at fp32
        one = types.SimpleNamespace(get_world_size=lambda: 1)
        offs1 = {0: get_vertex_offsets(ND, 1), 1: get_vertex_offsets(NS, 1)}
        rel1 = build_relation_graph(edges, 1, 0, offs1, 0, 1)

        def cpu(dtype, dense):
            m = _mk_layer(one, False).to(dtype)
            a, b = xd.to(dtype).requires_grad_(), xs.to(dtype).requires_grad_()
            o = _dense_transformer(m, a, b, edges) if dense else m(a, rel1, x_j=b)
            gr = torch.autograd.grad(o, [a, b] + list(m.parameters()), w.to(dtype))
            return [o.detach()[d0:d1], gr[0][d0:d1], gr[1][s0:s1]] + list(gr[2:])

        ref64, ref32 = cpu(torch.float64, False), cpu(torch.float32, True)
        names = ["out", "dx", "dx_j"] + [n for n, _ in layer.named_parameters()]
        for n, a, b, c in zip(names, [out, xdl.grad, xsl.grad] + pg, ref64, ref32):
            _compare(f"rccl-layer rank{rank}", n, a, b, c)
        for k in sorted(RATIOS):
            print(f"[dot-attn-parts] rank {rank} largest error / bound, {k}: {RATIOS[k]:.3f}")
    finally:
        comm.destroy()


def test_layer_overlap_two_ranks_rccl():
    """``overlap=True`` at W = 2 over real RCCL on the one GPU, on the skewed graph (rank 1
    receives no halo rows and still takes part in both exchanges), against the W = 1 layer at
    fp64 on the CPU."""
    run_ranks(_overlap_rccl_body, 2, timeout=240, backend="rccl-one-gpu")
