"""The edge softmax (csrc/kernels/edge_softmax.hip) at every lanes-per-edge width and the
elementwise epilogues of the bf16 path (``bias_relu_pack``, ``relu_mask_bwd``, ``col_sum`` in
csrc/kernels/elementwise.hip) against the fp64 oracles of test_dense_epilogue_cases.py.
Every call runs twice on fresh buffers and the results must be bitwise equal; every test
prints ``error / allowance`` before it asserts.

RECORD (MI355X; printed by ``test_zz_record``, not an input to any bound):
  largest error / allowance: edge_softmax_fwd<LPE> 0.004 / 0.003 / 0.007 / 0.005 / 0.011 /
  0.007 / 0.009 and edge_softmax_bwd<LPE> 0.005 / 0.004 / 0.009 / 0.010 / 0.008 / 0.009 /
  0.007 for LPE = 1, 2, 4, 8, 16, 32, 64; bias_relu_pack<bf16> 0.996 (half an ulp just above
  a power of two), bias_relu_pack<f32> bitwise, every mask word equal; col_sum<f32, 4> 0.017,
  col_sum<f32, 1> 0.012, col_sum<bf16, 8> 0.004, col_sum<bf16, 1> 0.001; no two runs differed.
"""
from __future__ import annotations

import pytest
import torch

import test_dense_epilogue_cases as C
from dgraph_amd.ops import kernels as K
from test_gat_kernels import bound

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST: dict = {}
DTYPES = [torch.float32, torch.bfloat16]


def _ops():
    from dgraph_amd import _native

    return _native.ops()


def note(kernel: str, ratio: float, what: str = "") -> None:
    WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)
    print(f"{kernel} {what}: error / allowance {ratio:.3f}")


def same_bits(a, b) -> bool:
    it = {4: torch.int32, 2: torch.int16, 8: torch.int64}[a.element_size()]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


# ------------------------------------------------------------------------------ edge softmax
def _softmax_case(rowptr, E, H, kind, neg_inf, label):
    ops = _ops()
    s, gr = C.softmax_inputs(rowptr, E, H, kind, neg_inf)
    a64, a32 = C.softmax_contract(rowptr, s), C.softmax_contract(rowptr, s, dtype=torch.float32)
    body = ~torch.isnan(a64)
    rp, sd, gd = rowptr.to(DEV), s.to(DEV), gr.to(DEV)
    outs = []
    for _ in range(2):
        a = torch.full((E, H), C.SENT, device=DEV)
        ops.edge_softmax_fwd(rp, sd, a)
        outs.append(a)
    torch.cuda.synchronize()
    assert same_bits(*outs), f"{label}: two forward runs differ"
    a = outs[0].cpu()
    assert bool((a[~body] == C.SENT).all()), f"{label}: wrote an entry of no row"
    assert bool(torch.isfinite(a).all()), f"{label}: not finite"
    lim = bound(a64[body], a32[body])
    note(f"edge_softmax_fwd<{C.lpe_for(H)}>", float((a.double() - a64)[body].abs().max()) / lim,
         label)
    assert float((a.double() - a64)[body].abs().max()) <= lim, label
    if neg_inf:
        assert bool((a[torch.isinf(s) & body] == 0).all()), f"{label}: -inf score, weight not 0"
    # the adjoint on the fp32 weights of the oracle
    al = torch.where(body, a64, torch.full_like(a64, C.SENT)).float()
    d64 = C.softmax_contract(rowptr, None, gr, al)
    d32 = C.softmax_contract(rowptr, None, gr, al, dtype=torch.float32)
    outs = []
    for _ in range(2):
        ds = torch.full((E, H), C.SENT, device=DEV)
        ops.edge_softmax_bwd(rp, al.to(DEV), gd, ds)
        outs.append(ds)
    torch.cuda.synchronize()
    assert same_bits(*outs), f"{label}: two backward runs differ"
    ds = outs[0].cpu()
    assert bool((ds[~body] == C.SENT).all()), f"{label}: wrote an entry of no row"
    lim = bound(d64[body], d32[body])
    note(f"edge_softmax_bwd<{C.lpe_for(H)}>", float((ds.double() - d64)[body].abs().max()) / lim,
         label)
    assert float((ds.double() - d64)[body].abs().max()) <= lim, label


@pytest.mark.parametrize("H", C.HEADS)
def test_edge_softmax(H):
    rowptr, E = C.softmax_pattern(H)
    for kind in C.SCORES:
        for neg_inf in (False, True):
            _softmax_case(rowptr, E, H, kind, neg_inf, f"H={H} {kind} -inf={neg_inf}")


@pytest.mark.parametrize("H", C.MANY_HEADS)
def test_edge_softmax_many_rows(H):
    rowptr, E = C.many_pattern()
    _softmax_case(rowptr, E, H, "small", False, f"H={H} many rows")


def test_edge_softmax_contract_checks():
    ops = _ops()
    rowptr, E = C.softmax_pattern(4)
    rp = rowptr.to(DEV)
    s = torch.zeros(E, 4, device=DEV)

    def refuses(fn, *args):
        written = [t for t in args if t.dtype == torch.float32 and float(t.flatten()[0]) == C.SENT]
        with pytest.raises(RuntimeError):
            fn(*args)
        torch.cuda.synchronize()
        assert all(bool((t == C.SENT).all()) for t in written)

    sent = lambda *shape: torch.full(shape, C.SENT, device=DEV)  # noqa: E731
    refuses(ops.edge_softmax_fwd, rp, s, sent(E - 1, 4))
    refuses(ops.edge_softmax_fwd, rp, s, sent(E, 3))
    refuses(ops.edge_softmax_fwd, rp, s, sent(E * 4))
    refuses(ops.edge_softmax_fwd, rp, torch.zeros(E, 65, device=DEV), sent(E, 65))
    refuses(ops.edge_softmax_fwd, rp.int(), s, sent(E, 4))
    refuses(ops.edge_softmax_fwd, rp[:0], s, sent(E, 4))
    refuses(ops.edge_softmax_bwd, rp, s, torch.zeros(E - 1, 4, device=DEV), sent(E, 4))
    refuses(ops.edge_softmax_bwd, rp, s, s, sent(E + 1, 4))
    refuses(ops.edge_softmax_bwd, rp, s, s, sent(E, 5))
    refuses(ops.edge_softmax_bwd, rp, torch.zeros(E, 65, device=DEV),
            torch.zeros(E, 65, device=DEV), sent(E, 65))
    refuses(ops.edge_softmax_bwd, rp.int(), s, s, sent(E, 4))
    refuses(ops.edge_softmax_bwd, rp[:0], s, s, sent(E, 4))
    # one element of rowptr: no rows, nothing written
    a = sent(E, 4)
    ops.edge_softmax_fwd(rp[:1], s, a)
    torch.cuda.synchronize()
    assert bool((a == C.SENT).all())


# ------------------------------------------------------------------------------ mask epilogues
def _pack_case(shape, dtype, with_bias, on_device=False):
    dev = DEV if on_device else "cpu"
    y0, bias = C.pack_inputs(shape, dtype, with_bias, dev)
    y0, bias = y0.to(DEV), None if bias is None else bias.to(DEV)
    n = y0.numel()
    nwords = K.mask_words(n)
    label = f"{tuple(shape)} {dtype} bias={with_bias}"
    for relu in (True, False):
        t, keep, want = C.pack_oracle(y0, bias, relu)
        assert float(t.abs().min()) >= 0.1
        runs = []
        for _ in range(2):
            y = y0.clone()
            bits = torch.full((nwords + 16,), C.WORD_FILL, dtype=torch.int32, device=DEV)
            K.bias_relu_pack(y, bias, bits, relu=relu)
            runs.append((y, bits))
        torch.cuda.synchronize()
        assert same_bits(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), label
        y, bits = runs[0]
        if dtype == torch.float32:
            t32 = y0 if bias is None else y0 + bias
            want32 = torch.where(t32 > 0, t32, torch.zeros_like(t32)) if relu else t32
            bad = int((y != want32).sum())
            print(f"bias_relu_pack<f32> {label} relu={relu}: {bad} outputs differ")
            assert same_bits(y, want32), label
            assert bool(((y.double() - want).abs() <= 2.0 ** -24 * want.abs()).all())
        else:
            lim = 2.0 ** -8 * want.abs()
            err = (y.double() - want).abs()
            ratio = float((err / lim.clamp_min(1e-300)).max())
            note("bias_relu_pack<bf16>", ratio, f"{label} relu={relu}")
            assert bool((err <= lim).all()), label
        assert bool((bits[nwords:] == C.WORD_FILL).all()), f"{label}: wrote past the mask"
        if relu:
            ww = C.pack_words(keep)
            badw = int((bits[:nwords] != ww).sum())
            print(f"bias_relu_pack {label}: {badw} of {nwords} mask words differ")
            assert badw == 0, label
            # and back: g = keep ? g : 0 from the words just written
            g0 = y0
            outs = []
            for _ in range(2):
                g = g0.clone()
                K.relu_mask_bwd(g, bits[:nwords])
                outs.append(g)
            torch.cuda.synchronize()
            assert same_bits(*outs), label
            assert same_bits(outs[0], torch.where(keep, g0, torch.zeros_like(g0))), label
        else:
            assert bool((bits == C.WORD_FILL).all()), f"{label}: relu=False wrote the mask"


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", C.PACK_SHAPES, ids=str)
def test_bias_relu_pack(shape, dtype):
    for with_bias in (False, True):
        _pack_case(shape, dtype, with_bias)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_bias_relu_pack_grid_stride(dtype):
    """More than 2048 blocks x 16 chunks: every wave takes a second group of chunks."""
    _pack_case(C.PACK_BIG, dtype, True, on_device=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_bias_relu_pack_lds_limit(dtype):
    y = torch.full((8, 16392), C.SENT, dtype=dtype, device=DEV)
    with pytest.raises(RuntimeError):
        K.bias_relu_pack(y, torch.zeros(16392, device=DEV), None, relu=True)
    torch.cuda.synchronize()
    assert bool((y == C.SENT).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_relu_mask_bwd_constant_masks(dtype):
    """All-ones words (also past ``numel``, in a last chunk that ends early): nothing
    changes, not a bit; all-zeros words: everything is 0."""
    for shape in C.PACK_SHAPES + [(777 * 3, 40)]:
        y0, _ = C.pack_inputs(shape, dtype, False)
        g0 = y0.to(DEV)
        g0.view(-1)[::7] = -0.0
        n = g0.numel()
        ones = torch.full((K.mask_words(n),), -1, dtype=torch.int32, device=DEV)
        for _ in range(2):
            g = g0.clone()
            K.relu_mask_bwd(g, ones)
            torch.cuda.synchronize()
            assert same_bits(g, g0), (shape, dtype)
            g = g0.clone()
            K.relu_mask_bwd(g, torch.zeros_like(ones))
            torch.cuda.synchronize()
            assert same_bits(g, torch.zeros_like(g0)), (shape, dtype)
    assert any((s[0] * s[1]) % 512 for s in C.PACK_SHAPES[:5])


# ------------------------------------------------------------------------------ col_sum
def _col_sum_case(g, L, F, dtype, label, aligned=True):
    vec, nb, rpb, rpi, D = C.col_sum_plan(L, F, g.stride(0), dtype, aligned)
    assert (g.data_ptr() % 16 == 0) == aligned
    ref = g.double().sum(0)
    lim = D * 2.0 ** -24 * g.double().abs().sum(0)
    a, b = K.col_sum(g), K.col_sum(g)
    torch.cuda.synchronize()
    assert a.dtype == torch.float32 and a.shape == (F,)
    assert same_bits(a, b), f"{label}: two runs differ"
    err = (a.double() - ref).abs()
    note(f"col_sum<{'f32' if dtype == torch.float32 else 'bf16'}, {vec}>",
         float((err / lim.clamp_min(1e-300)).max()), label)
    assert bool((err <= lim).all()), label


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("L", C.COLSUM_L)
def test_col_sum(L, dtype):
    gen = torch.Generator(device=DEV).manual_seed(L)
    for F in C.COLSUM_F[dtype]:
        g = torch.randn(L, F, generator=gen, device=DEV).to(dtype)
        _col_sum_case(g, L, F, dtype, f"L={L} F={F}")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_col_sum_slices(dtype):
    """A row-strided slice, and column slices that start at a column that is no multiple of
    the vector width (a base that is not 16-byte aligned: scalar lanes)."""
    gen = torch.Generator(device=DEV).manual_seed(9)
    vec = 4 if dtype == torch.float32 else 8
    for L in (257, 1000):
        buf = torch.randn(L, 192, generator=gen, device=DEV).to(dtype)
        buf[:, 64:] = float("nan")
        _col_sum_case(buf[:, :64], L, 64, dtype, f"L={L} row-strided")
        buf = torch.randn(L, 4 * vec, generator=gen, device=DEV).to(dtype)
        off = vec // 2
        _col_sum_case(buf[:, off:off + vec], L, vec, dtype, f"L={L} misaligned", aligned=False)
        buf = torch.randn(L, 24 * vec, generator=gen, device=DEV).to(dtype)
        _col_sum_case(buf[:, off:off + 16 * vec], L, 16 * vec, dtype, f"L={L} misaligned wide",
                      aligned=False)


def test_zz_record():
    """Prints what the module docstring records."""
    print("largest error / allowance:", {k: round(v, 3) for k, v in sorted(WORST.items())})
