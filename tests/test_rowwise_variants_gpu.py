"""Every instantiation of the dense row-wise kernels on the GPU -- LayerNorm
(csrc/kernels/layernorm.hip), BatchNorm (batchnorm.hip), ``bias_act`` (act.hip),
``pair_relu`` / ``gather_add_act`` (edge_fused.hip), ``copy_rows`` / ``masked_gather_rows``
(rows.hip) -- called directly through ``_native.ops()`` and compared with the fp64 contracts
of tests/test_rowwise_cases.py, which also holds the inputs and the tables of widths and
pins them down on the CPU.

(a) LayerNorm: every width of ``LN_F`` x {fp32, bf16} x {affine, none} x {residual, none}
    at N = 203, 1031 and 1: y, mean, rstd, and the backward on the kernel's own mean / rstd;
    ``1000 + 0.1 randn`` rows and a constant row; 36,867 rows; repeatable dgamma / dbeta.
(b) LayerNorm width limits: the widest width of each path forward and backward (the bf16
    backward at F = 4096 takes 128 KB of dynamic LDS), one width past each raises.
(c) BatchNorm: the four modes at every (type, VEC, LPR) of ``BN_F``, with all of gamma /
    beta / c1 / c2 and with none, with and without ReLU, contiguous / row-strided /
    unaligned (VEC = 1) operands, N = 203 and 3, 17,415 rows, N = 0, big-mean statistics,
    exact-zero gates, repeatable reductions. LEFT OUT: a row-strided or unaligned ``out``
    (and ``dx``). ``bn_apply`` allocates its output itself, contiguous, so ``ldo != F`` and an
    unaligned ``out`` cannot be reached through the op; only x and dy are strided here.
(d) BatchNorm dropout: p = 0.1 and 0.5; forward, backward reduce and backward apply share
    ``dropout_keep_mask``; a strided x gives the same mask; the constructed seeds whose
    element hashes between the fp64 and the fp32 threshold.
(e) ``bias_act``: acts 0, 1, 2 x ``ACT_F`` (vector widths up to 1024 fp32 / 2048 bf16),
    contiguous / strided / unaligned, with and without b, N = 203 and 1, 2,125 rows; db
    against the sum of the STORED dz; exact-zero gates; the width limits raise.
(f) ``pair_relu``: three modes x int32 / int64 x ``EDGE_F`` on the degree ladder (mode 2 on
    its transpose), strided operands, an ``out`` taller than the pattern, exact-zero gates,
    69,635 rows, bf16 counts above 256.
(g) ``gather_add_act``: forward and backward x four activations x ``EDGE_F``, every null
    combination of Y / P / Q, strided and unaligned operands, E = 203 and 69,635,
    exact-zero gates for relu and leaky-relu, SiLU at +-90.
(h) ``copy_rows`` (``COPY_F``: VEC 4 / 8, 2 and 1, int32 / int64, src / dst / both / neither,
    negative sources and destinations, strided, n = 1, 203 and 135,171, accumulate) and
    ``masked_gather_rows``.

Accuracy rule, the project's: ``|kernel - fp64| <= test_gat_kernels.bound(ref64, ref32)``
with ``ref32`` the same contract in fp32 on the CPU; a bf16 OUTPUT adds ``2^-8 |v|`` per
rounding (tests/test_spmm_generic_cases.py): y, dx, dz, out: one rounding; mean, rstd,
dgamma, dbeta, db and the BatchNorm reductions are fp32 / fp64 outputs: none. ``copy_rows``
without accumulate, ``masked_gather_rows`` and every exact-zero case on integers must EQUAL
the contract; the dropout keep pattern must equal ``dropout_keep_mask``. Outputs the caller
passes are sentinel-filled and, where the op takes strided operands, wider and taller than
the slice written: outside it the sentinel must survive bitwise, inside none may. (The
LayerNorm and BatchNorm ops allocate their outputs themselves.) Random ReLU cases keep
their pre-activations 1e-3 away from 0 where fp32 rounding could decide the gate.

Largest ``error / bound`` seen on an MI355X (a record, not an input to any bound; every
figure is printed before it is asserted). The bf16 outputs y / dx / dz / out reach 0.95 to
0.99 in every family: that is their one rounding, half a bf16 ulp being up to 2^-8 |v|; the
figures below are the fp32 runs and the fp32 outputs of the bf16 runs.

    LayerNorm      y 0.108   mean 0.008   rstd 0.004   dx 0.013   dgamma 0.013   dbeta 0.009
                   bf16: mean 0.007   rstd 0.005   dgamma 0.014   dbeta 0.006
      big mean     y 0.125   rstd 0.125   dx 0.013   dgamma 0.011
      constant row of 3     y 0.125   mean 0.004   rstd 0.002   dx 0.005
      constant row of 1000  y 0.125   mean 0.003   rstd 0.125   dx 0.005
                   (0.125: the kernel errs exactly like the fp32 contract, one rounding of
                   sum * (1 / F), and the bound is 8 times that)
      many rows    y 0.006   dx 0.007   dgamma 0.010      widest  y 0.006   dgamma 0.013
    BatchNorm      stats 0.005   y 0.005   reduce 0.005   dx 0.007    bf16: stats 0.013
      big mean     stats 0.000   y 0.004   reduce 0.002   dx 0.004
      dropout      y 0.006   reduce 0.004   dx 0.007      many rows  y 0.003   dx 0.005
    bias_act       y 0.006   dz 0.030   db 0.028          many rows  dz 0.026   db 0.011
    pair_relu      mode 0 0.060   mode 1 0.002   mode 2 0.039   many rows 0.004
    gather_add_act fwd 0.006   bwd 0.037   many edges bwd 0.030   SiLU at +-90 0.000
    copy_rows      accumulate 0.008

The whole file (335 cases) takes 8 s there; no case takes more than 0.5 s. The bf16
LayerNorm backward at F = 4096 launches with its 128 KB of dynamic LDS as it is, so
``ln_shape_ok`` stays.

What the file found: (1) the LayerNorm forward subtracted an UNROUNDED ``sum * (1 / F)``
(the compiler fused the product into ``v - mu``) while storing the rounded mean for the
backward: a row of 1000s came out with d = -3e-5 instead of 0 and y off by 0.03 (error /
bound 2.7 at bf16 F = 3 of the big-mean case, 5 to 160 on the row of 1000s at the scalar
widths from 29 up); fixed in layernorm.hip. (2) The BatchNorm dropout threshold: the
kernels derive it from float32(p), ``dropout_keep_mask`` derived it from the double; fixed
in models/norm.py, and the constructed seeds of (d) hold the two together.

Shown to bite on three arithmetic-only mutants, each tried once, none kept:
(i) the LayerNorm backward not adding the second chunk's dgamma term (CH >= 2): fails all
    16 widths with CH >= 2 of ``test_layer_norm_every_width`` and both
    ``test_layer_norm_width_limits``; tests/test_kernels_gpu.py::test_layer_norm_native fails
    10 of its cases too, the rest of that file, test_batchnorm_gpu.py and test_act_gpu.py pass;
(ii) ``pair_relu``'s single-step tail loop skipped at LPR 16: fails
    ``test_pair_relu_every_variant`` at every width that reaches LPR 16 (fp32 36, 13, and 12
    through its unaligned layout; bf16 72, 13; int32 and int64) and the bf16 F = 72 zero-gate
    case; of the older tests ``test_pair_relu_modes`` at F = 64 fp32 and
    ``test_gcn_layer_gpu_matches_cpu`` fail, nothing else;
(iii) ``> 0`` turned into ``>= 0`` in ``act_grad`` of act.hip: fails
    ``test_bias_act_many_rows_and_zero_gate`` (the exact-zero case) and nothing else here;
    all 554 older tests of test_kernels_gpu.py, test_batchnorm_gpu.py and test_act_gpu.py pass.
"""
from __future__ import annotations

import functools
import time

import pytest
import torch

from dgraph_amd import _native
from dgraph_amd.models.norm import dropout_keep_mask
from test_rowwise_cases import (ACC_F, ACT_F, BN_F, COPY_F, EDGE_F, ELEM, EPS, GAP_ELEM,
                                GAP_SHAPE, LN_CONST, LN_F, LN_LIMIT, LN_PAST, MASKED_F,
                                TORCH_DT, allowance, bias_act_contract, bn_bwd_apply_contract,
                                bn_bwd_reduce_contract, bn_fwd_contract, bn_stats_contract,
                                colsum_contract, copy_rows_contract, count_case, gaa_contract,
                                gap_cases, ints, ln_bwd_contract, ln_fwd_contract,
                                ln_zero_gate, many_pattern, many_rows, masked_gather_contract,
                                off_zero, pair_relu_contract, rnd, widths, zero_gate_bias,
                                zero_gate_bn, zero_gate_gaa, zero_gate_pair)
from test_segment_cases import ladder_csr, transposed

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.25e9  # what output buffers hold before a call
DTS = ("fp32", "bf16")
IDX = (torch.int32, torch.int64)
F64, F32 = torch.float64, torch.float32
RATIOS: dict = {}
T0 = time.time()


def ops():
    return _native.ops()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(RATIOS):
        print(f"\n[rowwise variants] largest error / bound, {k}: {RATIOS[k]:.3f}", end="")
    print(f"\n[rowwise variants] wall time {time.time() - T0:.1f} s")


def dev(t, dt="fp32"):
    return None if t is None else t.to(TORCH_DT[dt]).to(DEV)


def within(tag, name, got, ref64, ref32, dt="fp32", roundings=1):
    """|got - fp64| against :func:`allowance`, element by element; prints the figures and
    records the largest ratio per (kernel, output)."""
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape, (tag, name, got.shape, ref64.shape)
    assert bool(torch.isfinite(got).all()), f"{tag} {name}: not finite"
    if not got.numel():
        return
    err = (got - ref64.double()).abs()
    lim = allowance(ref64, ref32, dt, roundings)
    ratio = float((err / lim).max())
    print(f"{tag} {name}: err {float(err.max()):.3e} allowance {float(lim.max()):.3e} "
          f"error / bound {ratio:.3f}")
    key = f"{tag.split('[')[0].strip()} {'bf16' if '[bf16' in tag else 'fp32'} {name}"
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    assert ratio <= 1.0, f"{tag} {name}: error / bound {ratio:.3f}"


def same(tag, name, got, want):
    assert torch.equal(got.detach().cpu(), want), f"{tag} {name}: differs from the contract"


# ------------------------------------------------------------------ framed operands
LAYOUTS = ("contig", "strided", "unaligned")


def geometry(F, dt, layout, vec=None):
    """(row stride, column offset): ``contig``: (F, 0); ``strided``: a wider row at an
    offset that keeps the 16-byte path (multiples of ``vec``, default 16 bytes' worth);
    ``unaligned``: one element off, odd stride: VEC = 1."""
    V = vec or 16 // ELEM[dt]
    if layout == "contig":
        return F, 0
    if layout == "strided":
        return F + 3 * V, V
    return F + 3 * V + 1, 1


def sentinel(dt):
    return torch.tensor(SENT).to(TORCH_DT[dt])


def frame(rows, F, dt, layout="contig", extra_rows=2, vec=None):
    """A sentinel-filled buffer and the [rows, F] slice of it an op writes."""
    ld, off = geometry(F, dt, layout, vec)
    buf = torch.full((rows + extra_rows, ld), SENT, dtype=TORCH_DT[dt], device=DEV)
    return buf, buf[:rows, off:off + F]


def frame_kept(tag, buf, view):
    """Outside the slice the sentinel survives bitwise; inside none does."""
    rows, F = view.shape
    off = view.storage_offset() - buf.storage_offset()
    s = sentinel("bf16" if buf.dtype == torch.bfloat16 else "fp32").to(DEV)
    outside = torch.ones_like(buf, dtype=torch.bool)
    outside[:rows, off:off + F] = False
    assert bool((buf[outside] == s).all()), f"{tag}: wrote outside its slice"
    assert not bool((view == s).any()), f"{tag}: left part of its slice unwritten"


def place(t, dt, layout="contig", vec=None, fill=77.0):
    """``t`` [rows, F] on the GPU as a slice of a wider buffer (see :func:`geometry`)."""
    if t is None:
        return None
    rows, F = t.shape
    ld, off = geometry(F, dt, layout, vec)
    if layout == "contig":
        return dev(t, dt).contiguous().clone()
    buf = torch.full((rows + 1, ld), fill, dtype=TORCH_DT[dt], device=DEV)
    buf[:rows, off:off + F] = dev(t, dt)
    return buf[:rows, off:off + F]


def table(tab):
    return [pytest.param(dt, F, id=f"{dt}-{F}") for dt in DTS for F, _ in widths(tab, dt)]


# ============================================================ (a), (b) LayerNorm
def ln_inputs(N, F, dt, kind="plain"):
    x = rnd((N, F), 100 + F, dt, kind)
    return dict(x=x, res=rnd((N, F), 101 + F, dt), dy=rnd((N, F), 102 + F, dt),
                g=rnd((F,), 103 + F), b=rnd((F,), 104 + F))


def ln_check(tag, c, dt, affine, res):
    """One forward and one backward (on the kernel's own mean / rstd) against the
    contracts."""
    g, b = (c["g"], c["b"]) if affine else (None, None)
    r = c["res"] if res else None
    y, mean, rstd = ops().layer_norm_fwd(dev(c["x"], dt), dev(g), dev(b), dev(r, dt), EPS)
    r64, r32 = ln_fwd_contract(c["x"], g, b, r), ln_fwd_contract(c["x"], g, b, r, dtype=F32)
    assert y.dtype == TORCH_DT[dt] and mean.dtype == F32 and rstd.dtype == F32
    within(tag, "y", y, r64[0], r32[0], dt, 1)
    within(tag, "mean", mean, r64[1], r32[1])
    within(tag, "rstd", rstd, r64[2], r32[2])
    dx, dg, db = ops().layer_norm_bwd(dev(c["dy"], dt), dev(c["x"], dt), mean, rstd, dev(g))
    mk, rk = mean.cpu(), rstd.cpu()
    d64 = ln_bwd_contract(c["dy"], c["x"], mk, rk, g)
    d32 = ln_bwd_contract(c["dy"], c["x"], mk, rk, g, dtype=F32)
    within(tag, "dx", dx, d64[0], d32[0], dt, 1)
    within(tag, "dgamma", dg, d64[1], d32[1])
    within(tag, "dbeta", db, d64[2], d32[2])
    return dg, db


@pytest.mark.parametrize("dt,F", table(LN_F))
def test_layer_norm_every_width(dt, F):
    for N in (203, 1031, 1):
        c = ln_inputs(N, F, dt)
        for affine in (True, False):
            for res in (True, False):
                ln_check(f"layer_norm [{dt} F={F} N={N} affine={affine} res={res}]", c, dt,
                         affine, res)


@pytest.mark.parametrize("dt,F", table(LN_F))
def test_layer_norm_big_mean_and_constant_row(dt, F):
    ln_check(f"layer_norm big-mean [{dt} F={F}]", ln_inputs(203, F, dt, "big"), dt, True, True)
    # the contract of row 5: mean 3 (1000), rstd = eps^-1/2, y = beta; one call per value,
    # so that each row is held to the bound of its own tensor
    for value in LN_CONST:
        c = ln_inputs(11, F, dt)
        c["x"] = ln_zero_gate(F, value).to(TORCH_DT[dt]).float()
        ln_check(f"layer_norm constant-row {value:g} [{dt} F={F}]", c, dt, True, False)


def test_layer_norm_many_rows():
    N, F = many_rows("ln"), 50
    ln_check(f"layer_norm many-rows [fp32 F={F} N={N}]", ln_inputs(N, F, "fp32"), "fp32",
             True, True)


def test_layer_norm_partials_repeat():
    c = ln_inputs(1031, 172, "fp32")
    a = ln_check("layer_norm repeat [fp32 F=172 N=1031]", c, "fp32", True, False)
    b = ln_check("layer_norm repeat [fp32 F=172 N=1031]", c, "fp32", True, False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("dt", DTS)
def test_layer_norm_width_limits(dt):
    """The widest width of each path runs forward AND backward (one check, ``ln_shape_ok``,
    governs both); the next width of the path raises before anything is launched."""
    for F in LN_LIMIT[dt]:
        ln_check(f"layer_norm widest [{dt} F={F}]", ln_inputs(203, F, dt), dt, True, True)
    for F in LN_PAST[dt]:
        x = dev(rnd((3, F), 1, dt), dt)
        with pytest.raises(RuntimeError, match="feature width too large"):
            ops().layer_norm_fwd(x, None, None, None, EPS)
        with pytest.raises(RuntimeError, match="feature width too large"):
            ops().layer_norm_bwd(x, x, torch.zeros(3, device=DEV), torch.ones(3, device=DEV),
                                 None)


# ================================================================ (c), (d) BatchNorm
def bn_inputs(N, F, dt, kind="plain", positive=False):
    """x, dy, the column statistics of x (fp32, as the module derives them), affine
    parameters and c1 / c2; pre-activations of both parameter sets kept off 0. ``positive``:
    x rebuilt so that every pre-activation is at least 0.4 (the dropout pattern tests)."""
    x = rnd((N, F), 200 + F, dt, kind)
    xd = x.double()
    mean = xd.mean(0).float()
    rstd = torch.rsqrt(xd.var(0, unbiased=False) + EPS).float() if N > 1 else torch.ones(F)
    g, b = rnd((F,), 201 + F), rnd((F,), 202 + F)
    if positive:
        g = g.abs() + 0.5
        pre = 0.5 + rnd((N, F), 206 + F).abs()
        x = (mean.double() + (pre.double() - b.double()) / (g.double() * rstd.double()))
        x = x.to(TORCH_DT[dt]).float()
    pres = [lambda v: (v - mean.double()) * rstd.double() * g.double() + b.double(),
            lambda v: (v - mean.double()) * rstd.double()]
    x = off_zero(x, pres, dt, step=0.5 if kind == "plain" else (8.0 if dt == "bf16" else 0.01))
    if positive:
        assert float(pres[0](x.double()).min()) > 0.4
    return dict(x=x, dy=rnd((N, F), 203 + F, dt), mean=mean, rstd=rstd, g=g, b=b,
                c1=rnd((F,), 204 + F) * 0.1, c2=rnd((F,), 205 + F) * 0.1)


def bn_run(tag, c, dt, params, relu, layout="contig", p=0.0, seed=0, keep=None, exact=False):
    """The four passes called directly on one input; returns the outputs."""
    N, F = c["x"].shape
    g, b, c1, c2 = (c["g"], c["b"], c["c1"], c["c2"]) if params else (None,) * 4
    x, dy = place(c["x"], dt, layout), place(c["dy"], dt, layout)
    center = c["x"][0].clone() if N else torch.zeros(F)
    mean, rstd = c["mean"], c["rstd"]
    stats = ops().bn_reduce(x, None, dev(center), None, None, None, False, 0, 0.0, 0)
    y = ops().bn_apply(x, None, dev(mean), dev(rstd), dev(g), dev(b), None, None, relu, 0,
                       p, seed)
    red = ops().bn_reduce(x, dy, dev(mean), dev(rstd), dev(g), dev(b), relu, 1, p, seed)
    dx = ops().bn_apply(x, dy, dev(mean), dev(rstd), dev(g), dev(b), dev(c1), dev(c2), relu, 1,
                        p, seed)
    assert stats.dtype == F64 and red.dtype == F64 and stats.shape == (2, F)
    assert y.dtype == TORCH_DT[dt] and y.shape == (N, F) and y.is_contiguous()
    out = dict(stats=stats, y=y, red=red, dx=dx)
    refs = {}
    for dtype in (F64, F32):
        refs[dtype] = dict(
            stats=bn_stats_contract(c["x"], center, dtype),
            y=bn_fwd_contract(c["x"], mean, rstd, g, b, relu, keep, p, dtype),
            red=bn_bwd_reduce_contract(c["x"], c["dy"], mean, rstd, g, b, relu, keep, p, dtype),
            dx=bn_bwd_apply_contract(c["x"], c["dy"], mean, rstd, g, b, c1, c2, relu, keep, p,
                                     dtype))
    for k in ("stats", "y", "red", "dx"):
        if exact:
            same(tag, k, out[k], refs[F64][k].to(out[k].dtype))
        else:
            within(tag, k, out[k], refs[F64][k], refs[F32][k], dt if k in ("y", "dx") else "fp32")
    return out


@pytest.mark.parametrize("dt,F", table(BN_F))
def test_batchnorm_every_variant(dt, F):
    for N in (203, 3):
        c = bn_inputs(N, F, dt)
        for layout in LAYOUTS:
            for params in (True, False):
                for relu in (False, True):
                    bn_run(f"batchnorm [{dt} F={F} N={N} {layout} params={params} relu={relu}]",
                           c, dt, params, relu, layout)


def test_batchnorm_many_rows_and_none():
    N, F = many_rows("bn"), 50
    bn_run(f"batchnorm many-rows [fp32 F={F} N={N}]", bn_inputs(N, F, "fp32"), "fp32", True, True)
    for dt in DTS:
        x = torch.empty(0, 36, dtype=TORCH_DT[dt], device=DEV)
        z = ops().bn_reduce(x, None, torch.zeros(36, device=DEV), None, None, None, False, 0,
                            0.0, 0)
        assert z.shape == (2, 36) and int(torch.count_nonzero(z)) == 0
        z = ops().bn_reduce(x, x, torch.zeros(36, device=DEV), torch.ones(36, device=DEV), None,
                            None, True, 1, 0.0, 0)
        assert z.shape == (2, 36) and int(torch.count_nonzero(z)) == 0


@pytest.mark.parametrize("dt,F", [("fp32", 68), ("fp32", 29), ("bf16", 136), ("bf16", 29)])
def test_batchnorm_big_mean_zero_gate_repeat(dt, F):
    c = bn_inputs(203, F, dt, "big")
    a = bn_run(f"batchnorm big-mean [{dt} F={F}]", c, dt, True, True)
    b = bn_run(f"batchnorm big-mean [{dt} F={F}]", c, dt, True, True)
    assert torch.equal(a["stats"], b["stats"]) and torch.equal(a["red"], b["red"])
    z = zero_gate_bn(203, F)
    for layout in ("contig", "unaligned"):
        bn_run(f"batchnorm zero-gate [{dt} F={F} {layout}]", z, dt, True, True, layout,
               exact=True)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("dt,F", [("fp32", 68), ("fp32", 29), ("bf16", 136), ("bf16", 29)])
def test_batchnorm_dropout_one_mask(dt, F, p):
    N, seed = 203, (0x1234567 << 32) + 0x89ABCDE
    c = bn_inputs(N, F, dt, positive=True)
    keep = dropout_keep_mask(seed, N, F, "cpu", p)
    tag = f"batchnorm dropout [{dt} F={F} p={p}]"
    o = bn_run(tag, c, dt, True, True, p=p, seed=seed, keep=keep)
    same(tag, "keep pattern", o["y"] != 0, keep)
    s = bn_run(tag + " strided", c, dt, True, True, "strided", p=p, seed=seed, keep=keep)
    u = bn_run(tag + " unaligned", c, dt, True, True, "unaligned", p=p, seed=seed, keep=keep)
    for k in ("y", "dx"):  # the index is r F + c, whatever the row stride
        assert torch.equal(s[k], o[k]) and torch.equal(u[k] != 0, o[k] != 0), (tag, k)


@pytest.mark.parametrize("p,seed,h,kernel_keeps", gap_cases())
def test_batchnorm_dropout_gap_elements(p, seed, h, kernel_keeps):
    """The element whose hash lies between floor(double(p) 2^32) and floor(float32(p) 2^32):
    the kernel's decision is the CPU mask's."""
    N, F = GAP_SHAPE
    r, col = GAP_ELEM
    c = bn_inputs(N, F, "fp32", positive=True)
    keep = dropout_keep_mask(seed, N, F, "cpu", p)
    assert bool(keep[r, col]) == kernel_keeps
    tag = f"batchnorm dropout gap [p={p} hash={h}]"
    o = bn_run(tag, c, "fp32", True, True, p=p, seed=seed, keep=keep)
    same(tag, "keep pattern", o["y"] != 0, keep)
    assert bool(o["y"][r, col] != 0) == kernel_keeps
    # dx carries the mask too: with c1 = c2 = 0 it is 0 exactly where dy was dropped
    c0 = dict(c, c1=torch.zeros(F), c2=torch.zeros(F))
    o = bn_run(tag + " c=0", c0, "fp32", True, True, p=p, seed=seed, keep=keep)
    assert bool(o["dx"][r, col] != 0) == kernel_keeps


# ==================================================================== (e) bias_act
def act_layouts(F):
    return LAYOUTS if F <= 256 else LAYOUTS[:2]


def bias_act_run(tag, z, b, dy, act, dt, layout="contig", exact=False):
    N, F = z.shape
    zb, dyb = place(z, dt, layout), place(dy, dt, layout)
    ybuf, y = frame(N, F, dt, layout)
    ops().bias_act(zb, dev(b), act, y)
    frame_kept(tag + " y", ybuf, y)
    dzbuf, dz = frame(N, F, dt, layout)
    db = ops().bias_act_bwd(dyb, zb, dev(b), act, dz)
    frame_kept(tag + " dz", dzbuf, dz)
    db2 = ops().bias_act_bwd(dyb, zb, dev(b), act, frame(N, F, dt, layout)[1])
    assert torch.equal(db, db2), f"{tag}: db not repeatable"
    stored = dz.detach().cpu().float()
    assert db.dtype == F32 and db.shape == (F,)
    if exact:
        same(tag, "y", y, bias_act_contract(z, b, act).to(TORCH_DT[dt]))
        same(tag, "dz", dz, bias_act_contract(z, b, act, dy).to(TORCH_DT[dt]))
        same(tag, "db", db, colsum_contract(stored).float())
        return
    within(tag, "y", y, bias_act_contract(z, b, act), bias_act_contract(z, b, act, dtype=F32),
           dt, 1)
    within(tag, "dz", dz, bias_act_contract(z, b, act, dy),
           bias_act_contract(z, b, act, dy, dtype=F32), dt, 1)
    # the bias gradient sums the STORED dz: an fp32 output, no bf16 rounding of its own
    within(tag, "db", db, colsum_contract(stored), colsum_contract(stored, F32))


@pytest.mark.parametrize("dt,F", table(ACT_F))
def test_bias_act_every_variant(dt, F):
    for N in (203, 1):
        z, dy, b = rnd((N, F), 300 + F, dt), rnd((N, F), 301 + F, dt), rnd((F,), 302 + F)
        for act in (0, 1, 2):
            for layout in act_layouts(F):
                for bias in (b, None):
                    bias_act_run(f"bias_act [{dt} F={F} N={N} act={act} {layout} "
                                 f"b={bias is not None}]", z, bias, dy, act, dt, layout)


def test_bias_act_many_rows_and_zero_gate():
    N, F = many_rows("act"), 1024
    z, dy, b = rnd((N, F), 310), rnd((N, F), 311), rnd((F,), 312)
    bias_act_run(f"bias_act many-rows [fp32 F={F} N={N}]", z, b, dy, 1, "fp32")
    for dt, F in (("fp32", 12), ("fp32", 7), ("bf16", 24), ("bf16", 73)):
        z, b, dy = zero_gate_bias(203, F)
        assert int((z + b == 0).sum()) >= 1
        bias_act_run(f"bias_act zero-gate [{dt} F={F}]", z, b, dy, 2, dt, exact=True)


@pytest.mark.parametrize("dt", DTS)
def test_bias_act_width_limits_raise(dt):
    V = 16 // ELEM[dt]
    for F, layout in ((257, "contig"), (256 * V + V, "contig"), (256 * V, "unaligned"),
                      (600 if dt == "fp32" else 1032, "unaligned")):
        z = place(rnd((5, F), 320, dt), dt, layout)
        ybuf, y = frame(5, F, dt, layout)
        with pytest.raises(RuntimeError, match="exceeds the limit of"):
            ops().bias_act(z, None, 1, y)
        with pytest.raises(RuntimeError, match="exceeds the limit of"):
            ops().bias_act_bwd(z, z, None, 1, y)
        assert bool((ybuf == sentinel(dt).to(DEV)).all())  # nothing was launched


# =================================================================== (f) pair_relu
@functools.lru_cache(maxsize=None)
def pair_case(dt, F):
    """P, Q, g on the ladder and the three modes' contracts (mode 2 on the transpose)."""
    csr = ladder_csr()
    t, _ = transposed(csr)
    P, Q = rnd((csr.num_rows, F), 400 + F, dt), rnd((csr.num_cols, F), 401 + F, dt)
    g = rnd((csr.num_rows, F), 402 + F, dt)
    refs = {}
    for dtype in (F64, F32):
        refs[dtype] = (pair_relu_contract(csr.rowptr, csr.col, 0, P, Q, dtype=dtype),
                       pair_relu_contract(csr.rowptr, csr.col, 1, P, Q, rowmul=g, dtype=dtype),
                       pair_relu_contract(t.rowptr, t.col, 2, Q, P, gat2=g, dtype=dtype))
    return P, Q, g, refs


def pair_run(tag, rowptr, col, t_rowptr, t_col, P, Q, g, refs, dt, layout="contig",
             exact=False, modes=(0, 1, 2)):
    """The three modes into framed outputs two rows taller than the pattern."""
    n, ns, F = rowptr.numel() - 1, t_rowptr.numel() - 1, P.shape[1]
    assert 0 <= int(col.min()) and int(col.max()) < Q.shape[0] and int(rowptr[-1]) == col.numel()
    assert 0 <= int(t_col.min()) and int(t_col.max()) < P.shape[0]
    Pd, Qd, gd = (place(v, dt, layout) for v in (P, Q, g))
    rp, cl, trp, tcl = (v.to(DEV) for v in (rowptr, col, t_rowptr, t_col))
    for mode in modes:
        rows = ns if mode == 2 else n
        buf, out = frame(rows, F, dt, layout)
        # contiguous: the op is handed an ``out`` TALLER than the pattern (two rows past
        # nrows, which must keep the sentinel); strided: exactly nrows rows of a taller buffer
        arg = buf[:, :F] if layout == "contig" else out
        assert arg.shape[0] == rows + (2 if layout == "contig" else 0)
        if mode == 0:
            ops().pair_relu(rp, cl, 0, Pd, Qd, None, None, arg)
        elif mode == 1:
            ops().pair_relu(rp, cl, 1, Pd, Qd, None, gd, arg)
        else:
            ops().pair_relu(trp, tcl, 2, Qd, Pd, gd, None, arg)
        frame_kept(f"{tag} mode {mode}", buf, out)
        if exact:
            same(tag, f"mode {mode}", out, refs[F64][mode].to(TORCH_DT[dt]))
        else:
            within(tag, f"mode {mode}", out, refs[F64][mode], refs[F32][mode], dt, 1)


@pytest.mark.parametrize("idx", IDX, ids=["i32", "i64"])
@pytest.mark.parametrize("dt,F", table(EDGE_F))
def test_pair_relu_every_variant(dt, F, idx):
    csr = ladder_csr(idx)
    t, _ = transposed(csr, idx)
    P, Q, g, refs = pair_case(dt, F)
    for layout in LAYOUTS:
        pair_run(f"pair_relu [{dt} F={F} {layout}]", csr.rowptr, csr.col, t.rowptr, t.col, P, Q,
                 g, refs, dt, layout)


@pytest.mark.parametrize("dt,F", [("fp32", 12), ("fp32", 29), ("fp32", 150), ("bf16", 24),
                                  ("bf16", 72), ("bf16", 7)])
def test_pair_relu_zero_gate(dt, F):
    """Integer operands: about 1 / 7 of the pre-activations are exactly 0 and must count as
    NOT positive; every sum is an exact integer, rounded once for a bf16 output."""
    csr = ladder_csr()
    t, _ = transposed(csr)
    P, Q, g = zero_gate_pair(csr, F)
    g = g[:csr.num_rows]
    refs = {F64: (pair_relu_contract(csr.rowptr, csr.col, 0, P, Q),
                  pair_relu_contract(csr.rowptr, csr.col, 1, P, Q, rowmul=g),
                  pair_relu_contract(t.rowptr, t.col, 2, Q, P, gat2=g))}
    pair_run(f"pair_relu zero-gate [{dt} F={F}]", csr.rowptr, csr.col, t.rowptr, t.col, P, Q, g,
             refs, dt, exact=True)


def test_pair_relu_many_rows():
    n, F, ns = many_rows("pair"), 12, 257
    rowptr, col = many_pattern(n, ns)
    P, Q, g = rnd((n, F), 410), rnd((ns, F), 411), rnd((n, F), 412)
    G2 = rnd((ns, F), 413)
    rp, cl = rowptr.to(DEV), col.to(torch.int32).to(DEV)
    for mode, (m, g2) in enumerate(((None, None), (g, None), (None, G2))):
        buf, out = frame(n, F, "fp32")
        ops().pair_relu(rp, cl, mode, dev(P), dev(Q), dev(g2), dev(m), out)
        frame_kept(f"pair_relu many-rows mode {mode}", buf, out)
        r64 = pair_relu_contract(rowptr, col, mode, P, Q, g2, m)
        r32 = pair_relu_contract(rowptr, col, mode, P, Q, g2, m, dtype=F32)
        within(f"pair_relu many-rows [fp32 F={F} n={n}]", f"mode {mode}", out, r64, r32)


@pytest.mark.parametrize("F", [24, 7])
def test_pair_relu_bf16_counts_above_256(F):
    """Counts of 771 and 263 times 1..7: the count stays fp32 until the one rounding of the
    product (a count rounded to bf16 first gives 772 and 264)."""
    rowptr, col, P, Q, m = count_case(F)
    buf, out = frame(3, F, "bf16")
    ops().pair_relu(rowptr.to(DEV), col.to(DEV), 1, dev(P, "bf16"), dev(Q, "bf16"), None,
                    dev(m, "bf16"), out)
    frame_kept("pair_relu counts", buf, out)
    want = pair_relu_contract(rowptr, col, 1, P, Q, rowmul=m)
    assert torch.equal(want[:, 0], torch.tensor([771.0, 263.0, 5.0], dtype=F64))
    same("pair_relu counts", "mode 1", out, want.to(torch.bfloat16))


# ============================================================== (g) gather_add_act
COMBOS = ("YPQ", "Y", "P", "Q", "PQ", "YP", "YQ", "")


def gaa_inputs(E, F, dt, nP=31, nQ=17, seed=500):
    g = torch.Generator().manual_seed(seed + F)
    src, dst = (torch.randint(0, n, (E,), generator=g) for n in (nP, nQ))
    P, Q = rnd((nP, F), seed + 1 + F, dt), rnd((nQ, F), seed + 2 + F, dt)
    Y = off_zero(rnd((E, F), seed + 3 + F, dt),
                 [lambda v: v + P.double()[src] + Q.double()[dst]], dt)
    return dict(Y=Y, P=P, Q=Q, src=src, dst=dst, gin=rnd((E, F), seed + 4 + F, dt))


def gaa_run(tag, c, dt, act, combo="YPQ", layout="contig", exact=None):
    E, F = c["gin"].shape
    assert 0 <= int(c["src"].min()) and int(c["src"].max()) < c["P"].shape[0]
    assert 0 <= int(c["dst"].min()) and int(c["dst"].max()) < c["Q"].shape[0]
    Y, P, Q = (c[k] if k in combo else None for k in "YPQ")
    Yd, Pd, Qd, gd = (place(v, dt, layout) for v in (Y, P, Q, c["gin"]))
    sd, dd = c["src"].to(DEV), c["dst"].to(DEV)
    for bwd in (False, True):
        buf, out = frame(E, F, dt, layout, extra_rows=1)
        ops().gather_add_act(Yd, Pd, sd if P is not None else None, Qd,
                             dd if Q is not None else None, gd if bwd else None, out, act)
        name = "bwd" if bwd else "fwd"
        frame_kept(f"{tag} {name}", buf, out)
        gin = c["gin"] if bwd else None
        r64 = gaa_contract(E, F, Y, P, c["src"], Q, c["dst"], act, gin)
        r32 = gaa_contract(E, F, Y, P, c["src"], Q, c["dst"], act, gin, dtype=F32)
        if exact is not None:
            same(tag, name, out, (r64 if exact == F64 else r32).to(TORCH_DT[dt]))
        else:
            within(tag, name, out, r64, r32, dt, 1)


@pytest.mark.parametrize("dt,F", table(EDGE_F))
def test_gather_add_act_every_variant(dt, F):
    c = gaa_inputs(203, F, dt)
    for act in (0, 1, 2, 3):
        for layout in LAYOUTS:
            gaa_run(f"gather_add_act [{dt} F={F} act={act} {layout}]", c, dt, act, "YPQ", layout)
        for combo in COMBOS[1:]:
            gaa_run(f"gather_add_act [{dt} F={F} act={act} terms={combo or 'none'}]", c, dt,
                    act, combo)


def test_gather_add_act_many_edges():
    E, F = many_rows("gaa"), 50
    c = gaa_inputs(E, F, "fp32", nP=1000, nQ=777)
    gaa_run(f"gather_add_act many-edges [fp32 F={F} E={E}]", c, "fp32", 2)
    gaa_run(f"gather_add_act many-edges [fp32 F={F} E={E}]", c, "fp32", 1)


@pytest.mark.parametrize("dt,F", [("fp32", 12), ("fp32", 29), ("bf16", 24), ("bf16", 7)])
def test_gather_add_act_zero_gate_and_silu_tails(dt, F):
    z = zero_gate_gaa(203, F, 31, 17)
    assert int((z["Y"] + z["P"][z["src"]] + z["Q"][z["dst"]] == 0).sum()) >= 1
    # relu: integers, equal to the fp64 contract; leaky: 0.2 x is ONE fp32 product in the
    # kernel and in the fp32 contract alike (fp64 holds another 0.2), so equal to that
    gaa_run(f"gather_add_act zero-gate relu [{dt} F={F}]", z, dt, 1, exact=F64)
    gaa_run(f"gather_add_act zero-gate leaky [{dt} F={F}]", z, dt, 3, exact=F32)
    # SiLU where __expf overflows (x = -90) and underflows (+90): finite, within the bound
    c = gaa_inputs(203, F, dt)
    c["Y"] = torch.where(rnd((203, F), 520) > 1, 90.0, -90.0)
    assert (c["Y"] == 90).any() and (c["Y"] == -90).any()
    gaa_run(f"gather_add_act silu +-90 [{dt} F={F}]", c, dt, 2, "Y")


# ===================================================== (h) copy_rows, masked_gather
def copy_indices(n, nx, nout, idx, seed):
    """Sources in [-1, nx) with about one in eight negative; distinct destinations in
    [0, nout) with about one in eight replaced by -1."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, nx, (n,), generator=g)
    src[torch.rand(n, generator=g) < 0.125] = -1
    dst = torch.randperm(nout, generator=g)[:n]
    dst[torch.rand(n, generator=g) < 0.125] = -1
    return src.to(idx), dst.to(idx)


def copy_run(tag, x, src, dst, nout, dt, layout, vec, accumulate=False):
    nx, F = x.shape
    for i, lim in ((src, nx), (dst, nout)):
        assert i is None or (int(i.min()) >= -1 and int(i.max()) < lim)
    xd = place(x, dt, layout, vec)
    buf, out = frame(nout, F, dt, layout, vec=vec)
    before = buf.cpu()
    off = out.storage_offset() - buf.storage_offset()
    ops().copy_rows(xd, None if src is None else src.to(DEV), None if dst is None else
                    dst.to(DEV), out, accumulate)
    want = before.clone()
    want[:nout, off:off + F] = copy_rows_contract(x.to(TORCH_DT[dt]), src, dst,
                                                  before[:nout, off:off + F])
    same(tag, "out and its frame", buf, want)  # bitwise, the untouched rows included


@pytest.mark.parametrize("idx", IDX, ids=["i32", "i64"])
@pytest.mark.parametrize("dt,F,path", [pytest.param(dt, F, p, id=f"{dt}-{F}") for dt in DTS
                                       for F, p in widths(COPY_F, dt)])
def test_copy_rows_every_variant(dt, F, path, idx):
    vec = {"vec": 16 // ELEM[dt], "vec2": 2, "scalar": 1}[path]
    nx = 211
    x = rnd((nx, F), 600 + F, dt)
    for n in (1, 203):
        src, dst = copy_indices(n, nx, 230, idx, 601 + F + n)
        for layout in ("contig", "strided"):
            tag = f"copy_rows [{dt} F={F} n={n} {layout}]"
            copy_run(tag + " src+dst", x, src, dst, 230, dt, layout, vec)
            copy_run(tag + " src", x, src, None, n + 3, dt, layout, vec)
            copy_run(tag + " dst", x[:n], None, dst, 230, dt, layout, vec)
        copy_run(f"copy_rows [{dt} F={F} neither]", x[:n], None, None, n + 3, dt, "contig", vec)


def test_copy_rows_many_rows():
    """131,072 + 4,099 rows at VEC 1, LPR 64 (F = 50 from a base 4 bytes off 8): 4,099 lane
    groups take a second step of four rows."""
    n, F, nx = many_rows("copy"), 50, 1000
    x = rnd((nx, F), 610)
    src, dst = copy_indices(n, nx, n + 5, torch.int32, 611)
    flat = torch.full((1 + nx * F,), 77.0, device=DEV)
    xd = flat[1:].view(nx, F)
    xd.copy_(x)
    obuf = torch.full((1 + (n + 5) * F,), SENT, device=DEV)
    out = obuf[1:].view(n + 5, F)
    assert xd.data_ptr() % 8 == 4 and out.data_ptr() % 8 == 4
    ops().copy_rows(xd, src.to(DEV), dst.to(DEV), out, False)
    want = copy_rows_contract(x, src, dst, torch.full((n + 5, F), SENT))
    same("copy_rows many-rows", "out", out, want)
    assert float(obuf[0]) == torch.tensor(SENT).item()


@pytest.mark.parametrize("idx", IDX, ids=["i32", "i64"])
@pytest.mark.parametrize("F,layout", [(F, "contig") for F in ACC_F] +
                         [(36, "strided"), (36, "unaligned"), (29, "strided")])
def test_copy_rows_accumulate(F, layout, idx):
    """fp32, every (VEC, LPR) of VEC 4 and 1 (``ACC_F``), duplicate destinations: the
    atomics' order is free, so against fp64 ``index_add_`` within the bound; rows no
    destination names stay bitwise."""
    nx, nout, n = 211, 60, 203
    g = torch.Generator().manual_seed(620 + F)
    x, acc = rnd((nx, F), 621 + F), rnd((nout, F), 622 + F)
    src = torch.randint(-1, nx, (n,), generator=g).to(idx)
    dst = torch.randint(-1, 40, (n,), generator=g).to(idx)  # rows 40.. are never named
    out = place(acc, "fp32", layout)
    ops().copy_rows(place(x, "fp32", layout), src.to(DEV), dst.to(DEV), out, True)
    r64 = copy_rows_contract(x.double(), src, dst, acc.double(), True)
    r32 = copy_rows_contract(x, src, dst, acc, True)
    within(f"copy_rows accumulate [fp32 F={F} {layout}]", "out", out, r64, r32)
    same("copy_rows accumulate", "unnamed rows", out[40:], acc[40:])
    xb = dev(x, "bf16")
    with pytest.raises(RuntimeError, match="accumulate needs fp32"):
        ops().copy_rows(xb, src.to(DEV), dst.to(DEV), torch.zeros(nout, F, dtype=torch.bfloat16,
                                                                  device=DEV), True)


@pytest.mark.parametrize("F", MASKED_F)
@pytest.mark.parametrize("dt", DTS)
def test_masked_gather_rows(dt, F):
    n, nx = 203, 97
    g = torch.Generator().manual_seed(630 + F)
    x = rnd((nx, F), 631 + F, dt)
    idx, mask = torch.randint(0, nx, (n,), generator=g), torch.randint(0, 3, (n,), generator=g)
    for layout in ("contig", "strided"):
        buf, out = frame(n, F, dt, layout)
        before = buf.cpu()
        off = out.storage_offset() - buf.storage_offset()
        ops().masked_gather_rows(place(x, dt, layout), idx.to(DEV), mask.to(DEV), 1, out)
        want = before.clone()
        want[:n, off:off + F] = masked_gather_contract(x.to(TORCH_DT[dt]), idx, mask, 1,
                                                       before[:n, off:off + F])
        same(f"masked_gather_rows [{dt} F={F} {layout}]", "out and its frame", buf, want)
        assert int((mask != 1).sum()) > 30 and int((mask == 1).sum()) > 30
