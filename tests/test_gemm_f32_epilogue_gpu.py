"""gemm_f32's epilogue and staging (csrc/kernels/gemm_f32.hip) at every tile shape, around the
16-row fragment and the 256-row block, and with more tiles than CUs, for each epilogue operand
alone and all together. Every case runs the same call twice: on contiguous, 16-byte aligned
tensors, and on views shifted by one float, ``buf[:, 1:1 + N]`` of an ``[rows, N + 4]`` buffer
(the Python wrapper and the binding accept such views: unit column stride is all they ask). The
first result is checked against fp64 on the CPU over the whole product, the second must equal
the first bitwise, and everything the call must not write keeps its sentinel. An epilogue with
16-byte accesses for aligned operands (measured and not kept: PERFORMANCE.md, round 8) has to
pass this file unchanged: the shifted views are what would take the 4-byte path beside it.

Inputs as in tests/test_f32_kernels_gpu.py: unit-normal A, B / 8; tolerance of the dual-GEMM
tests there (atol=1e-4, rtol=1e-5)."""
import functools

import pytest
import torch

from dgraph_amd.ops import f32 as F32

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENT = -7.0
PAD = 37  # extra output rows under o_rows

KS = [(32, 0), (64, 0), (128, 128)]  # one stage (it also prefetches the next tile); two; dual
NS = [64, 128, 176, 192, 256]
SMALL_MS = [1, 15, 17, 255, 257, 773]
OPERANDS = ["bias", "cin_beta", "cin_alias", "gate", "gate_alias", "relu", "row_scale", "a_rows",
            "o_rows", "all"]
ALL = {"bias", "cin_alias", "gate", "relu", "row_scale", "a_rows", "o_rows"}


def _big_m():
    # 2 x 256 x CUs + 5 rows: every persistent block pulls more than one 256-row tile
    return 2 * 256 * torch.cuda.get_device_properties(0).multi_processor_count + 5


@functools.lru_cache(maxsize=4)
def _inputs(M, K1, K2):
    """The operands of one (M, K) shape on the CPU, shared by the cases that use it; nobody
    writes to them."""
    g = torch.Generator().manual_seed(1000003 * K1 + 7919 * K2 + M)
    d = dict(src=torch.randn(M + 50, K1, generator=g),
             a_rows=torch.randperm(M + 50, generator=g)[:M],
             A2=torch.randn(M, K2, generator=g) if K2 else None,
             B1=torch.randn(K1, 256, generator=g) / 8,
             B2=torch.randn(K2, 256, generator=g) / 8 if K2 else None,
             bias=torch.randn(256, generator=g), rs=torch.rand(M, generator=g) + 0.5,
             o_rows=torch.randperm(M + PAD, generator=g)[:M],
             cin=torch.randn(M + PAD, 256, generator=g),
             gate=torch.randn(M + PAD, 256, generator=g))
    return d


def _shifted(t):
    """A copy of ``t`` as the view buf[:, 1:1 + N] of a sentinel-filled [rows, N + 4] buffer."""
    buf = torch.full((t.shape[0], t.shape[1] + 4), SENT, device=t.device)
    v = buf[:, 1:1 + t.shape[1]]
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return buf, v


def _case(M, N, K1, K2, ops):
    """Runs one call on aligned tensors and on shifted views. Returns (aligned result, fp64
    reference), both on the CPU over all output rows."""
    d = _inputs(M, K1, K2)
    gather, scatter = "a_rows" in ops, "o_rows" in ops
    rows = M + PAD if scatter else M
    A1 = (d["src"] if gather else d["src"][:M]).to(DEV)
    B1 = d["B1"][:, :N].contiguous().to(DEV)
    A2 = d["A2"].to(DEV) if K2 else None
    B2 = d["B2"][:, :N].contiguous().to(DEV) if K2 else None
    cin_sep, cin_al = "cin_beta" in ops, "cin_alias" in ops
    gate_sep, gate_al = "gate" in ops, "gate_alias" in ops
    beta = 0.75 if (cin_sep or cin_al) else 1.0
    # what out holds before the call: read through an aliasing operand, else a sentinel
    init = d["cin"][:rows, :N].contiguous() if (cin_al or gate_al) else torch.full((rows, N), SENT)
    cin0 = d["cin"][:rows, :N].contiguous() if cin_sep else (init if cin_al else None)
    gate0 = d["gate"][:rows, :N].contiguous() if gate_sep else (init if gate_al else None)
    kw = dict(a_rows=d["a_rows"].to(DEV) if gather else None,
              bias=d["bias"][:N].contiguous().to(DEV) if "bias" in ops else None,
              o_rows=d["o_rows"].to(DEV) if scatter else None, relu="relu" in ops, beta=beta,
              row_scale=d["rs"].to(DEV) if "row_scale" in ops else None)

    # contiguous, 16-byte aligned tensors
    out = init.to(DEV)
    assert out.data_ptr() % 16 == 0 and out.stride(0) % 4 == 0
    F32.gemm_f32(A1, B1, A2, B2, out=out,
                 cin=out if cin_al else (cin0.to(DEV) if cin_sep else None),
                 gate=out if gate_al else (gate0.to(DEV) if gate_sep else None), **kw)
    # the same call on views shifted by one float
    obuf, oview = _shifted(init.to(DEV))
    cbuf = gbuf = None
    cv = gv = None
    if cin_sep:
        cbuf, cv = _shifted(cin0.to(DEV))
    if gate_sep:
        gbuf, gv = _shifted(gate0.to(DEV))
    F32.gemm_f32(A1, B1, A2, B2, out=oview, cin=oview if cin_al else cv,
                 gate=oview if gate_al else gv, **kw)
    torch.cuda.synchronize()
    assert torch.equal(oview, out), "shifted views differ from aligned tensors"
    assert bool((obuf[:, 0] == SENT).all()) and bool((obuf[:, 1 + N:] == SENT).all())
    for b, src0 in ((cbuf, cin0), (gbuf, gate0)):  # read-only operands are not written
        if b is not None:
            assert torch.equal(b[:, 1:1 + N].cpu(), src0)

    # fp64 on the CPU
    a = d["src"].double()[d["a_rows"]] if gather else d["src"][:M].double()
    v = a @ d["B1"][:, :N].double()
    if K2:
        v = v + d["A2"].double() @ d["B2"][:, :N].double()
    o = d["o_rows"] if scatter else torch.arange(M)
    if "row_scale" in ops:
        v = v * d["rs"].double().unsqueeze(1)
    if "bias" in ops:
        v = v + d["bias"][:N].double()
    if cin0 is not None:
        v = v + beta * cin0[o].double()
    if gate0 is not None:
        v = torch.where(gate0[o] > 0, v, torch.zeros_like(v))
    if "relu" in ops:
        v = v.clamp_min(0)
    ref = init.double().clone()  # rows the call does not address keep what they held
    ref[o] = v
    got = out.cpu()
    untouched = torch.ones(rows, dtype=torch.bool)
    untouched[o] = False
    assert torch.equal(got[untouched], init[untouched])
    return got, ref


def _check(M, N, K1, K2, ops):
    got, ref = _case(M, N, K1, K2, ops)
    torch.testing.assert_close(got.double(), ref, atol=1e-4, rtol=1e-5)


@pytest.mark.parametrize("K1,K2", KS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", SMALL_MS)
def test_gemm_f32_epilogue_shapes(M, N, K1, K2):
    """Every epilogue operand together, at every tile shape and row count around the 16-row
    fragment and the 256-row block."""
    _check(M, N, K1, K2, ALL)


@pytest.mark.parametrize("N", NS)  # (varies fastest: one set of inputs per K)
@pytest.mark.parametrize("K1,K2", KS)
def test_gemm_f32_epilogue_many_tiles(N, K1, K2):
    """2 x 256 x CUs + 5 rows: every block pulls more than one tile (the next tile's first
    stage is in flight across the epilogue's loads and stores)."""
    _check(_big_m(), N, K1, K2, ALL)


@pytest.mark.parametrize("ops", OPERANDS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K1,K2", [(32, 0), (128, 128)])
def test_gemm_f32_epilogue_operands(K1, K2, N, ops):
    """Each epilogue operand alone, and all together, over several tiles with a partial last
    one. o_rows is a permutation into a taller sentinel-filled buffer."""
    _check(773, N, K1, K2, ALL if ops == "all" else {ops})


def test_gemm_f32_epilogue_cin_separate_gate_alias():
    """The other pairing of the in-place operands: cin its own tensor, gate read from out."""
    _check(773, 256, 128, 128, {"bias", "cin_beta", "gate_alias", "row_scale"})


@pytest.mark.parametrize("N", [176, 256])
def test_gemm_f32_epilogue_send_rows(N):
    """The fused halo pack on aligned tensors and on shifted views: rows sent to 0, 1 and 3 peers; the send rows equal
    the output rows bitwise and every other send-buffer row keeps its sentinel."""
    g = torch.Generator().manual_seed(N)
    M, K = 1000, 128
    x = torch.randn(M, K, generator=g)
    W = torch.randn(K, N, generator=g) / 8
    bias = torch.randn(N, generator=g)
    cnt = torch.tensor([0, 1, 3])[torch.randint(0, 3, (M,), generator=g)]
    ptr = torch.zeros(M + 1, dtype=torch.long)
    ptr[1:] = torch.cumsum(cnt, 0)
    n_send = int(ptr[-1])
    pos = torch.randperm(n_send + 7, generator=g)[:n_send].to(torch.int32)
    ref = (x.double() @ W.double() + bias.double()).clamp_min(0)
    rows = torch.repeat_interleave(torch.arange(M), cnt)
    written = torch.zeros(n_send + 7, dtype=torch.bool)
    written[pos.long()] = True
    outs = []
    for shifted in (False, True):
        if shifted:
            sbuf, send = _shifted(torch.full((n_send + 7, N), SENT, device=DEV))
            obuf, out = _shifted(torch.full((M, N), SENT, device=DEV))
        else:
            send = torch.full((n_send + 7, N), SENT, device=DEV)
            out = torch.full((M, N), SENT, device=DEV)
        F32.gemm_f32(x.to(DEV), W.to(DEV), bias=bias.to(DEV), relu=True, out=out,
                     send=(send, ptr.to(DEV), pos.to(DEV)))
        torch.cuda.synchronize()
        so, oc = send.cpu(), out.cpu()
        assert torch.equal(so[pos.long()], oc[rows])
        assert bool((so[~written] == SENT).all())
        if shifted:
            assert bool((sbuf[:, 0] == SENT).all()) and bool((sbuf[:, 1 + N:] == SENT).all())
            assert bool((obuf[:, 0] == SENT).all()) and bool((obuf[:, 1 + N:] == SENT).all())
        outs.append(oc)
    torch.testing.assert_close(outs[0].double(), ref, atol=1e-4, rtol=1e-5)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("N", [176, 256])
def test_gemm_f32_epilogue_run_to_run(N):
    """Two runs of the largest M under the dynamic tile schedule: bitwise equal."""
    M = _big_m()
    d = _inputs(M, 128, 128)
    A1, A2 = d["src"][:M].to(DEV), d["A2"].to(DEV)
    B1, B2 = d["B1"][:, :N].contiguous().to(DEV), d["B2"][:, :N].contiguous().to(DEV)
    bias = d["bias"][:N].contiguous().to(DEV)
    runs = [F32.gemm_f32(A1, B1, A2, B2, bias=bias, relu=True) for _ in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(runs[0], runs[1])
