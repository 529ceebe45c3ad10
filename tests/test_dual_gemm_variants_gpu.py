"""Every compiled instantiation of the two bf16 dual-GEMM kernels -- the column-half kernel
``dual_gemm_kernel<NT, NC1, NC2>`` (36) and the B-stationary kernel
``dual_gemm_bs_kernel<NT, K, HC, HM, RELU>`` (72) -- through the raw op, against the fp64
contract of test_dual_gemm_cases.py, which holds the inputs, the oracle, the case table
(``TABLE`` / ``reach``: which instantiation each case launches, the dispatch restated) and
the CPU tests showing that the table is complete and the comparisons bite.

* ``test_table[N-K1-K2]``: every case of the shape at ``M = 289`` and ``M = 32 (3 CUs) + 17``,
  on exact data (bitwise: the output is the round-to-nearest-even bf16 of ``v``, every keep
  bit is ``v > 0``) and on full-mantissa data (``allowance``; keep bits where ``sure``).
* ``test_small_rows``: ``M`` in {1, 31, 32, 33, 255, 256, 257} once per kernel family and NT.
* ``test_layouts``: column slices of wider buffers (NaN around the inputs, a sentinel around
  the output), ``cin`` aliasing a strided ``out``, a row slice at row 256 with the matching
  slice of ``mask_in``.
* ``test_long_run``: ``M = 32 CUs (2 * 8 + 2) + 17``, one case per ring depth of the
  B-stationary kernel and one column-half case, against ``torch.matmul`` in fp64 on the GPU.
* ``test_contract_checks`` / ``test_no_rows``: what must raise before a launch, and ``M = 0``.

Every launch runs twice on fresh buffers and the two results (output buffer and mask words,
slack included) must be bitwise equal. ``mask_out`` holds ``0x5A5A...`` before every call
and is followed by guard words that must survive. ``set_dual_gemm_variant(2)`` is restored
in a ``finally``.

Words of ``mask_out`` between block ``ceil(M / 32)`` and ``tile32_mask_words(M, N)`` (the
256-row padding) are outside the contract; what each kernel does with them is in the RECORD.

RECORD (MI355X; printed by ``test_zz_record``, not an input to any bound):
  largest error / allowance on full-mantissa data: B-stationary 0.989, column-half 0.992
  (half a bf16 ulp of a value just above a power of two is 2^-8 of it; the accumulation
  term is a small part); exact data: no output and no mask word differed in any case; all
  108 instantiations launched; no two runs differed.
  Padding words of mask_out: the column-half kernel writes 0 to all of them (each of its 8
  waves stores the words of its 32 rows, kept or not), the B-stationary kernel leaves them
  as they were (it runs no tile past ``ceil(M / 32)``).
"""
from __future__ import annotations

import contextlib

import pytest
import torch

import test_dual_gemm_cases as C
from dgraph_amd.ops import reference as R
from dgraph_amd.ops.dense import tile32_mask_words

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
WORST: dict = {}    # kernel family -> largest error / allowance on full-mantissa data
LAUNCHED: set = set()
BETWEEN: dict = {}  # kernel family -> what it left in the padding words of mask_out


def _ops():
    from dgraph_amd import _native

    return _native.ops()


def cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


@contextlib.contextmanager
def variant(v: int):
    ops = _ops()
    try:
        ops.set_dual_gemm_variant(v)
        yield ops
    finally:
        ops.set_dual_gemm_variant(2)


def upload(c, P=None, SP=None):
    """The operands of a shape on the device, with the fp64 product of the CPU oracle."""
    if P is None:
        P, SP = C.product(c)
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in c.items()}
    d["P"], d["SP"] = P.to(DEV), SP.to(DEV)
    d["M"], d["N"] = c["A1"].shape[0], c["B1t"].shape[0]
    d["mask_in"] = R.tile32_encode(c["keep_in"]).to(DEV)
    d["keep_in_cpu"] = c["keep_in"]
    return d


def _in_cols(t, off, ld):
    """``t`` as a column slice of a NaN-filled ``[rows, ld]`` buffer."""
    if t is None:
        return None
    buf = torch.full((t.shape[0], ld), float("nan"), dtype=t.dtype, device=DEV)
    v = buf[:, off:off + t.shape[1]]
    v.copy_(t)
    return v


def _in_rows(t, pre):
    """``t`` as the rows ``pre:`` of a buffer whose first ``pre`` rows are NaN."""
    if t is None:
        return None
    buf = torch.full((pre + t.shape[0], t.shape[1]), float("nan"), dtype=t.dtype, device=DEV)
    buf[pre:].copy_(t)
    return buf[pre:]


def fresh(d, flags, layout):
    """Freshly allocated operands of one launch: (args of the op, out, out buffer, mask_out)."""
    cin, mask_in, relu = flags
    M, N = d["M"], d["N"]
    A1, A2 = d["A1"], d["A2"]
    ct = d["cin"] if cin else None
    mi = d["mask_in"] if mask_in else None
    bf = dict(dtype=torch.bfloat16, device=DEV)
    if layout == "cols":
        A1 = _in_cols(A1, 8, A1.shape[1] + 8)
        A2 = None if A2 is None else _in_cols(A2, 8, A2.shape[1] + 8)
        ct = _in_cols(ct, N // 2, 2 * N)
        obuf = torch.full((M, 2 * N), C.SENT, **bf)
        out = obuf[:, N // 2:N // 2 + N]
    elif layout == "alias":
        assert cin
        obuf = torch.full((M, 2 * N), C.SENT, **bf)
        out = obuf[:, N // 2:N // 2 + N]
        out.copy_(d["cin"])
        ct = out
    elif layout == "rows":
        A1, A2, ct = _in_rows(A1, 256), _in_rows(A2, 256), _in_rows(ct, 256)
        obuf = torch.full((256 + M, N), C.SENT, **bf)
        out = obuf[256:]
        if mask_in:
            g = torch.Generator().manual_seed(5)
            whole = torch.cat([torch.rand(256, N, generator=g) > 0.5, d["keep_in_cpu"]])
            w0, wh = tile32_mask_words(256, N), tile32_mask_words(M, N)
            mi = R.tile32_encode(whole).to(DEV)[w0:w0 + wh]
    else:
        obuf = out = torch.full((M, N), C.SENT, **bf)
    mo = None
    if relu:
        mo = torch.full((tile32_mask_words(M, N) + GUARD,), C.FILL, dtype=torch.int64,
                        device=DEV)
    args = (A1, d["B1t"], A2, d["B2t"], d["bias"], ct, out, mo, mi, bool(relu))
    return args, out, obuf, mo


def outside_ok(obuf, layout, N) -> bool:
    if layout in ("cols", "alias"):
        return bool((obuf[:, :N // 2] == C.SENT).all() and (obuf[:, N // 2 + N:] == C.SENT).all())
    if layout == "rows":
        return bool((obuf[:256] == C.SENT).all())
    return True


def bits(t):
    return t.contiguous().view(torch.int16)


def run_case(d, v, flags, layout=None, label=""):
    """One case: two launches on fresh buffers, bitwise equal; then against the oracle."""
    cin, mask_in, relu = flags
    M, N, K = d["M"], d["N"], d["K"]
    K1 = d["A1"].shape[1]
    name = C.reach(v, N, K1, K - K1, *flags)
    fam = name[0]
    tag = f"{name} M={M} {d['data']} {layout or 'contig'} {label}"
    with variant(v) as ops:
        args, out, obuf, mo = fresh(d, flags, layout)
        ops.dual_gemm(*args)
        args2, _, obuf2, mo2 = fresh(d, flags, layout)
        ops.dual_gemm(*args2)
        torch.cuda.synchronize()
    LAUNCHED.add(name)
    assert torch.equal(bits(obuf), bits(obuf2)), f"{tag}: two runs differ in out"
    if relu:
        assert torch.equal(mo, mo2), f"{tag}: two runs differ in mask_out"
    assert outside_ok(obuf, layout, N), f"{tag}: wrote around the output slice"
    kin = d["keep_in"] if mask_in else None
    e = C.epilogue(d["P"], d["SP"], d["bias"], d["cin"] if cin else None, kin, relu)
    W, nw = tile32_mask_words(M, N), (M + 31) // 32 * (N // 32) * 16
    if relu:
        assert bool((mo[W:] == C.FILL).all()), f"{tag}: wrote past tile32_mask_words"
        if nw < W:
            mid = mo[nw:W]
            BETWEEN.setdefault(fam, set()).add(
                "untouched" if bool((mid == C.FILL).all()) else
                "zeroed" if bool((mid == 0).all()) else "mixed")
    if d["data"] == "exact":
        C.exact_ok(d, e)
        want = e["out"].float().bfloat16()
        bad = int((bits(out) != bits(want)).sum())
        print(f"{tag}: {bad} of {out.numel()} outputs differ from the rounded fp64 value")
        assert bad == 0, tag
        if relu:
            ww = R.tile32_encode(e["keep"].cpu())[:nw].to(DEV)
            badw = int((mo[:nw] != ww).sum())
            print(f"{tag}: {badw} of {nw} mask words differ")
            assert badw == 0, tag
    else:
        s = C.sure(e, K, kin)
        omit = float((~s).double().mean())
        assert omit <= C.OMIT_CAP, (tag, omit)
        ratio = float(((out.double() - e["out"]).abs() / C.allowance(e, K)).max())
        WORST[fam] = max(WORST.get(fam, 0.0), ratio)
        print(f"{tag}: error / allowance {ratio:.3f} (keep bits not compared: {omit:.2e})")
        assert ratio <= 1.0, tag
        if relu:
            dec = R.tile32_decode(mo[:W].cpu(), M, N)
            assert torch.equal(R.tile32_encode(dec)[:nw], mo[:nw].cpu()), \
                f"{tag}: bits of rows past M are set"
            dec = dec.to(DEV)
            assert torch.equal(dec[s], e["keep"][s]), tag
            assert bool((out[~dec] == 0).all()), f"{tag}: output not 0 where its keep bit is 0"
    if mask_in:
        assert bool((out[~d["keep_in"]] == 0).all()), tag


@pytest.mark.parametrize("N,K1,K2", C.SHAPES, ids=lambda s: str(s))
def test_table(N, K1, K2):
    for M in (C.M_TAIL, C.m_cus(cus())):
        for data in ("exact", "full"):
            d = upload(C.make_inputs(N, K1, K2, M, data))
            for v, flag_list in C.shape_runs(N, K1, K2):
                for flags in flag_list:
                    run_case(d, v, flags)


@pytest.mark.parametrize("N", C.NS)
@pytest.mark.parametrize("v", [1, 2])
def test_small_rows(v, N):
    K1, K2 = C.LAYOUT_SHAPES[v]
    for M in C.SMALL_MS:
        for data in ("exact", "full"):
            d = upload(C.make_inputs(N, K1, K2, M, data))
            for flags in ((1, 1, 1), (0, 0, 1), (0, 1, 0)):
                run_case(d, v, flags)


@pytest.mark.parametrize("layout", C.LAYOUTS)
@pytest.mark.parametrize("N", C.NS)
@pytest.mark.parametrize("v", [1, 2])
def test_layouts(v, N, layout):
    K1, K2 = C.LAYOUT_SHAPES[v]
    for data in ("exact", "full"):
        d = upload(C.make_inputs(N, K1, K2, C.M_TAIL, data))
        for flags in ((1, 1, 1), (1, 0, 1) if layout == "alias" else (0, 1, 0)):
            run_case(d, v, flags, layout)


def test_relu_without_mask_out():
    """``relu`` with no ``mask_out``: the output alone."""
    for v in (1, 2):
        d = upload(C.make_inputs(128, 128, 128, C.M_TAIL, "exact"))
        e = C.epilogue(d["P"], d["SP"], d["bias"], None, None, True)
        with variant(v) as ops:
            out = torch.full((C.M_TAIL, 128), C.SENT, dtype=torch.bfloat16, device=DEV)
            ops.dual_gemm(d["A1"], d["B1t"], d["A2"], d["B2t"], d["bias"], None, out, None,
                          None, True)
        assert torch.equal(bits(out), bits(e["out"].float().bfloat16()))


@pytest.mark.parametrize("case", C.long_cases(), ids=lambda c: "-".join(map(str, c)))
def test_long_run(case):
    """Many tiles per block (the rings reach their steady state and turn over), exact data,
    against ``torch.matmul`` in fp64 on the device; twice, bitwise."""
    v, N, K1, K2, *flags = case
    M = C.m_long(cus())
    c = C.make_inputs(N, K1, K2, M, "exact")
    dc = {k: (t.to(DEV) if torch.is_tensor(t) else t) for k, t in c.items()}
    P = torch.matmul(dc["A1"].double(), dc["B1t"].double().t())
    if K2:
        P += torch.matmul(dc["A2"].double(), dc["B2t"].double().t())
    # exact data: S only has to stay below 2^11, and 2 (K1 + K2) + 4 bounds it
    d = upload(c, P, torch.full_like(P, 2.0 * (K1 + K2) + 4))
    del P
    name = C.reach(*case)
    if name[0] == "bs":
        print(f"{name}: NBUF = {C.bs_nbuf(name[1], name[2], name[3], name[4])}, "
              f"{(M + 31) // 32 // cus()} tiles per block")
    run_case(d, v, tuple(flags), label="long")


def test_contract_checks():
    """Each violation raises before any launch and leaves ``out`` as it was."""
    M, N, K = 64, 128, 128
    bf = dict(dtype=torch.bfloat16, device=DEV)
    A = torch.ones(M, K, **bf)
    Bt = torch.ones(N, K, **bf)
    ok_words = tile32_mask_words(M, N)
    ops = _ops()

    def refuses(out_shape=(M, N), **kw):
        out = torch.full(out_shape, C.SENT, **bf)
        a = dict(A1=A, B1t=Bt, A2=None, B2t=None, bias=None, cin=None, out=out, mask_out=None,
                 mask_in=None, relu=False)
        a.update(kw)
        out = a["out"]
        before = out.clone()
        with pytest.raises(RuntimeError):
            ops.dual_gemm(a["A1"], a["B1t"], a["A2"], a["B2t"], a["bias"], a["cin"], out,
                          a["mask_out"], a["mask_in"], a["relu"])
        torch.cuda.synchronize()
        assert torch.equal(bits(out), bits(before))

    for v in (1, 2):
        with variant(v):
            refuses(out_shape=(M, 160), B1t=torch.ones(160, K, **bf))             # N
            refuses(A1=torch.ones(M, 64, **bf), B1t=torch.ones(N, 64, **bf))      # K1
            refuses(A2=torch.ones(M, 64, **bf), B2t=torch.ones(N, 64, **bf))      # K2
            refuses(A1=torch.ones(M, K + 4, **bf)[:, :K])                          # row stride
            refuses(A1=torch.ones(M * K + 1, **bf)[1:].view(M, K))                 # base + 1
            refuses(out=torch.full((M * N + 1,), C.SENT, **bf)[1:].view(M, N))
            refuses(out=torch.full((M, N + 4), C.SENT, **bf)[:, :N])
            refuses(B1t=torch.ones(N, K + 8, **bf)[:, :K])                         # B1t strided
            refuses(B1t=torch.ones(K, N, **bf).t())
            refuses(mask_in=torch.zeros(ok_words - 1, dtype=torch.int64, device=DEV))
            refuses(relu=True, mask_out=torch.zeros(ok_words - 1, dtype=torch.int64, device=DEV))
            refuses(cin=torch.ones(M, N - 32, **bf))                               # cin shape
            refuses(cin=torch.ones(M - 1, N, **bf))
            refuses(cin=torch.ones(M, N + 4, **bf)[:, :N])
            refuses(A1=torch.ones(M, K, device=DEV))                               # fp32
            refuses(B1t=torch.ones(N, K, device=DEV))
            refuses(out=torch.full((M, N), C.SENT, device=DEV))
            refuses(cin=torch.ones(M, N, device=DEV))
            refuses(mask_in=torch.zeros(ok_words, dtype=torch.int32, device=DEV))


def test_no_rows():
    """``M = 0`` returns without a launch: nothing is written."""
    bf = dict(dtype=torch.bfloat16, device=DEV)
    for v in (1, 2):
        with variant(v) as ops:
            mo = torch.full((GUARD,), C.FILL, dtype=torch.int64, device=DEV)
            back = torch.full((4, 128), C.SENT, **bf)
            ops.dual_gemm(torch.ones(0, 128, **bf), torch.ones(128, 128, **bf), None, None,
                          torch.ones(128, device=DEV), None, back[:0], mo, None, True)
            torch.cuda.synchronize()
            assert bool((mo == C.FILL).all()) and bool((back == C.SENT).all())


def test_zz_record():
    """Prints what the module docstring records."""
    print("largest error / allowance on full-mantissa data:",
          {k: round(v, 3) for k, v in sorted(WORST.items())})
    print("mask_out words of the 256-row padding:", {k: sorted(v) for k, v in BETWEEN.items()})
    print("instantiations launched in this run:", len(LAUNCHED))
