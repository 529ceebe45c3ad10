"""The per-edge dot product kernel (csrc/kernels/sddmm.hip) on the GPU at every path, against
the contract of tests/test_edge_dot.py evaluated in fp64.

Accuracy rule: ``|kernel - fp64| <= test_gat_kernels.bound(ref64, ref32)`` with both
references from the contract (fp32: one term at a time); nothing is taken from the kernel's
own output. For bf16 the contract takes the bf16-rounded inputs, whose products are exact in
fp32. Every ``error / bound`` is printed before it is asserted.

Largest error / bound seen on an MI355X (the floor of the bound, 2e-5 of the largest value,
is what most cases meet; the kernel's fma's are closer to fp64 than the fp32 contract is):

    forward, every path, fp32     0.007      bf16                      0.005
    with row_scale and scale      0.007      more than one grid sweep  0.003
    op da                         0.107      op db                     0.011
    aggregate dw                  0.004      decoder loss / dz         0.002 / 0.003
    W = 2 scores / da / db        0.005 / 0.006 / 0.004
"""
from __future__ import annotations

import dataclasses
import functools

import pytest
import torch

from conftest import rank_device, run_ranks
from dgraph_amd.ops import kernels as K
from dgraph_amd.ops.aggregate import aggregate
from dgraph_amd.ops.csr import CSR
from test_edge_dot import edge_dot_contract
from test_gat_kernels import bound
from test_pna import skewed_csr, values

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.25e9  # what the score buffer holds outside the block the kernel may write
RATIOS: dict = {}

# (F, heads) and whether the shape must take the vector path
CASES = {(1, 1): False, (3, 1): False, (3, 3): False, (4, 1): True, (8, 2): True,
         (12, 4): False, (64, 1): True, (64, 4): True, (64, 16): True, (172, 1): False,
         (256, 8): True, (512, 8): True, (600, 1): False, (600, 3): False,
         # heads wider than one wave's 256 columns (2 and 4 column blocks), and past the limit
         (512, 1): True, (2048, 2): True, (2048, 1): False}
BF16_CASES = [(8, 2), (64, 4), (172, 1), (600, 3), (512, 1)]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(RATIOS):
        print(f"\n[edge_dot] largest error / bound, {k}: {RATIOS[k]:.3f}", end="")


def within(tag, name, got, ref64, ref32):
    """|got - fp64| against :func:`bound`; prints the figures, records the ratio."""
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape, f"{tag} {name}: shape {got.shape} != {ref64.shape}"
    assert bool(torch.isfinite(got).all()), f"{tag} {name}: not finite"
    err = float((got - ref64.double()).abs().max()) if got.numel() else 0.0
    bd = bound(ref64, ref32)
    print(f"{tag} {name}: err {err:.3e} bound {bd:.3e} ratio {err / bd:.3f}")
    key = f"{tag.split('[')[0]} {name}"
    RATIOS[key] = max(RATIOS.get(key, 0.0), err / bd)
    assert err <= bd, f"{tag} {name}: error {err:.3e} above the bound {bd:.3e}"


def inputs(F, dtype=torch.float32):
    """a [300, F] and b [257, F] of the skewed case, rounded to ``dtype`` (as fp32)."""
    a, b = values("plain", 300, F, F + 1), values("plain", 257, F, F + 2)
    return a.to(dtype).float(), b.to(dtype).float()


@functools.lru_cache(maxsize=None)
def refs(F, heads, dtype=torch.float32, scale=1.0, scaled_rows=False):
    """(a, b, row_scale, fp64 scores, fp32 scores) of the skewed case, shared by the index
    widths and the layouts."""
    csr = skewed_csr()
    a, b = inputs(F, dtype)
    rs = torch.linspace(0.25, 2.0, 300) if scaled_rows else None
    r64 = edge_dot_contract(csr.rowptr, csr.col, a, b, heads, scale, rs)
    r32 = edge_dot_contract(csr.rowptr, csr.col, a, b, heads, scale, rs, dtype=torch.float32)
    return a, b, rs, r64, r32


def run(csr, a, b, heads, scale=1.0, rs=None):
    """The kernel into a narrow view of a sentinel buffer; asserts the tail stays untouched."""
    buf = torch.full((csr.nnz + 8, heads), SENT, device=a.device)
    s = K.edge_dot(csr.rowptr, csr.col, a, b, buf[:csr.nnz], heads=heads, scale=scale,
                   row_scale=rs)
    assert s.data_ptr() == buf.data_ptr()
    assert bool((buf[csr.nnz:] == SENT).all()), "the kernel wrote past its scores"
    return s


@pytest.mark.parametrize("F,heads", list(CASES))
@pytest.mark.parametrize("idx", [torch.int32, torch.int64])
def test_forward(F, heads, idx):
    assert K.edge_dot_vec_path(F, heads) == CASES[(F, heads)]
    a, b, _, r64, r32 = refs(F, heads)
    csr = skewed_csr(idx).to(DEV)
    s = run(csr, a.to(DEV), b.to(DEV), heads)
    within(f"fwd[F={F},H={heads}]", "s", s, r64, r32)


@pytest.mark.parametrize("F,heads", BF16_CASES)
@pytest.mark.parametrize("idx", [torch.int32, torch.int64])
def test_forward_bf16(F, heads, idx):
    a, b, _, r64, r32 = refs(F, heads, torch.bfloat16)
    csr = skewed_csr(idx).to(DEV)
    s = run(csr, a.to(DEV).bfloat16(), b.to(DEV).bfloat16(), heads)
    assert s.dtype == torch.float32
    within(f"bf16[F={F},H={heads}]", "s", s, r64, r32)


@pytest.mark.parametrize("F,heads", [(3, 1), (64, 4), (172, 1), (512, 1)])
def test_row_scale_and_scale(F, heads):
    a, b, rs, r64, r32 = refs(F, heads, torch.float32, -0.35, True)
    csr = skewed_csr(torch.int32).to(DEV)
    s = run(csr, a.to(DEV), b.to(DEV), heads, -0.35, rs.to(DEV))
    within(f"scaled[F={F},H={heads}]", "s", s, r64, r32)


@pytest.mark.parametrize("F,heads", [(3, 1), (8, 2), (64, 4), (172, 1), (256, 8), (600, 3)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bitwise_runs_index_widths_and_layouts(F, heads, dtype):
    """Two runs, the two index widths, and a / b as the column halves of one [N, 2F] buffer
    all give the same bits."""
    a, b = (t.to(DEV).to(dtype) for t in inputs(F, dtype))
    c32, c64 = skewed_csr(torch.int32).to(DEV), skewed_csr(torch.int64).to(DEV)
    s = run(c32, a, b, heads).clone()
    assert torch.equal(run(c32, a, b, heads), s)
    assert torch.equal(run(c64, a, b, heads), s)
    buf = torch.zeros(300, 2 * F, device=DEV, dtype=dtype)
    buf[:, :F], buf[:257, F:] = a, b
    ha, hb = buf[:, :F], buf[:257, F:]
    assert ha.stride(0) == 2 * F and hb.stride(0) == 2 * F
    assert torch.equal(run(c32, ha, hb, heads), s)


def sweep_pattern(total):
    """At least ``total`` slots in blocks of 70 rows / 5,000 slots: a 700-entry row, a row that
    ends at slot 1024 (a multiple of every chunk size) followed by 40 empty rows, 24 rows of
    one entry, a 3,000-entry row, a row of 2, an empty row, a 950-entry row."""
    block = [700, 324] + [0] * 40 + [1] * 24 + [3000, 2, 0, 950]
    deg = torch.tensor(block * (total // 5000 + 1))
    rowptr = torch.zeros(deg.numel() + 1, dtype=torch.long)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, 257, (int(rowptr[-1]),), generator=torch.Generator().manual_seed(9),
                        dtype=torch.int32)
    return CSR(rowptr, col, 257)


def test_more_slots_than_one_sweep_of_the_grid():
    """F = 4 with more slots than the launch's grid cap covers in one sweep: waves take a
    second chunk; rows straddle the chunks and a run of empty rows starts at a boundary."""
    from dgraph_amd import _native

    sweep = K.edge_dot_sweep_slots(4, 1)
    chunk = int(_native.ops().edge_dot_chunk_slots(4, 1))
    csr = sweep_pattern(sweep + 3 * chunk)
    assert csr.nnz > sweep + 2 * chunk
    deg, rp = csr.degree(), csr.rowptr
    assert 1024 % chunk == 0 and int(rp[2]) == 1024 and int(deg[2:42].sum()) == 0
    # rows that straddle a chunk boundary
    assert int(((rp[:-1] // chunk) != ((rp[1:] - 1).clamp(min=0) // chunk))[deg > 1].sum()) > 100
    g = torch.Generator().manual_seed(10)
    a = torch.randn(csr.num_rows, 4, generator=g)
    b = torch.randn(257, 4, generator=g)
    rows = torch.repeat_interleave(torch.arange(csr.num_rows), deg)
    c = csr.col.long()
    r64 = (a.double()[rows] * b.double()[c]).sum(-1, keepdim=True)
    r32 = torch.zeros(csr.nnz, 1)
    for d in range(4):
        r32 = r32 + (a[rows, d] * b[c, d]).unsqueeze(1)
    s = run(csr.to(DEV), a.to(DEV), b.to(DEV), 1)
    within("sweep[F=4]", "s", s, r64, r32)
    s64 = run(CSR(rp, csr.col.long(), 257).to(DEV), a.to(DEV), b.to(DEV), 1)
    assert torch.equal(s64, s)


@pytest.mark.parametrize("F,heads,same", [(64, 4, False), (172, 1, False), (64, 1, True)])
def test_autograd_op(F, heads, same):
    """``da`` and ``db`` of the op against the fp64 contract's gradients (``same``: one
    embedding on a square pattern, which takes the sum of both)."""
    from dgraph_amd.ops import edge_dot

    full = skewed_csr(torch.int32)
    csr = CSR(full.rowptr[:258].clone(), full.col[:int(full.rowptr[257])].clone(), 257) \
        if same else full
    a, b = inputs(F)
    a = b if same else a
    g = values("plain", csr.nnz, heads, 31)
    grads = {}
    for dt in (torch.float64, torch.float32):
        ar = a.to(dt).clone().requires_grad_()
        br = ar if same else b.to(dt).clone().requires_grad_()
        edge_dot_contract(csr.rowptr, csr.col, ar, br, heads, 0.5, None, dt).backward(g.to(dt))
        grads[dt] = (ar.grad, br.grad)
    ad = a.to(DEV).requires_grad_()
    bd = ad if same else b.to(DEV).requires_grad_()
    s = edge_dot(ad, bd, csr.to(DEV), heads=heads, scale=0.5)
    s.backward(g.to(DEV))
    tag = f"op[F={F},H={heads}{',a is b' if same else ''}]"
    within(tag, "da", ad.grad, grads[torch.float64][0], grads[torch.float32][0])
    if not same:
        within(tag, "db", bd.grad, grads[torch.float64][1], grads[torch.float32][1])


@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_aggregate_edge_weight_gradient(reduce):
    csr = skewed_csr(torch.int32)
    F, H = 64, 2
    x, g = values("plain", 257, F, 41), values("plain", 300, F, 42)
    w = values("plain", csr.nnz, H, 43)
    rs = csr.inv_degree() if reduce == "mean" else None
    r64 = edge_dot_contract(csr.rowptr, csr.col, g, x, H, 1.0, rs)
    r32 = edge_dot_contract(csr.rowptr, csr.col, g, x, H, 1.0, rs, dtype=torch.float32)
    wd = w.to(DEV).requires_grad_()
    aggregate(x.to(DEV), csr.to(DEV), edge_weight=wd, reduce=reduce, heads=H).backward(g.to(DEV))
    within(f"aggregate[{reduce}]", "dw", wd.grad, r64, r32)


def test_aggregate_backward_holds_no_per_edge_feature_tensor():
    """F = 128, two heads, weights (and x) requiring grad: across the second backward (the
    first builds the cached transpose) the peak of allocated memory rises by less than one
    ``[nnz, F]`` fp32 tensor, and by less than a third of it: the path's own allocations are
    ``[nnz, heads]`` arrays and one ``[257, F]``."""
    csr = skewed_csr(torch.int32).to(DEV)
    F, H = 128, 2
    x = values("plain", 257, F, 51).to(DEV).requires_grad_()
    w = values("plain", csr.nnz, H, 52).to(DEV).requires_grad_()
    g = values("plain", 300, F, 53).to(DEV)
    aggregate(x, csr, edge_weight=w, heads=H).backward(g)
    x.grad = w.grad = None
    out = aggregate(x, csr, edge_weight=w, heads=H)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out.backward(g)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    edge_tensor = csr.nnz * F * 4
    print(f"backward peak rise {rise} B, one [nnz, F] tensor {edge_tensor} B")
    assert w.grad is not None and x.grad is not None
    assert rise < edge_tensor
    assert rise < edge_tensor / 3


def test_binding_checks():
    csr = skewed_csr(torch.int32).to(DEV)
    a, b = (t.to(DEV) for t in inputs(64))

    def call(a_, b_, heads=4, out=None, rs=None):
        return K.edge_dot(csr.rowptr, csr.col, a_, b_, out, heads=heads, row_scale=rs)

    flat = torch.zeros(300 * 64 + 4, device=DEV)
    off = flat[1:1 + 300 * 64].view(300, 64)  # base 4 B past a 16-B boundary
    off.copy_(a)
    with pytest.raises(RuntimeError, match="aligned"):
        call(off, b)
    with pytest.raises(RuntimeError, match="aligned"):
        call(a, torch.zeros(257, 66, device=DEV)[:, :64])  # row stride 66
    with pytest.raises(RuntimeError, match="column stride"):
        call(a, torch.zeros(64, 257, device=DEV).t())
    with pytest.raises(RuntimeError, match="float32 or bfloat16"):
        call(a.half(), b.half())
    with pytest.raises(RuntimeError, match="like a"):
        call(a, b.bfloat16())
    with pytest.raises(RuntimeError, match="out must be"):
        call(a, b, out=torch.zeros(csr.nnz, 4, device=DEV, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="out must be"):
        call(a, b, out=torch.zeros(csr.nnz, 2, device=DEV))
    with pytest.raises(RuntimeError, match="row_scale"):
        call(a, b, rs=torch.ones(299, device=DEV))
    with pytest.raises(RuntimeError, match="must have the CSR's"):
        call(a[:299], b)
    with pytest.raises(RuntimeError):
        call(a, b.cpu())  # wrong device
    with pytest.raises(RuntimeError):
        K.edge_dot(csr.rowptr.cpu(), csr.col, a, b, heads=4)
    # the generic path has no alignment contract: F = 172 (D / 4 = 43) off a 16-B boundary
    # and with an odd row stride is the same bits as the contiguous case
    a2, b2 = (t.to(DEV) for t in inputs(172))
    assert not K.edge_dot_vec_path(172, 1)
    flat = torch.zeros(300 * 173 + 4, device=DEV)
    odd = flat[1:1 + 300 * 173].view(300, 173)[:, :172]
    odd.copy_(a2)
    assert torch.equal(K.edge_dot(csr.rowptr, csr.col, odd, b2),
                       K.edge_dot(csr.rowptr, csr.col, a2, b2))
    # nothing to do: no launch, the shapes still come back
    empty = CSR(torch.zeros(301, dtype=torch.long), torch.zeros(0, dtype=torch.int32), 257).to(DEV)
    assert K.edge_dot(empty.rowptr, empty.col, a, b, heads=4).shape == (0, 4)
    z = K.edge_dot(csr.rowptr, csr.col, a[:, :0], b[:, :0])
    assert z.shape == (csr.nnz, 1) and torch.count_nonzero(z) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ decoder and loss
def test_decoder_loss_and_gradient():
    from dgraph_amd.models.link_pred import InnerProductDecoder, negative_pattern, recon_loss

    full = skewed_csr(torch.int32)
    pos = CSR(full.rowptr[:258].clone(), full.col[:int(full.rowptr[257])].clone(), 257)
    neg = negative_pattern(pos, 5, torch.Generator().manual_seed(61))
    z = 0.2 * values("plain", 257, 64, 62)
    res = {}
    for dt in (torch.float64, torch.float32):
        zr = z.to(dt).clone().requires_grad_()
        loss = zr.new_zeros(())
        for pat, target in ((pos, 1.0), (neg, 0.0)):
            s = edge_dot_contract(pat.rowptr, pat.col, zr, zr, 1, 1.0, None, dt)
            loss = loss + torch.nn.functional.binary_cross_entropy_with_logits(
                s, torch.full_like(s, target))
        loss.backward()
        res[dt] = (loss.detach().reshape(1), zr.grad)
    zd = z.to(DEV).requires_grad_()
    loss = recon_loss(zd, pos.to(DEV), neg.to(DEV), InnerProductDecoder())
    loss.backward()
    within("decoder", "loss", loss.reshape(1), res[torch.float64][0], res[torch.float32][0])
    within("decoder", "dz", zd.grad, res[torch.float64][1], res[torch.float32][1])


# ------------------------------------------------------------------ W = 2
def _tiny_shape():
    from dgraph_amd.data.synthetic import SHAPES

    return dataclasses.replace(SHAPES["ogbn-arxiv"], name="tiny-64", num_nodes=64,
                               num_directed_edges=400)


def _w2_body(rank, world):
    import test_edge_dot as D
    from dgraph_amd.comm.rccl_exec import RCCLExecutor
    from dgraph_amd.data.synthetic import build_partition
    from dgraph_amd.parallel.dist_graph import DistGraph

    shape = _tiny_shape()
    dev = rank_device()
    # the whole graph on the CPU in fp64 and fp32 (generated on the device like the ranks'
    # parts: the synthetic generator draws from the device's random stream)
    p = build_partition(shape, 0, 1, dev)
    csr1 = p["csr"].to("cpu")
    g1 = DistGraph(csr1, p["L"], 0)
    r1, c1 = csr1.row_ids(), csr1.col.long()
    graph, lo, grow, gcol = D.rank_graph(shape, rank, world, dev)
    sl = slice(lo, lo + graph.L)
    for same in (False, True):
        ref = {dt: D.run_dist(dt, g1, 0, r1, c1, "cpu", shape, same)
               for dt in (torch.float64, torch.float32)}
        s, da, db = D.run_dist(torch.float32, graph, lo, grow, gcol, dev, shape, same)
        tag = "W=2 a is b" if same else "W=2"
        within(tag, "s", s, D.expected_scores(torch.float64, grow, gcol, shape, same),
               D.expected_scores(torch.float32, grow, gcol, shape, same))
        within(tag, "da", da, ref[torch.float64][1][sl], ref[torch.float32][1][sl])
        within(tag, "db", db, ref[torch.float64][2][sl], ref[torch.float32][2][sl])
    torch.cuda.synchronize()
    RCCLExecutor.close_all()


def test_dist_edge_dot_two_ranks_rccl():
    """At W = 2 over real RCCL (both ranks on GPU 0, a 64-vertex graph): ``dist_edge_dot``
    scores, ``da`` and ``db`` against the single-rank op on the CPU in fp64, with two
    embeddings and with one."""
    run_ranks(_w2_body, 2, backend="rccl-one-gpu")
