"""The native segment max / min kernels (csrc/kernels/spmm_max.hip) and everything built on
them, against the CPU reference on the same inputs: the forward is a selection, so values
and winning slots must match exactly; backward sums are compared with an fp64 reference."""
import functools

import pytest
import torch

from conftest import rank_device, run_ranks
from dgraph_amd.ops import kernels as K
from dgraph_amd.ops.aggregate import aggregate
from dgraph_amd.ops.csr import CSR

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _rand_csr(R_, C, avg_deg, idx_dtype, skew=False, seed=0):
    """The recipe of tests/test_kernels_gpu.py (CPU tensors): Poisson degrees; with
    ``skew`` row 0 has 5,000 entries and the middle row none."""
    g = torch.Generator().manual_seed(seed)
    deg = torch.poisson(torch.full((R_,), float(avg_deg)), generator=g).long()
    if skew and R_ > 3:
        deg[0] = 5000
        deg[R_ // 2] = 0
    rowptr = torch.zeros(R_ + 1, dtype=torch.long)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, C, (int(rowptr[-1]),), generator=g)
    return CSR(rowptr, col.to(idx_dtype), C)


def _tol(dtype):
    return dict(atol=2e-2, rtol=2e-2) if dtype == torch.bfloat16 else dict(atol=1e-4, rtol=1e-4)


def _x(C, F, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(C, F, generator=g).to(dtype)


@functools.lru_cache(maxsize=None)
def _fwd_reference(F, dtype, minimum):
    """CPU reference of the skewed 300 x 257 case (shared by the index widths)."""
    csr = _rand_csr(300, 257, 7, torch.int64, skew=True, seed=F)
    return K.segment_extreme(csr.rowptr, csr.col, _x(257, F, dtype, F), minimum=minimum)


@pytest.mark.parametrize("F", [1, 3, 4, 8, 100, 128, 172, 256, 600])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("idx", [torch.int32, torch.int64])
@pytest.mark.parametrize("minimum", [False, True])
def test_forward_matches_reference(F, dtype, idx, minimum):
    csr = _rand_csr(300, 257, 7, idx, skew=True, seed=F).to(DEV)
    x = _x(257, F, dtype, F).to(DEV)
    out, arg = K.segment_extreme(csr.rowptr, csr.col, x, minimum=minimum)
    eo, ea = _fwd_reference(F, dtype, minimum)
    assert out.dtype == dtype and arg.dtype == torch.int32
    assert torch.equal(arg.cpu(), ea)
    assert torch.equal(out.cpu().float(), eo.float())  # bf16: after exact widening
    assert torch.count_nonzero(out[150]) == 0 and bool((arg[150] == -1).all())
    assert int(arg[0].max()) < 5000 and int(arg.min()) >= -1


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", ["max", "min", "max_all_negative", "min_all_positive"])
def test_ties_multi_edges_and_signs(case, dtype):
    """64 rows over 5 columns (every row repeats columns), small-integer values (ties
    everywhere): the first slot wins, and the gradient goes to it alone, once."""
    reduce = case[:3]
    g = torch.Generator().manual_seed(11)
    deg = torch.randint(0, 41, (64,), generator=g)
    rowptr = torch.zeros(65, dtype=torch.long)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, 5, (int(rowptr[-1]),), generator=g, dtype=torch.int32)
    csr = CSR(rowptr, col, 5)
    x = torch.randint(-2, 3, (5, 40), generator=g).float()
    if case == "max_all_negative":
        x = x - 3.0  # an accumulator initialised to 0 would win
    if case == "min_all_positive":
        x = x + 3.0
    x = x.to(dtype)
    gy = torch.randint(-3, 4, (64, 40), generator=g).to(dtype)  # integers: exact sums

    xc = x.clone().requires_grad_()
    eo = aggregate(xc, csr, reduce=reduce)
    eo.backward(gy)
    _, ea = K.segment_extreme(csr.rowptr, csr.col, x, minimum=reduce == "min")

    dcsr = csr.to(DEV)
    xd = x.to(DEV).requires_grad_()
    out, arg = K.segment_extreme(dcsr.rowptr, dcsr.col, xd.detach(), minimum=reduce == "min")
    assert torch.equal(arg.cpu(), ea)
    assert torch.equal(out.cpu().float(), eo.detach().float())
    aggregate(xd, dcsr, reduce=reduce).backward(gy.to(DEV))
    assert torch.equal(xd.grad.cpu().float(), xc.grad.float())


@pytest.mark.parametrize("F", [3, 64, 172, 600])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("idx", [torch.int32, torch.int64])
@pytest.mark.parametrize("reduce", ["max", "min"])
def test_backward_matches_fp64_reference(F, dtype, idx, reduce):
    csr = _rand_csr(300, 257, 7, idx, skew=True, seed=F)
    x = _x(257, F, dtype, F)
    gy = _x(300, F, dtype, F + 1000)
    xr = x.double().requires_grad_()  # widening is exact: same winners
    aggregate(xr, csr, reduce=reduce).backward(gy.double())
    xd = x.to(DEV).requires_grad_()
    aggregate(xd, csr.to(DEV), reduce=reduce).backward(gy.to(DEV))
    assert xd.grad.dtype == dtype
    torch.testing.assert_close(xd.grad.cpu().double(), xr.grad, **_tol(dtype))


def test_strided_input_and_empty_patterns():
    csr = _rand_csr(50, 40, 4, torch.int64, seed=1)
    big = _x(40, 48, torch.float32, 5)
    gy = _x(50, 32, torch.float32, 6)
    xr = big[:, 8:40].double().requires_grad_()
    er = aggregate(xr, csr, reduce="max")
    er.backward(gy.double())
    bigd = big.to(DEV).requires_grad_()
    xs = bigd[:, 8:40]  # row stride 48, feature stride 1
    out = aggregate(xs, csr.to(DEV), reduce="max")
    out.backward(gy.to(DEV))
    assert torch.equal(out.detach().cpu().double(), er.detach())
    torch.testing.assert_close(bigd.grad[:, 8:40].cpu().double(), xr.grad, atol=1e-4, rtol=1e-4)
    assert torch.count_nonzero(bigd.grad[:, :8]) == 0
    # all rows empty; then no columns at all (zero nnz and a 0-row x)
    empty = _rand_csr(50, 40, 0, torch.int32).to(DEV)
    out, arg = K.segment_extreme(empty.rowptr, empty.col, torch.randn(40, 32, device=DEV))
    assert torch.count_nonzero(out) == 0 and bool((arg == -1).all())
    none = CSR(torch.zeros(8, dtype=torch.long, device=DEV),
               torch.zeros(0, dtype=torch.int32, device=DEV), 0)
    x0 = torch.zeros(0, 16, device=DEV, requires_grad=True)
    o = aggregate(x0, none, reduce="min")
    o.sum().backward()
    assert o.shape == (7, 16) and torch.count_nonzero(o) == 0 and x0.grad.shape == (0, 16)


def _rank0_of_two(device):
    from dgraph_amd.data.synthetic import SHAPES, build_partition
    from dgraph_amd.parallel.dist_graph import DistGraph

    shape = SHAPES["ogbn-papers100M"].scaled(5e-5)
    part = build_partition(shape, 0, 2, device, global_frac=0.05, window=256, rehearse=True)
    g = DistGraph(part["csr"], part["L"], part["H"], part["send_local_idx"],
                  part["send_splits"], part["recv_splits"], None)
    return part, g


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_two_sources_match_the_unsplit_csr(dtype):
    """Interior pass + halo pass in second-source mode (row-compacted halo CSR) against one
    pass over the unsplit CSR with [x_local; halo_rows]; gradients against the reference."""
    part, g = _rank0_of_two(DEV)
    L, H, F = part["L"], part["H"], 72
    assert 1000 < L < 10000 and H > 0
    full = part["csr"]
    xa = _x(L + H, F, dtype, 2).to(DEV)
    gy = _x(L, F, dtype, 3).to(DEV)
    e0 = g.edges_aggregated
    out, arg = g.aggregate_extreme(xa[:L].contiguous(), halo_rows=xa[L:].contiguous())
    ref = aggregate(xa, full, reduce="max")
    assert torch.equal(out, ref)
    assert bool((arg >= 0).any()) and bool((arg <= -2).any())
    halo_out = torch.empty(H, F, dtype=dtype, device=DEV)
    gx = g.aggregate_extreme_T(gy, arg, halo_out=halo_out)
    assert g.edges_aggregated - e0 == 2 * g.nnz
    # reference: fp64 on the CPU over the unsplit CSR (random values: no ties between
    # distinct sources, so the slot order inside a row does not matter)
    xr = xa.cpu().double().requires_grad_()
    aggregate(xr, full.to("cpu"), reduce="max").backward(gy.cpu().double())
    torch.testing.assert_close(gx.cpu().double(), xr.grad[:L], **_tol(dtype))
    torch.testing.assert_close(halo_out.cpu().double(), xr.grad[L:], **_tol(dtype))


def test_second_source_rule_crafted():
    from dgraph_amd.parallel.dist_graph import DistGraph

    # 3 local rows, 2 halo rows (columns 3, 4). Row 0: interior and halo entries, the halo
    # value EQUALS the interior maximum; row 1: halo entries only; row 2: interior only.
    rows = torch.tensor([0, 0, 0, 1, 1, 2, 2])
    cols = torch.tensor([3, 1, 2, 4, 3, 0, 1])
    csr = CSR.from_coo(rows, cols, 3, 5).to(DEV)
    g = DistGraph(csr, 3, 2, torch.tensor([0, 1], dtype=torch.int32, device=DEV), [0, 2],
                  [0, 2], None)
    x = torch.tensor([[1.0, -4.0], [5.0, -1.0], [2.0, -3.0]], device=DEV)
    halo = torch.tensor([[5.0, -1.0], [7.0, -9.0]], device=DEV)
    out, arg = g.aggregate_extreme(x, halo_rows=halo)
    assert torch.equal(out.cpu(), torch.tensor([[5.0, -1.0], [7.0, -1.0], [5.0, -1.0]]))
    # row 0: interior slot 0 (column 1) keeps the tie; row 1: halo slots 0 / 1 of its halo
    # row; row 2: interior slot 1 (column 1)
    assert arg.cpu().tolist() == [[0, 0], [-2, -3], [1, 1]]
    gy = torch.tensor([[1.0, 2.0], [4.0, 8.0], [16.0, 32.0]], device=DEV)
    halo_out = torch.empty(2, 2, device=DEV)
    gx = g.aggregate_extreme_T(gy, arg, halo_out=halo_out)
    assert torch.equal(gx.cpu(), torch.tensor([[0.0, 0.0], [17.0, 34.0], [0.0, 0.0]]))
    assert torch.equal(halo_out.cpu(), torch.tensor([[0.0, 8.0], [4.0, 0.0]]))
    # minimum: row 0 keeps its interior winners, row 1 takes the halo's, row 2 the interior's
    out_min, arg_min = g.aggregate_extreme(x, minimum=True, halo_rows=halo)
    assert torch.equal(out_min.cpu(), torch.tensor([[2.0, -3.0], [5.0, -9.0], [1.0, -4.0]]))
    assert arg_min.cpu().tolist() == [[1, 1], [-3, -2], [0, 0]]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bitwise_deterministic(dtype):
    csr = _rand_csr(300, 257, 7, torch.int32, skew=True, seed=9).to(DEV)
    x = _x(257, 172, dtype, 9).to(DEV)
    gy = _x(300, 172, dtype, 10).to(DEV)
    res = []
    for _ in range(2):
        xi = x.clone().requires_grad_()
        out, arg = K.segment_extreme(csr.rowptr, csr.col, x)
        aggregate(xi, csr, reduce="max").backward(gy)
        res.append((out, arg, xi.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_graphsage_max_matches_cpu():
    """GraphSAGE(aggr="max") on the GPU against the same model on the CPU, at the
    tolerances of tests/test_sage.py::test_stack_matches_dense."""
    from dgraph_amd.data.synthetic import SHAPES, build_partition, node_data
    from dgraph_amd.models.sage import GraphSAGE
    from dgraph_amd.parallel.dist_graph import DistGraph

    shape = SHAPES["ogbn-arxiv"].scaled(0.01)
    p = build_partition(shape, 0, 1, "cpu")
    x, _, _ = node_data(shape, 0, p["offsets"], "cpu", dtype=torch.float32)
    torch.manual_seed(0)
    m = GraphSAGE(shape.num_features, 32, shape.num_classes, 2, aggr="max")
    res = {}
    for dev in ("cpu", DEV):
        md = m.to(dev)
        md.zero_grad()
        g = DistGraph(p["csr"].to(dev), p["L"], 0, symmetric=True)
        out = md(x.to(dev), g)
        out.square().mean().backward()
        res[dev] = (out.detach().cpu(), [q.grad.detach().cpu().clone() for q in md.parameters()])
    torch.testing.assert_close(res[DEV][0], res["cpu"][0], atol=1e-5, rtol=1e-4)
    for a, b in zip(res[DEV][1], res["cpu"][1]):
        torch.testing.assert_close(a, b, atol=1e-6, rtol=1e-4)


def _w2_body(rank, world):
    import test_segment_max_dist as D

    from dgraph_amd.comm.rccl_exec import RCCLExecutor

    D._dist_max_body(rank, world, rank_device())
    torch.cuda.synchronize()
    RCCLExecutor.close_all()


def test_dist_max_two_ranks_rccl():
    """dist_aggregate(reduce="max") forward and backward at W = 2 over real RCCL (both
    ranks on GPU 0) against the W = 1 result."""
    run_ranks(_w2_body, 2, backend="rccl-one-gpu")
