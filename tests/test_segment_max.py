"""Max / min neighbourhood aggregation on the CPU reference path: the first-slot tie rule
against an explicit slot-order scan, the second-source (halo) rule, gradients, and the
error paths of the public surface."""
import pytest
import torch

from dgraph_amd.models.sage import GraphSAGE, SAGEConv
from dgraph_amd.ops import kernels as K
from dgraph_amd.ops.aggregate import aggregate
from dgraph_amd.ops.csr import CSR


def _tie_csr(seed=0, rows=64, cols=5, max_deg=40):
    g = torch.Generator().manual_seed(seed)
    deg = torch.randint(0, max_deg + 1, (rows,), generator=g)
    deg[3] = 0
    rowptr = torch.zeros(rows + 1, dtype=torch.long)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, cols, (int(rowptr[-1]),), generator=g, dtype=torch.int32)
    return CSR(rowptr, col, cols)


def _scan(csr, x, minimum, out=None, arg=None, second=False):
    """The contract, literally: scan each row's slots in order with a strict comparison."""
    R, F = csr.num_rows, x.shape[1]
    if out is None:
        out = torch.zeros(R, F, dtype=x.dtype)
        arg = torch.full((R, F), -1, dtype=torch.int32)
    for r in range(R):
        s, e = int(csr.rowptr[r]), int(csr.rowptr[r + 1])
        for f in range(F):
            for k in range(s, e):
                v = x[int(csr.col[k]), f]
                none = arg[r, f] == -1
                if none or (v < out[r, f] if minimum else v > out[r, f]):
                    out[r, f] = v
                    arg[r, f] = (-2 - (k - s)) if second else (k - s)
    return out, arg


@pytest.mark.parametrize("minimum", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
def test_reference_is_the_slot_order_scan(minimum, dtype):
    csr = _tie_csr()
    g = torch.Generator().manual_seed(1)
    x = torch.randint(-2, 3, (5, 6), generator=g).to(dtype)
    x[x == 0] = torch.tensor([0.0, -0.0]).to(dtype)[torch.arange(int((x == 0).sum())) % 2]
    out, arg = K.segment_extreme(csr.rowptr, csr.col, x, minimum=minimum)
    eo, ea = _scan(csr, x, minimum)
    assert arg.dtype == torch.int32
    assert torch.equal(arg, ea)
    assert torch.equal(out, eo)
    assert torch.all(out[3] == 0) and torch.all(arg[3] == -1)


@pytest.mark.parametrize("minimum", [False, True])
def test_second_source_replaces_only_when_strictly_better(minimum):
    a, b = _tie_csr(2, rows=40, max_deg=6), _tie_csr(3, rows=40, max_deg=6)
    g = torch.Generator().manual_seed(4)
    x = torch.randint(-2, 3, (5, 7), generator=g).float()
    h = torch.randint(-2, 3, (5, 7), generator=g).float()
    out, arg = K.segment_extreme(a.rowptr, a.col, x, minimum=minimum)
    bc = b.compact_rows()
    K.segment_extreme(bc.rowptr, bc.col, h, out, arg, minimum=minimum, second=True,
                      row_map=bc.row_map)
    eo, ea = _scan(a, x, minimum)
    # the halo scan against the interior incumbent: first strictly better halo slot wins
    eo2, ea2 = eo.clone(), ea.clone()
    for r in range(40):
        s, e = int(b.rowptr[r]), int(b.rowptr[r + 1])
        for f in range(7):
            for k in range(s, e):
                v = h[int(b.col[k]), f]
                if ea2[r, f] == -1 or (v < eo2[r, f] if minimum else v > eo2[r, f]):
                    eo2[r, f], ea2[r, f] = v, -2 - (k - s)
    assert torch.equal(out, eo2) and torch.equal(arg, ea2)
    assert (arg >= 0).any() and (arg <= -2).any() and (arg == -1).any()


@pytest.mark.parametrize("reduce", ["max", "min"])
def test_backward_routes_to_one_slot(reduce):
    """Ties and multi-edges: the whole of g[r, f] goes to the first winning slot's source;
    an integer g makes the sums exact, so a split or a double count shows."""
    csr = _tie_csr(5)
    g = torch.Generator().manual_seed(6)
    x = torch.randint(-2, 3, (5, 8), generator=g).float().requires_grad_()
    gy = torch.randint(-3, 4, (64, 8), generator=g).float()
    out = aggregate(x, csr, reduce=reduce)
    out.backward(gy)
    _, arg = _scan(csr, x.detach(), reduce == "min")
    exp = torch.zeros(5, 8)
    for r in range(64):
        for f in range(8):
            if arg[r, f] >= 0:
                exp[int(csr.col[int(csr.rowptr[r]) + int(arg[r, f])]), f] += gy[r, f]
    assert torch.equal(x.grad, exp)


def test_symmetric_pattern_uses_a_real_transpose():
    """``arg`` is not symmetric even when the pattern is: the backward must not take the
    symmetric CSR's transpose shortcut."""
    rows = torch.tensor([0, 0, 1, 1, 2, 2, 1, 3])
    cols = torch.tensor([1, 2, 0, 2, 0, 1, 3, 1])
    sym = CSR.from_coo(rows, cols, 4, 4)
    sym.symmetric = True
    plain = CSR.from_coo(rows, cols, 4, 4)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(4, 5, generator=g)
    gy = torch.randn(4, 5, generator=g)
    grads = []
    for c in (sym, plain):
        xi = x.clone().requires_grad_()
        aggregate(xi, c, reduce="max").backward(gy)
        grads.append(xi.grad)
    assert torch.equal(grads[0], grads[1])
    t, rel = sym.transpose_rel()
    assert t is not sym and rel.dtype == torch.int32
    assert sym.transpose_rel()[1] is rel  # cached


@pytest.mark.parametrize("reduce", ["max", "min"])
def test_gradcheck_fp64(reduce):
    g = torch.Generator().manual_seed(7)
    mask = torch.rand(20, 15, generator=g) < 0.3
    mask[4] = False  # an empty row
    r, c = torch.nonzero(mask, as_tuple=True)
    csr = CSR.from_coo(r, c, 20, 15)
    # a permutation of distinct values: no ties, so the function is differentiable here
    x = (torch.randperm(15 * 6, generator=g).double().reshape(15, 6) / 7.0 - 5.0)
    x.requires_grad_()
    assert torch.autograd.gradcheck(lambda t: aggregate(t, csr, reduce=reduce), (x,),
                                    eps=1e-6, atol=1e-6)


def test_zero_nnz_and_zero_rows():
    csr = CSR(torch.zeros(8, dtype=torch.long), torch.zeros(0, dtype=torch.int32), 0)
    x = torch.zeros(0, 4, requires_grad=True)
    out = aggregate(x, csr, reduce="max")
    assert out.shape == (7, 4) and torch.count_nonzero(out) == 0
    out.sum().backward()
    assert x.grad.shape == (0, 4)


def test_error_paths():
    csr = _tie_csr()
    x = torch.randn(5, 8)
    with pytest.raises(ValueError):
        aggregate(x, csr, edge_weight=torch.ones(csr.nnz), reduce="max")
    with pytest.raises(ValueError):
        aggregate(x, csr, reduce="max", heads=2)
    with pytest.raises(ValueError):
        aggregate(x, csr, reduce="median")
    with pytest.raises(ValueError):
        SAGEConv(8, 8, order="project_first", aggr="max")
    with pytest.raises(ValueError):
        GraphSAGE(8, 8, 4, 2, aggr="median")
    assert SAGEConv(8, 8).aggr == "mean"
