"""fp32 row-group SpMM: the column-mapped variant that loads the row's self-term index at
the top of the row and its gate and self-term rows together (csrc/kernels/spmm_f32.hip, GS)
against an fp64 CPU reference and, bitwise, against the generic path of the same kernel. A
call with a ``row_map`` always takes the generic path, so the identity map gives the
generic result of the same call.

Shapes: every lane-group width (F = 64 / 128 / 256 in one pass, and in 64-column passes),
row counts that leave partial row groups (1, 3, 5, 1027), zero-degree rows, a row of degree
70 (crosses a chunk of 16 / 32 / 64 neighbours) and one of degree ~3000."""
import pytest
import torch

from dgraph_amd.ops import f32 as F32

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = dict(atol=2e-5, rtol=1e-5)  # the f32 SpMM tests' tolerance (test_f32_kernels_gpu.py)
NCOL = 1500


def _degrees(n, g):
    deg = torch.poisson(torch.full((n,), 9.0), generator=g).long()
    special = [0, 70, 3000] if n >= 3 else [70]
    deg[:len(special)] = torch.tensor(special)
    if n > 4:
        deg[3] = 0
        deg[n - 1] = 0
    return deg


def _csr(n, seed):
    g = torch.Generator().manual_seed(seed)
    deg = _degrees(n, g)
    rp = torch.zeros(n + 1, dtype=torch.long)
    rp[1:] = torch.cumsum(deg, 0)
    col = torch.randint(0, NCOL, (int(rp[-1]),), generator=g).to(torch.int32)
    return rp, col, g


def _run(rp, col, x, out0, n, **kw):
    """(fp64 CPU reference, device result, device result of the generic path)."""
    def dev(v):
        return v.to(DEV) if isinstance(v, torch.Tensor) else v

    ref = out0.double().clone()
    F32.spmm_f32(rp, col, x.double(), ref,
                 **{k: (v.double() if isinstance(v, torch.Tensor) and v.is_floating_point()
                        else v) for k, v in kw.items()})
    kd = {k: dev(v) for k, v in kw.items()}
    out = out0.to(DEV)
    F32.spmm_f32(rp.to(DEV), col.to(DEV), x.to(DEV), out, **kd)
    gen = out0.to(DEV)
    F32.spmm_f32(rp.to(DEV), col.to(DEV), x.to(DEV), gen,
                 row_map=torch.arange(n, device=DEV), **kd)
    return ref, out, gen


def _check(ref, out, gen):
    torch.testing.assert_close(out.double().cpu(), ref, **TOL)
    assert torch.equal(out, gen)


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("n", [1, 3, 5, 1027])
@pytest.mark.parametrize("F,pc", [(64, 64), (128, 128), (256, 64), (256, 256)])
def test_column_mapped_gate_self_term(F, pc, n, two):
    """The input-layer gradient pass: a column-mapped operand stored on ~30 % of the
    columns (u; small values, as a gradient: the degree-3000 row sums ~900 of them in
    fp32), the row's own term through ``self_map`` and the ReLU gate; ``two``: the mapped
    index splits over a second source. Alone and accumulating in place (beta = 1)."""
    rp, col, g = _csr(n, 300 + F + n)
    nk = int(NCOL * 0.3)
    keep = torch.randperm(NCOL, generator=g)[:nk].sort().values
    cmap = torch.full((NCOL,), -1, dtype=torch.int32)
    cmap[keep] = torch.arange(nk, dtype=torch.int32)
    u = torch.randn(nk, F, generator=g) * 0.02
    gate = torch.randn(n, F, generator=g)
    # the self term lives on a third of the output rows (of a larger row space: self_row0)
    row0 = 11
    n_self = max(1, n // 3)
    smap = torch.full((row0 + n,), -1, dtype=torch.int32)
    smap[row0 + torch.randperm(n, generator=g)[:n_self]] = torch.arange(n_self,
                                                                        dtype=torch.int32)
    v = torch.randn(n_self, F, generator=g)
    base = torch.randn(n, F, generator=g)
    kw = dict(col_map=cmap, gate=gate, self_add=v, self_map=smap, self_row0=row0,
              pass_cols=pc)
    if two:
        ns = nk // 2
        kw.update(x2=u[ns:].contiguous(), nsplit=ns)
        u = u[:ns].contiguous()
    _check(*_run(rp, col, u, base, n, **kw))
    _check(*_run(rp, col, u, base, n, beta=1.0, **kw))
    # over a row list (output row i <- CSR row rows[i]; gate, self term and row_scale are the
    # OUTPUT row's), scaled
    rows = torch.arange(n).flip(0).contiguous()
    rs = torch.rand(n, generator=g)
    _check(*_run(rp, col, u, base, n, row_ids=rows, row_scale=rs, **kw))
