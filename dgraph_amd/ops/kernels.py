"""Functional entry points of the native op library (device dispatch).

GPU tensors -> hand-written HIP kernels in ``csrc/kernels`` (via ``torch.ops.dgraph_amd``);
CPU tensors -> :mod:`dgraph_amd.ops.reference`. There is no GPU fallback: a missing
native library raises (see :func:`dgraph_amd._native.ops`).

Native-kernel counterparts of the reference's ``torch_local`` module
(DGraph/distributed/csrc/torch_local_kernels.cu:28-254), generalised to bf16/fp32,
int32/int64 indices and wave64.
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import _native
from . import philox as _philox
from . import reference as _ref


def _native_ok(t: torch.Tensor) -> bool:
    return t.is_cuda


def _f32(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if t is None:
        return None
    if t.dtype != torch.float32 or not t.is_contiguous():
        t = t.float().contiguous()
    return t


def spmm(
    rowptr: torch.Tensor,
    col: torch.Tensor,
    x: torch.Tensor,
    out: Optional[torch.Tensor] = None,
    *,
    edge_weight: Optional[torch.Tensor] = None,
    col_scale: Optional[torch.Tensor] = None,
    row_scale: Optional[torch.Tensor] = None,
    heads: int = 1,
    beta: float = 0.0,
    split=None,
    row_map: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """CSR aggregation ``out[r] = row_scale[r]*sum_j w_j*col_scale[c_j]*x[c_j] + beta*out[r]``.

    ``split``: a :class:`~dgraph_amd.ops.csr.HubSplit` of this CSR (one head only): hub
    rows sum their first ``split.cap`` entries in the main pass and their tails in
    independent segment waves, added back in a fixed order (same result; no wave is held
    by a 10^5-degree row).

    ``row_map``: CSR row r is output row ``row_map[r]`` (a row-compacted CSR,
    :meth:`~dgraph_amd.ops.csr.CSR.compact_rows`); ``out`` must then be given."""
    R = rowptr.numel() - 1
    F = x.shape[1]
    if row_map is not None and out is None:
        raise ValueError("spmm: row_map needs an explicit out")
    if out is None:
        out = torch.empty(R, F, dtype=x.dtype, device=x.device)
        beta = 0.0
    heads = max(int(heads), 1)
    if split is not None and heads != 1:
        split = None
    cap = split.cap if split is not None else 0
    ew, cs, rs = _f32(edge_weight), _f32(col_scale), _f32(row_scale)
    if _native_ok(x):
        ops = _native.ops()
        ops.spmm(rowptr, col, ew, cs, rs, x, out, heads, F // heads, float(beta), cap,
                 row_map)
        if split is not None:
            part = torch.empty(split.num_segments, F, dtype=torch.float32, device=x.device)
            ops.spmm_hub_partials(split.seg_beg, split.seg_end, col, ew, cs, x, part)
            ops.spmm_hub_reduce(part, split.hub_seg_ptr, split.hub_rows, rs, out)
        return out
    if row_map is not None:
        rs_c = None if row_scale is None else row_scale[row_map]
        tmp = out[row_map] if beta != 0.0 else torch.empty(R, F, dtype=out.dtype,
                                                            device=out.device)
        _ref.spmm(rowptr, col, x, tmp, edge_weight, col_scale, rs_c, heads, beta, cap)
        out[row_map] = tmp
    else:
        _ref.spmm(rowptr, col, x, out, edge_weight, col_scale, row_scale, heads, beta, cap)
    if split is not None:
        pdt = torch.float64 if x.dtype == torch.float64 else torch.float32
        part = torch.empty(split.num_segments, F, dtype=pdt, device=x.device)
        _ref.spmm_hub_partials(split.seg_beg, split.seg_end, col, x, part, edge_weight,
                               col_scale)
        _ref.spmm_hub_reduce(part, split.hub_seg_ptr, split.hub_rows, out, row_scale)
    return out


def _seed_tensor(seed, device) -> torch.Tensor:
    """The DropEdge seed as ONE int64 on ``device`` (the kernels read it from memory)."""
    if isinstance(seed, torch.Tensor):
        if seed.numel() != 1 or seed.dtype != torch.int64:
            raise ValueError("seed must be a Python int or a 1-element int64 tensor")
        return seed if seed.device == device else seed.to(device)
    return torch.tensor([int(seed)], dtype=torch.int64, device=device)


def _drop_entries(rowptr, col, seed, p, undirected, transposed, row_map, row_ids, col_ids,
                  row_base, col_base):
    """``(out_rows [R], entry_rows [nnz], keep [nnz])`` of the DropEdge contract in torch:
    the output row of every CSR row and entry, and the keep decision of every entry."""
    R = rowptr.numel() - 1
    out_rows = row_map.long() if row_map is not None else torch.arange(R, device=col.device)
    rows = torch.repeat_interleave(out_rows, (rowptr[1:] - rowptr[:-1]).long())
    c = col.long()
    rid = row_ids[rows] if row_ids is not None else rows + int(row_base)
    cid = col_ids[c] if col_ids is not None else c + int(col_base)
    dst, src = (cid, rid) if transposed else (rid, cid)
    return out_rows, rows, _philox.edge_keep_mask(seed, dst, src, p, undirected)


def spmm_drop(
    rowptr: torch.Tensor,
    col: torch.Tensor,
    x: torch.Tensor,
    out: Optional[torch.Tensor] = None,
    *,
    seed,
    p: float,
    undirected: bool = False,
    transposed: bool = False,
    col_scale: Optional[torch.Tensor] = None,
    row_scale: Optional[torch.Tensor] = None,
    beta: float = 0.0,
    row_map: Optional[torch.Tensor] = None,
    row_ids: Optional[torch.Tensor] = None,
    col_ids: Optional[torch.Tensor] = None,
    row_base: int = 0,
    col_base: int = 0,
) -> torch.Tensor:
    """CSR aggregation over a random subgraph (DropEdge) drawn from ``seed``; no pattern is
    rebuilt and no mask stored. For CSR row ``r``, output row ``o = row_map[r]`` (or ``r``)::

        out[o] = row_scale[o] * sum_{k in row r, keep_k} col_scale[c_k] * x[c_k] + beta * out[o]
        keep_k = edge_keep_mask(seed, dst, src, p, undirected)        (ops/philox.py)
        rid = row_ids[o] (or row_base + o),  cid = col_ids[c_k] (or col_base + c_k)
        (dst, src) = (cid, rid) if transposed else (rid, cid)

    ``transposed`` says the CSR is the transposed pattern (rows are sources), which is the
    whole backward: ``dx = A_keep^T g`` with the same seed. The sum is over a subgraph: no
    ``1 / (1 - p)`` rescale. Parallel entries with equal ``(dst, src)`` share one fate.
    ``seed``: a Python int or a 1-element int64 tensor on ``x``'s device, which the kernel
    reads (a captured step draws a new subgraph per replay). ``row_map`` needs ``out``.

    GPU: fp32 rows with any row strides, fp32 accumulation in a fixed order (bitwise
    reproducible, equal for int32 / int64 ``col``); the row of a dropped entry is never
    loaded. Not supported: bf16 rows, edge weights, heads, hub splitting. CPU: the contract
    in torch (``index_add_`` over the kept entries) in ``x``'s dtype."""
    R, F = rowptr.numel() - 1, x.shape[1]
    if row_map is not None and out is None:
        raise ValueError("spmm_drop: row_map needs an explicit out")
    if out is None:
        out = torch.empty(R, F, dtype=x.dtype, device=x.device)
        beta = 0.0
    seed = _seed_tensor(seed, x.device)
    if _native_ok(x):
        _native.ops().spmm_drop_f32(rowptr, col, x, out, seed, float(p), bool(undirected),
                                    bool(transposed), _f32(col_scale), _f32(row_scale),
                                    float(beta), row_map, row_ids, col_ids, int(row_base),
                                    int(col_base))
        return out
    out_rows, rows, keep = _drop_entries(rowptr, col, seed, p, undirected, transposed, row_map,
                                         row_ids, col_ids, row_base, col_base)
    ck = col.long()[keep]
    contrib = x[ck]
    if col_scale is not None:
        contrib = contrib * col_scale[ck].to(x.dtype)[:, None]
    agg = torch.zeros(out.shape[0], F, dtype=x.dtype, device=x.device)
    agg.index_add_(0, rows[keep], contrib)
    agg = agg[out_rows]
    if row_scale is not None:
        agg = agg * row_scale[out_rows].to(x.dtype)[:, None]
    if beta != 0.0:
        agg = agg + beta * out[out_rows].to(x.dtype)
    out[out_rows] = agg.to(out.dtype)
    return out


def kept_degree(
    rowptr: torch.Tensor,
    col: torch.Tensor,
    out: Optional[torch.Tensor] = None,
    *,
    seed,
    p: float,
    undirected: bool = False,
    transposed: bool = False,
    accumulate: bool = False,
    row_map: Optional[torch.Tensor] = None,
    row_ids: Optional[torch.Tensor] = None,
    col_ids: Optional[torch.Tensor] = None,
    num_cols: Optional[int] = None,
    row_base: int = 0,
    col_base: int = 0,
) -> torch.Tensor:
    """``kept[o]`` (int32) = the number of entries of CSR row ``r`` that :func:`spmm_drop`
    keeps with the same arguments (``+=`` with ``accumulate``: the second block of a
    two-source graph). An exact integer result; no feature traffic, no atomics. ``num_cols``:
    the number of source rows (what ``col_ids`` must cover); by default ``col_ids``'s length.
    ``row_map`` / ``accumulate`` need ``out``."""
    R = rowptr.numel() - 1
    if (row_map is not None or accumulate) and out is None:
        raise ValueError("kept_degree: row_map / accumulate need an explicit out")
    if out is None:
        out = torch.empty(R, dtype=torch.int32, device=col.device)
    seed = _seed_tensor(seed, col.device)
    if _native_ok(col):
        if num_cols is None:
            num_cols = col_ids.numel() if col_ids is not None else 0
        _native.ops().kept_degree(rowptr, col, out, seed, float(p), bool(undirected),
                                  bool(transposed), bool(accumulate), row_map, row_ids, col_ids,
                                  int(num_cols), int(row_base), int(col_base))
        return out
    out_rows, rows, keep = _drop_entries(rowptr, col, seed, p, undirected, transposed, row_map,
                                         row_ids, col_ids, row_base, col_base)
    cnt = torch.zeros(out.shape[0], dtype=torch.int64, device=col.device)
    cnt.index_add_(0, rows[keep], torch.ones_like(rows[keep]))
    cnt = cnt[out_rows].to(torch.int32)
    out[out_rows] = out[out_rows] + cnt if accumulate else cnt
    return out


def edge_dot(
    rowptr: torch.Tensor,
    col: torch.Tensor,
    a: torch.Tensor,
    b: torch.Tensor,
    out: Optional[torch.Tensor] = None,
    *,
    heads: int = 1,
    scale: float = 1.0,
    row_scale: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Per-edge dot products (SDDMM): ``out[k, h] = scale * row_scale[r(k)] *
    <a[r(k), h-slice], b[col[k], h-slice]>`` for every CSR slot ``k``, ``r(k)`` the row that
    holds it; ``[nnz, heads]``. GPU: ``a`` / ``b`` fp32 or bf16 (the same), each with its own
    row stride (column halves of one buffer are fine), ``out`` contiguous fp32, fp32
    accumulation in a fixed order (bitwise reproducible, equal for int32 / int64 ``col``); a
    head width that takes the vector path (:func:`edge_dot_vec_path`) needs bases aligned to
    4 elements and row strides divisible by 4. CPU: the composed expression, in ``a``'s
    dtype (fp64 stays fp64, anything else is computed in fp32)."""
    heads = int(heads)
    nnz, F = col.numel(), a.shape[1]
    if heads < 1 or F % heads != 0:
        raise ValueError(f"edge_dot: heads={heads} must divide the width {F}")
    if _native_ok(a):
        if out is None:
            out = torch.empty(nnz, heads, dtype=torch.float32, device=a.device)
        if F == 0:
            return out.zero_()
        _native.ops().edge_dot(rowptr, col, a, b, out, heads, float(scale), _f32(row_scale))
        return out
    return _ref.edge_dot(rowptr, col, a, b, out, heads, scale, row_scale)


def edge_dot_vec_path(F: int, heads: int) -> bool:
    """True when the native :func:`edge_dot` runs ``(F, heads)`` on its 4-elements-per-lane
    path (``D = F / heads`` a multiple of 4, ``D / 4`` a power of two, ``D <= 1024``), which
    has the alignment contract; every other shape runs the element-per-lane path."""
    return bool(_native.ops().edge_dot_vec_path(int(F), int(heads)))


def edge_dot_sweep_slots(F: int, heads: int) -> int:
    """The CSR slots one sweep of the native :func:`edge_dot` launch covers at its grid cap
    (cap workgroups x 4 waves x the slots a wave takes at a time); a pattern with more has
    waves that take a second chunk."""
    ops = _native.ops()
    return int(ops.edge_dot_grid_cap()) * 4 * int(ops.edge_dot_chunk_slots(int(F), int(heads)))


def segment_extreme(
    rowptr: torch.Tensor,
    col: torch.Tensor,
    x: torch.Tensor,
    out: Optional[torch.Tensor] = None,
    arg: Optional[torch.Tensor] = None,
    *,
    minimum: bool = False,
    second: bool = False,
    row_map: Optional[torch.Tensor] = None,
):
    """Segment max (``minimum``: min) over the CSR rows with the winning slot:
    ``out[r, f] = max_k x[col[k], f]`` (0 for an empty row) and ``arg[r, f]`` (int32) = the
    offset within row ``r`` of the FIRST slot that attains it (-1 for an empty row).

    ``second``: ``out`` / ``arg`` hold the result of an earlier pass over another source
    (the interior block); an entry of this pass replaces it only where strictly better, and
    is recorded as ``-2 - offset``. ``row_map`` as in :func:`spmm`. Returns ``(out, arg)``."""
    R = rowptr.numel() - 1
    F = x.shape[1]
    if (second or row_map is not None) and (out is None or arg is None):
        raise ValueError("segment_extreme: second / row_map need explicit out and arg")
    if out is None:
        out = torch.empty(R, F, dtype=x.dtype, device=x.device)
    if arg is None:
        arg = torch.empty(out.shape[0], F, dtype=torch.int32, device=x.device)
    if _native_ok(x):
        _native.ops().segment_extreme_fwd(rowptr, col, x, out, arg, bool(minimum),
                                          bool(second), row_map)
        return out, arg
    return _ref.segment_extreme(rowptr, col, x, out, arg, minimum, second, row_map)


def segment_extreme_bwd(
    t_rowptr: torch.Tensor,
    t_col: torch.Tensor,
    rel: torch.Tensor,
    g: torch.Tensor,
    arg: torch.Tensor,
    out: Optional[torch.Tensor] = None,
    *,
    halo: bool = False,
    beta: float = 0.0,
) -> torch.Tensor:
    """Backward of :func:`segment_extreme` as a gather over the transposed pattern
    (``t_rowptr`` / ``t_col``: rows = source rows, columns = destination rows; ``rel[k]``:
    entry k's offset within its destination row, :meth:`CSR.transpose_rel`):
    ``out[c] = beta * out[c] + sum_k g[t_col[k]] * [arg[t_col[k]] == rel[k]]``
    (``halo``: ``== -2 - rel[k]``). No atomics; fixed summation order."""
    C = t_rowptr.numel() - 1
    if out is None:
        out = torch.empty(C, g.shape[1], dtype=g.dtype, device=g.device)
        beta = 0.0
    if _native_ok(g):
        _native.ops().segment_extreme_bwd(t_rowptr, t_col, rel, g, arg, out, bool(halo),
                                          float(beta))
        return out
    return _ref.segment_extreme_bwd(t_rowptr, t_col, rel, g, arg, out, halo, beta)


def segment_pna(
    rowptr: torch.Tensor,
    col: torch.Tensor,
    x: torch.Tensor,
    *,
    mean: Optional[torch.Tensor] = None,
    sdev: Optional[torch.Tensor] = None,
    vmax: Optional[torch.Tensor] = None,
    amax: Optional[torch.Tensor] = None,
    vmin: Optional[torch.Tensor] = None,
    amin: Optional[torch.Tensor] = None,
    eps: float = 1e-5,
    second: bool = False,
    final: bool = True,
    prev_rowptr: Optional[torch.Tensor] = None,
    row_map: Optional[torch.Tensor] = None,
) -> None:
    """Mean, standard deviation, max and min of each CSR row's entries in ONE pass over the
    neighbour rows, written into the given outputs (each ``[rows, F]`` with its own row
    stride: normally the column blocks of one ``[rows, A*F]`` buffer). With
    ``n = max(entries, 1)``: ``mean = sum x / n``,
    ``sdev = sqrt(max(sum (x - mean)^2, 0) / n + eps)`` (an empty row: 0 and ``sqrt(eps)``);
    ``vmax`` / ``amax`` and ``vmin`` / ``amin`` exactly as :func:`segment_extreme`. The three
    pairs are each optional.

    Two sources: the first pass runs with ``final=False`` (``sdev`` then holds the sum of
    squared deviations), the second with ``second=True`` and ``prev_rowptr`` = the first
    source's row pointer over the OUTPUT rows; it must visit every output row (no
    row-compacted block), since a pass finalises only the rows it visits. ``row_map`` as in
    :func:`spmm`."""
    if (mean is None) != (sdev is None) or (vmax is None) != (amax is None) \
            or (vmin is None) != (amin is None):
        raise ValueError("segment_pna: (mean, sdev), (vmax, amax), (vmin, amin) come in pairs")
    if second and mean is not None and prev_rowptr is None:
        raise ValueError("segment_pna: a second pass over the moments needs prev_rowptr")
    if _native_ok(x):
        _native.ops().segment_pna_fwd(rowptr, col, x, mean, sdev, vmax, amax, vmin, amin,
                                      float(eps), bool(second), bool(final), prev_rowptr,
                                      row_map)
        return
    _ref.segment_pna(rowptr, col, x, mean, sdev, vmax, amax, vmin, amin, eps, second, final,
                     prev_rowptr, row_map)


def segment_pna_bwd(
    t_rowptr: torch.Tensor,
    t_col: torch.Tensor,
    rel: torch.Tensor,
    x: torch.Tensor,
    inv_deg: Optional[torch.Tensor],
    out: Optional[torch.Tensor] = None,
    *,
    g_mean: Optional[torch.Tensor] = None,
    g_std: Optional[torch.Tensor] = None,
    mean: Optional[torch.Tensor] = None,
    sdev: Optional[torch.Tensor] = None,
    g_max: Optional[torch.Tensor] = None,
    amax: Optional[torch.Tensor] = None,
    g_min: Optional[torch.Tensor] = None,
    amin: Optional[torch.Tensor] = None,
    halo: bool = False,
    beta: float = 0.0,
) -> torch.Tensor:
    """Backward of :func:`segment_pna` as a gather over the transposed pattern (the triple
    of :func:`segment_extreme_bwd`); ``x`` holds this block's source rows, ``inv_deg[r]`` is
    ``1 / max(total entries of destination r, 1)``:
    ``out[c] = beta * out[c] + sum_k inv_deg[r] (g_mean[r] + g_std[r] (x[c] - mean[r]) /
    sdev[r]) + g_max[r] [amax[r] == key_k] + g_min[r] [amin[r] == key_k]``, ``r = t_col[k]``,
    ``key_k = rel[k]`` (``halo``: ``-2 - rel[k]``). ``None`` gradients drop their terms. No
    atomics; fixed summation order."""
    C = t_rowptr.numel() - 1
    if out is None:
        out = torch.empty(C, x.shape[1], dtype=x.dtype, device=x.device)
        beta = 0.0
    if _native_ok(x):
        _native.ops().segment_pna_bwd(t_rowptr, t_col, rel, x, inv_deg, g_mean, g_std, mean,
                                      sdev, g_max, amax, g_min, amin, out, bool(halo),
                                      float(beta))
        return out
    return _ref.segment_pna_bwd(t_rowptr, t_col, rel, x, inv_deg, out, g_mean, g_std, mean,
                                sdev, g_max, amax, g_min, amin, halo, beta)


def temperature_rows(t, x: torch.Tensor, name: str) -> torch.Tensor:
    """The temperature as a contiguous ``[F]`` vector of ``x``'s dtype on its device (a
    float or a one-element tensor is expanded)."""
    F = x.shape[1]
    if not isinstance(t, torch.Tensor):
        return torch.full((F,), float(t), dtype=x.dtype, device=x.device)
    t = t.detach().to(device=x.device, dtype=x.dtype)
    if t.numel() == 1:
        return t.reshape(1).expand(F).contiguous()
    if t.dim() != 1 or t.numel() != F:
        raise ValueError(f"{name}: t must be a scalar or [{F}], got {tuple(t.shape)}")
    return t.contiguous()


def segment_softmax(
    rowptr: torch.Tensor,
    col: torch.Tensor,
    x: torch.Tensor,
    t,
    out: Optional[torch.Tensor] = None,
    lse: Optional[torch.Tensor] = None,
    *,
    second: bool = False,
    row_map: Optional[torch.Tensor] = None,
):
    """Softmax aggregation of each CSR row's entries in ONE pass over the neighbour rows:
    with ``s_k = t[f] * x[col[k], f]``, ``out[r, f] = sum_k softmax_k(s)_k x[col[k], f]`` and
    ``lse[r, f] = log sum_k exp(s_k)`` (0 and ``-inf`` for an empty row), about a running
    maximum (no overflow for any ``t x``). ``t``: ``[F]`` (a scalar is expanded), any sign.
    ``(out, lse)`` is the whole state: every weight is ``exp(t x[c] - lse[r])``.

    ``second``: ``out`` / ``lse`` hold the result of an earlier pass over another source (the
    interior block), which this pass starts from; a row without an entry here is left
    bitwise as it is. ``row_map`` as in :func:`spmm`. Returns ``(out, lse)``."""
    R = rowptr.numel() - 1
    F = x.shape[1]
    if (second or row_map is not None) and (out is None or lse is None):
        raise ValueError("segment_softmax: second / row_map need explicit out and lse")
    t = temperature_rows(t, x, "segment_softmax")
    if out is None:
        out = torch.empty(R, F, dtype=x.dtype, device=x.device)
    if lse is None:
        lse = torch.empty(out.shape[0], F, dtype=x.dtype, device=x.device)
    if _native_ok(x):
        _native.ops().segment_softmax_fwd(rowptr, col, x, t, out, lse, bool(second), row_map)
        return out, lse
    return _ref.segment_softmax(rowptr, col, x, t, out, lse, second, row_map)


def segment_softmax_bwd(
    t_rowptr: torch.Tensor,
    t_col: torch.Tensor,
    x: torch.Tensor,
    t,
    g: torch.Tensor,
    out_fwd: torch.Tensor,
    lse: torch.Tensor,
    out: Optional[torch.Tensor] = None,
    want_dt: bool = True,
    *,
    dt_partials: Optional[torch.Tensor] = None,
):
    """Backward of :func:`segment_softmax` as a gather over the transposed pattern
    (``t_rowptr`` / ``t_col``: rows = source rows of ``x``, columns = destination rows of
    ``g`` / ``out_fwd`` / ``lse``) of ANY subset of the entries, given the final
    ``(out_fwd, lse)``: per entry ``w = exp(t x[c] - lse[r])``, ``d = x[c] - out_fwd[r]``,
    ``dx[c] = sum_k w g[r] (1 + t d)`` and ``dt = sum_c sum_k w g[r] d^2``. ``dt`` comes as
    fixed-order partial rows ``[P, F]`` (one per workgroup; ``dt = partials.sum(0)``) in
    ``dt_partials`` when given (the GPU needs ``P = segment_softmax_dt_parts(rows)``), else
    a fresh buffer; ``want_dt=False`` skips it and touches no buffer. No atomics.
    Returns ``(dx, partials or None)``."""
    C = t_rowptr.numel() - 1
    F = x.shape[1]
    t = temperature_rows(t, x, "segment_softmax_bwd")
    if out is None:
        out = torch.empty(C, F, dtype=x.dtype, device=x.device)
    if _native_ok(x):
        ops = _native.ops()
        part = None
        if want_dt:
            part = dt_partials if dt_partials is not None else torch.empty(
                ops.segment_softmax_dt_parts(C), F, dtype=torch.float32, device=x.device)
        ops.segment_softmax_bwd(t_rowptr, t_col, x, t, g, out_fwd, lse, out, part)
        return out, part
    dx, part = _ref.segment_softmax_bwd(t_rowptr, t_col, x, t, g, out_fwd, lse, out, want_dt)
    if part is not None and dt_partials is not None:
        dt_partials.zero_()
        dt_partials[:1] = part.to(dt_partials.dtype)
        part = dt_partials
    return dx, part


def _check_gated_rows(name: str, F: int, ref: torch.Tensor, **arrays) -> None:
    """The operands of the gated aggregation: 2-D, ``F`` wide, of ``ref``'s dtype (fp32 on
    the GPU) on its device, unit column stride."""
    if ref.is_cuda and ref.dtype != torch.float32:
        raise ValueError(f"{name}: the GPU kernels are float32, got {ref.dtype}")
    for nm, a in arrays.items():
        if a is None:
            continue
        if a.dim() != 2 or a.shape[1] != F:
            raise ValueError(f"{name}: {nm} must be [rows, {F}], got {tuple(a.shape)}")
        if a.dtype != ref.dtype or a.device != ref.device:
            raise ValueError(f"{name}: {nm} must be {ref.dtype} on {ref.device}, got "
                             f"{a.dtype} on {a.device}")
        if F > 1 and a.shape[0] > 0 and a.stride(1) != 1:
            raise ValueError(f"{name}: {nm} must have unit column stride, got strides "
                             f"{a.stride()}")


def segment_gated(
    rowptr: torch.Tensor,
    col: torch.Tensor,
    k: torch.Tensor,
    q: torch.Tensor,
    v: torch.Tensor,
    out: Optional[torch.Tensor] = None,
    ds: Optional[torch.Tensor] = None,
    *,
    want_ds: bool = False,
    accumulate: bool = False,
):
    """Gated aggregation of each CSR row's entries in ONE pass over the neighbour rows: with
    ``s = sigmoid(k[r, f] + q[col[j], f])``, ``out[r, f] = sum_j s v[col[j], f]`` and, with
    ``want_ds`` or a ``ds`` buffer, ``ds[r, f] = sum_j s (1 - s) v[col[j], f]`` from the same
    pass (zeros for an empty row). ``ds`` is the whole saved state of the destination side:
    ``dk = g * ds``. ``k`` has the CSR's rows, ``q`` / ``v`` the rows its column ids index;
    every operand may be a column view of a wider buffer (its own row stride).

    ``accumulate``: ``out`` (and ``ds``) hold the result of an earlier pass over another
    source (the interior block), which this pass adds to; a row without an entry here is left
    bitwise as it is. Returns ``(out, ds)`` (``ds`` is ``None`` when not asked for)."""
    R = rowptr.numel() - 1
    F = k.shape[1]
    if accumulate and (out is None or (want_ds and ds is None)):
        raise ValueError("segment_gated: accumulate needs explicit out (and ds with want_ds)")
    if out is None:
        out = torch.empty(R, F, dtype=k.dtype, device=k.device)
    if ds is None and want_ds:
        ds = torch.empty(out.shape[0], F, dtype=k.dtype, device=k.device)
    _check_gated_rows("segment_gated", F, k, k=k, q=q, v=v, out=out, ds=ds)
    if q.shape[0] != v.shape[0]:
        raise ValueError("segment_gated: q and v must have the same row count, got "
                         f"{q.shape[0]} and {v.shape[0]}")
    if k.shape[0] < R or out.shape[0] < R or (ds is not None and ds.shape[0] < R):
        raise ValueError(f"segment_gated: k, out and ds need >= {R} rows")
    if _native_ok(k):
        _native.ops().segment_gated_fwd(rowptr, col, k, q, v, out, ds, bool(accumulate))
        return out, ds
    return _ref.segment_gated(rowptr, col, k, q, v, out, ds, accumulate)


def segment_gated_bwd_src(
    t_rowptr: torch.Tensor,
    t_col: torch.Tensor,
    k: torch.Tensor,
    q: torch.Tensor,
    v: torch.Tensor,
    g: torch.Tensor,
    dq: Optional[torch.Tensor] = None,
    dv: Optional[torch.Tensor] = None,
):
    """Source side of the backward of :func:`segment_gated` as a gather over the transposed
    pattern (``t_rowptr`` / ``t_col``: rows = source rows of ``q`` / ``v``, columns =
    destination rows of ``k`` / ``g``) of ANY subset of the entries: per entry ``s =
    sigmoid(k[r] + q[c])``, ``dv[c] = sum s g[r]`` and ``dq[c] = v[c] sum s (1 - s) g[r]``.
    Every source row is written (zeros for one nobody reads). ``dq`` / ``dv`` may be the
    halves of one ``[C, 2F]`` buffer. No atomics. Returns ``(dq, dv)``."""
    C = t_rowptr.numel() - 1
    F = q.shape[1]
    if dq is None:
        dq = torch.empty(C, F, dtype=q.dtype, device=q.device)
    if dv is None:
        dv = torch.empty(C, F, dtype=q.dtype, device=q.device)
    _check_gated_rows("segment_gated_bwd_src", F, q, k=k, q=q, v=v, g=g, dq=dq, dv=dv)
    if min(q.shape[0], v.shape[0], dq.shape[0], dv.shape[0]) < C:
        raise ValueError(f"segment_gated_bwd_src: q, v, dq and dv need >= {C} rows")
    if k.shape[0] < g.shape[0]:
        raise ValueError("segment_gated_bwd_src: k has fewer rows than g "
                         f"({k.shape[0]} < {g.shape[0]})")
    if _native_ok(q):
        _native.ops().segment_gated_bwd_src(t_rowptr, t_col, k, q, v, g, dq, dv)
        return dq, dv
    return _ref.segment_gated_bwd_src(t_rowptr, t_col, k, q, v, g, dq, dv)


def _check_edge_rows(name: str, x: torch.Tensor, e: torch.Tensor, col: torch.Tensor) -> None:
    """The edge rows of :func:`segment_softmax_edge`: ``[nnz, F]`` of ``x``'s dtype (fp32 on
    the GPU) on its device, unit column stride."""
    F = x.shape[1]
    if x.dim() != 2 or e.dim() != 2 or tuple(e.shape) != (col.numel(), F):
        raise ValueError(f"{name}: e must be [{col.numel()}, {F}] (one row per CSR slot), got "
                         f"{tuple(e.shape)}")
    if e.dtype != x.dtype or e.device != x.device:
        raise ValueError(f"{name}: e must be {x.dtype} on {x.device}, got {e.dtype} on "
                         f"{e.device}")
    if x.is_cuda and x.dtype != torch.float32:
        raise ValueError(f"{name}: the GPU kernels are float32, got {x.dtype}")
    for nm, v in (("x", x), ("e", e)):
        if F > 1 and v.shape[0] > 0 and v.stride(1) != 1:
            raise ValueError(f"{name}: {nm} must have unit column stride, got strides "
                             f"{v.stride()}")


def segment_softmax_edge_dt_parts(rows: int) -> int:
    """The number of ``dt`` partial rows the GPU backward of :func:`segment_softmax_edge`
    writes for a pattern of ``rows`` rows."""
    return int(_native.ops().segment_softmax_edge_dt_parts(int(rows)))


def segment_softmax_edge(
    rowptr: torch.Tensor,
    col: torch.Tensor,
    x: torch.Tensor,
    e: torch.Tensor,
    t,
    out: Optional[torch.Tensor] = None,
    lse: Optional[torch.Tensor] = None,
    *,
    relu: bool = True,
    eps: float = 1e-7,
    second: bool = False,
    row_map: Optional[torch.Tensor] = None,
):
    """Softmax aggregation of messages formed per edge, in ONE pass over the neighbour and
    edge rows: for CSR slot ``k`` of row ``r``, ``z = x[col[k]] + e[k]`` and ``m_k = (relu ?
    max(z, 0) : z) + eps`` (GENConv's message with edge features); ``out[r, f] = sum_k
    softmax_k(t_f m_k) m_k`` and ``lse[r, f] = log sum_k exp(t_f m_k)`` (0 and ``-inf`` for an
    empty row). ``e``: ``[nnz, F]``, one row per slot in slot order (its own row stride).
    ``t``, ``second`` and ``row_map`` as in :func:`segment_softmax`. ``(out, lse)`` is the
    whole state. Returns ``(out, lse)``."""
    name = "segment_softmax_edge"
    _check_edge_rows(name, x, e, col)
    R = rowptr.numel() - 1
    F = x.shape[1]
    if (second or row_map is not None) and (out is None or lse is None):
        raise ValueError(f"{name}: second / row_map need explicit out and lse")
    t = temperature_rows(t, x, name)
    if out is None:
        out = torch.empty(R, F, dtype=x.dtype, device=x.device)
    if lse is None:
        lse = torch.empty(out.shape[0], F, dtype=x.dtype, device=x.device)
    if row_map is None and (out.shape[0] < R or lse.shape[0] < R):
        raise ValueError(f"{name}: out / lse need at least {R} rows, got {out.shape[0]} / "
                         f"{lse.shape[0]}")
    if _native_ok(x):
        _native.ops().segment_softmax_edge_fwd(rowptr, col, x, e, t, out, lse, bool(relu),
                                               float(eps), bool(second), row_map)
        return out, lse
    return _ref.segment_softmax_edge(rowptr, col, x, e, t, out, lse, bool(relu), float(eps),
                                     second, row_map)


def segment_softmax_edge_bwd(
    rowptr: torch.Tensor,
    col: torch.Tensor,
    x: torch.Tensor,
    e: torch.Tensor,
    t,
    g: torch.Tensor,
    out_fwd: torch.Tensor,
    lse: torch.Tensor,
    de: Optional[torch.Tensor] = None,
    *,
    relu: bool = True,
    eps: float = 1e-7,
    want_dt: bool = True,
    dt_partials: Optional[torch.Tensor] = None,
):
    """Destination-side backward of :func:`segment_softmax_edge`, over the SAME pattern (not
    the transposed one) of ANY block of the entries, given the final ``(out_fwd, lse)``
    (``g`` / ``out_fwd`` / ``lse`` indexed by the CSR row): per slot ``w = exp(t m - lse[r])``,
    ``d = m - out_fwd[r]``, ``de[k] = w g[r] (1 + t d)`` where ``not relu`` or ``z > 0``, else
    exactly 0 (``z == 0`` has gradient 0, as ``torch.relu``), and ``dt = sum_k w g[r] d^2``.
    Every slot's row of ``de`` (``[>= nnz, F]``, own row stride; fresh when ``None``) is
    written. ``dt`` comes as fixed-order partial rows ``[P, F]`` (``dt = partials.sum(0)``) in
    ``dt_partials`` when given (the GPU needs ``P = segment_softmax_edge_dt_parts(rows)``),
    else a fresh buffer; ``want_dt=False`` skips it and touches no buffer. The source side is
    a row sum of ``de``: ``dx = spmm(tt.rowptr, tt.perm, de)`` over the slot-transposed
    pattern ``tt``. No atomics. Returns ``(de, partials or None)``."""
    name = "segment_softmax_edge_bwd"
    _check_edge_rows(name, x, e, col)
    R = rowptr.numel() - 1
    F = x.shape[1]
    nnz = col.numel()
    t = temperature_rows(t, x, name)
    if de is None:
        de = torch.empty(nnz, F, dtype=x.dtype, device=x.device)
    if de.dim() != 2 or de.shape[0] < nnz or de.shape[1] != F:
        raise ValueError(f"{name}: de must be [>= {nnz}, {F}], got {tuple(de.shape)}")
    for nm, v in (("g", g), ("out_fwd", out_fwd), ("lse", lse)):
        if v.dim() != 2 or v.shape[0] < R or v.shape[1] != F:
            raise ValueError(f"{name}: {nm} must be [>= {R}, {F}], got {tuple(v.shape)}")
    if _native_ok(x):
        ops = _native.ops()
        part = None
        if want_dt:
            P = ops.segment_softmax_edge_dt_parts(R)
            part = dt_partials if dt_partials is not None else torch.empty(
                P, F, dtype=torch.float32, device=x.device)
            if tuple(part.shape) != (P, F):
                raise ValueError(f"{name}: dt_partials must be [{P}, {F}], got "
                                 f"{tuple(part.shape)}")
        ops.segment_softmax_edge_bwd(rowptr, col, x, e, t, g, out_fwd, lse, de, bool(relu),
                                     float(eps), part)
        return de, part
    de, part = _ref.segment_softmax_edge_bwd(rowptr, col, x, e, t, g, out_fwd, lse, de,
                                             bool(relu), float(eps), want_dt)
    if part is not None and dt_partials is not None:
        dt_partials.zero_()
        dt_partials[:1] = part.to(dt_partials.dtype)
        part = dt_partials
    return de, part


def copy_rows(
    x: torch.Tensor,
    src_idx: Optional[torch.Tensor] = None,
    dst_idx: Optional[torch.Tensor] = None,
    out: Optional[torch.Tensor] = None,
    *,
    num_out_rows: Optional[int] = None,
    accumulate: bool = False,
) -> torch.Tensor:
    """``out[dst[i]] (+)= x[src[i]]`` (identity when an index is None)."""
    if out is None:
        n = (src_idx.numel() if src_idx is not None else x.shape[0])
        rows = num_out_rows if num_out_rows is not None else n
        alloc = torch.zeros if (accumulate or dst_idx is not None) else torch.empty
        out = alloc(rows, x.shape[1], dtype=torch.float32 if accumulate else x.dtype,
                    device=x.device)
    if src_idx is not None and dst_idx is not None and src_idx.dtype != dst_idx.dtype:
        src_idx, dst_idx = src_idx.long(), dst_idx.long()
    if _native_ok(x):
        xin = x.float() if (accumulate and x.dtype != torch.float32) else x
        _native.ops().copy_rows(xin, src_idx, dst_idx, out, bool(accumulate))
        return out
    return _ref.copy_rows(x, src_idx, dst_idx, out, accumulate)


def gather_rows(x: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """``out[i] = x[idx[i]]`` (zeros where idx < 0)."""
    out = torch.empty(idx.numel(), x.shape[1], dtype=x.dtype, device=x.device)
    return copy_rows(x, src_idx=idx, out=out)


def masked_gather_rows(x, idx, mask, value, out):
    if _native_ok(x):
        _native.ops().masked_gather_rows(x, idx.long(), mask.long(), int(value), out)
        return out
    return _ref.masked_gather_rows(x, idx, mask, value, out)


def edge_softmax_fwd(rowptr: torch.Tensor, scores: torch.Tensor) -> torch.Tensor:
    if _native_ok(scores):
        s = scores.float().contiguous()
        alpha = torch.empty_like(s)
        _native.ops().edge_softmax_fwd(rowptr, s, alpha)
        return alpha
    return _ref.edge_softmax_fwd(rowptr, scores)


def edge_softmax_bwd(rowptr: torch.Tensor, alpha: torch.Tensor, grad: torch.Tensor) -> torch.Tensor:
    if _native_ok(alpha):
        a = alpha.float().contiguous()
        g = grad.float().contiguous()
        ds = torch.empty_like(a)
        _native.ops().edge_softmax_bwd(rowptr, a, g, ds)
        return ds
    return _ref.edge_softmax_bwd(rowptr, alpha, grad)


def mask_words(numel: int) -> int:
    """int32 words of a keep mask for ``numel`` elements (512-element chunks x 16)."""
    return (numel + 511) // 512 * 16


def col_sum(g: torch.Tensor) -> torch.Tensor:
    """fp32 column sums of a 2-D tensor (bias gradients), deterministic."""
    if _native_ok(g) and g.dim() == 2 and g.stride(1) == 1:
        vec = 4 if g.dtype == torch.float32 else 8
        if g.shape[1] % vec != 0 or g.stride(0) % vec != 0 or g.data_ptr() % 16 != 0:
            vec = 1  # scalar-lane kernel variant (odd width, or a misaligned column slice)
        if g.shape[1] // vec <= 256:
            return _native.ops().col_sum(g)
        return torch.sum(g, dim=0, dtype=torch.float32)
    return _ref.col_sum(g)


def row_scale_colsum(x: torch.Tensor, s: torch.Tensor, out: torch.Tensor,
                     partial: torch.Tensor) -> torch.Tensor:
    """:func:`row_scale_cols` (bf16) that also writes fp32 column sums of the UNSCALED
    ``x`` over a fixed row partition into ``partial [nblocks, w]`` (may be a column slice
    of a wider partials tensor); ``partial.sum(0)`` are the column sums. Native: one
    pass (elementwise.hip row_scale_colsum)."""
    if _native_ok(x):
        _native.ops().row_scale_colsum(x, _f32(s), out, partial)
        return out
    return _ref.row_scale_colsum(x, s, out, partial)


def row_scale_cols(x: torch.Tensor, s: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """``out[r, :] = x[r, :] * s[r]`` for a row-strided ``x`` (e.g. a column slice);
    fp32 ``s``. Native: one streaming pass with 16-B lanes (elementwise.hip)."""
    if _native_ok(x):
        _native.ops().row_scale_cols(x, _f32(s), out)
        return out
    return _ref.row_scale_cols(x, s, out)


def bias_relu_pack(y: torch.Tensor, bias: Optional[torch.Tensor] = None,
                   bits: Optional[torch.Tensor] = None, relu: bool = True) -> None:
    """In place ``y = act(y + bias)``; optional 1-bit keep mask (int32 words)."""
    if _native_ok(y):
        _native.ops().bias_relu_pack(y, _f32(bias), bits, bool(relu))
        return
    _ref.bias_relu_pack(y, bias, bits, relu)


def relu_mask_bwd(g: torch.Tensor, bits: torch.Tensor) -> None:
    """In place ``g = keep ? g : 0`` from a mask written by :func:`bias_relu_pack`."""
    if _native_ok(g):
        _native.ops().relu_mask_bwd(g, bits)
        return
    _ref.relu_mask_bwd(g, bits)


def pair_relu(rowptr: torch.Tensor, col: torch.Tensor, mode: int, rowterm: torch.Tensor,
              gat: torch.Tensor, gat2: Optional[torch.Tensor] = None,
              rowmul: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fused edge-MLP aggregation (edge_fused.hip). mode 0: ``sum_c relu(R[r]+X[c])``;
    1: ``M[r] * #{R[r]+X[c] > 0}``; 2: ``sum_c X2[c] [R[r]+X[c] > 0]``."""
    R = rowptr.numel() - 1
    if out is None:
        out = torch.empty(R, gat.shape[1], dtype=gat.dtype, device=gat.device)
    if _native_ok(gat):
        _native.ops().pair_relu(rowptr, col, int(mode), rowterm, gat, gat2, rowmul, out)
        return out
    return _ref.pair_relu(rowptr, col, mode, rowterm, gat, gat2, rowmul, out)


ACT_IDS = {None: 0, "none": 0, "identity": 0, "relu": 1, "silu": 2, "leaky_relu": 3}


def gather_add_act(E: int, F: int, *, Y=None, P=None, src=None, Q=None, dst=None, gin=None,
                   act="none", out: Optional[torch.Tensor] = None,
                   dtype=None, device=None) -> torch.Tensor:
    """``out[e] = act(Y[e] + P[src[e]] + Q[dst[e]])``; with ``gin``: ``gin[e] * act'(...)``."""
    ref = next(t for t in (Y, P, Q, gin, out) if t is not None)
    if out is None:
        out = torch.empty(E, F, dtype=dtype or ref.dtype, device=device or ref.device)
    a = ACT_IDS[act]
    if _native_ok(out):
        _native.ops().gather_add_act(Y, P, src, Q, dst, gin, out, a)
        return out
    return _ref.gather_add_act(Y, P, src, Q, dst, gin, out, a)
