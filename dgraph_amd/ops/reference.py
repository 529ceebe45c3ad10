"""Pure-PyTorch fp32 reference implementations of the native ops.

Used (a) for CPU tensors, so the whole framework runs and is tested without a GPU, and
(b) as the numerics oracle the HIP kernels are compared against in ``tests/``.
Semantics match :mod:`dgraph_amd.ops.kernels` exactly (see csrc/kernels/kernels.h).
"""
from __future__ import annotations

from typing import Optional

import torch


def _row_ids(rowptr: torch.Tensor) -> torch.Tensor:
    deg = rowptr[1:] - rowptr[:-1]
    return torch.repeat_interleave(torch.arange(deg.numel(), device=rowptr.device), deg)


def spmm(
    rowptr: torch.Tensor,
    col: torch.Tensor,
    x: torch.Tensor,
    out: torch.Tensor,
    edge_weight: Optional[torch.Tensor] = None,
    col_scale: Optional[torch.Tensor] = None,
    row_scale: Optional[torch.Tensor] = None,
    heads: int = 1,
    beta: float = 0.0,
    cap: int = 0,
) -> torch.Tensor:
    """``cap > 0``: every row sums only its first ``cap`` entries (hub-split main pass)."""
    R = rowptr.numel() - 1
    F = x.shape[1]
    col = col.long()
    rows = _row_ids(rowptr)
    keep = None
    if cap > 0 and col.numel() > 0:
        slot = torch.arange(col.numel(), device=col.device) - rowptr[:-1].long()[rows]
        keep = slot < cap
        col, rows = col[keep], rows[keep]
        if edge_weight is not None:
            edge_weight = edge_weight.reshape(keep.numel(), -1)[keep]
    adt = torch.float64 if x.dtype == torch.float64 else torch.float32
    vals = x.to(adt)[col]
    if edge_weight is not None:
        w = edge_weight.to(adt).reshape(col.numel(), max(heads, 1))
        hd = F // max(heads, 1)
        vals = (vals.view(-1, max(heads, 1), hd) * w.unsqueeze(-1)).view(-1, F)
    if col_scale is not None:
        vals = vals * col_scale.to(adt)[col].unsqueeze(1)
    acc = torch.zeros(R, F, dtype=adt, device=x.device)
    acc.index_add_(0, rows, vals)
    if row_scale is not None:
        acc = acc * row_scale.to(adt).unsqueeze(1)
    if beta != 0.0:
        acc = acc + beta * out[:R].to(adt)
    out[:R].copy_(acc.to(out.dtype))
    return out


def edge_dot(rowptr, col, a, b, out=None, heads: int = 1, scale: float = 1.0,
             row_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out[k, h] = scale * row_scale[r(k)] * <a[r(k), h-slice], b[col[k], h-slice]>`` per
    CSR slot as two row gathers and a product (two ``[nnz, F]`` temporaries); fp64 for fp64
    inputs, else fp32. The edge-weight gradient of :func:`spmm`."""
    H = max(int(heads), 1)
    nnz = col.numel()
    cdt = torch.float64 if a.dtype == torch.float64 else torch.float32
    rows = _row_ids(rowptr)
    ar = a.to(cdt)[rows].view(nnz, H, a.shape[1] // H)
    bc = b.to(cdt)[col.long()].view(nnz, H, a.shape[1] // H)
    s = (ar * bc).sum(-1)
    if row_scale is not None:
        s = s * row_scale[rows].unsqueeze(1)
    if scale != 1.0:
        s = s * scale
    if out is None:
        return s
    out.copy_(s.to(out.dtype))
    return out


def spmm_hub_partials(seg_beg, seg_end, col, x, partials, edge_weight=None, col_scale=None):
    """fp32 sums of the hub-tail segments ``col[seg_beg[i]:seg_end[i]]`` (cf. kernels.h;
    fp64 for fp64 inputs, so gradcheck sees the split path at full precision)."""
    cdt = torch.float64 if x.dtype == torch.float64 else torch.float32
    lens = seg_end - seg_beg
    S = seg_beg.numel()
    if S == 0:
        return partials
    seg = torch.repeat_interleave(torch.arange(S, device=col.device), lens)
    off = torch.zeros(S + 1, dtype=torch.long, device=col.device)
    torch.cumsum(lens, 0, out=off[1:])
    pos = seg_beg[seg] + (torch.arange(seg.numel(), device=col.device) - off[:-1][seg])
    c = col.long()[pos]
    vals = x.to(cdt)[c]
    w = torch.ones(pos.numel(), dtype=cdt, device=col.device)
    if edge_weight is not None:
        w = w * edge_weight.reshape(-1).to(cdt)[pos]
    if col_scale is not None:
        w = w * col_scale.to(cdt)[c]
    acc = torch.zeros(S, x.shape[1], dtype=cdt, device=x.device)
    acc.index_add_(0, seg, vals * w.unsqueeze(1))
    partials[:S].copy_(acc)
    return partials


def spmm_hub_reduce(partials, hub_seg_ptr, hub_rows, out, row_scale=None):
    """``out[hub_rows[h]] += row_scale * sum of the hub's segment partials`` (in order)."""
    nh = hub_rows.numel()
    if nh == 0:
        return out
    cnt = hub_seg_ptr[1:] - hub_seg_ptr[:-1]
    cdt = torch.float64 if out.dtype == torch.float64 else torch.float32
    owner = torch.repeat_interleave(torch.arange(nh, device=out.device), cnt)
    acc = torch.zeros(nh, out.shape[1], dtype=cdt, device=out.device)
    acc.index_add_(0, owner, partials[: owner.numel()].to(cdt))
    if row_scale is not None:
        acc = acc * row_scale.to(cdt)[hub_rows].unsqueeze(1)
    out[hub_rows] = (out[hub_rows].to(cdt) + acc).to(out.dtype)
    return out


_NO_SLOT = 2**62


def segment_extreme(rowptr, col, x, out, arg, minimum=False, second=False, row_map=None):
    """Segment max (min) with the winning slot (cf. kernels.h). ``out[r, f]`` is the extremum
    of ``x[col[k], f]`` over row ``r``'s slots (0 for an empty row) and ``arg[r, f]`` the
    offset ``k - rowptr[r]`` of the FIRST slot attaining it (-1 for an empty row): a
    lexicographic (value, slot) reduction. ``second``: ``out`` / ``arg`` hold an incumbent,
    replaced only where this pass is strictly better (or there is none), recorded as
    ``-2 - offset``. ``row_map``: CSR row ``r`` is output row ``row_map[r]``."""
    R = rowptr.numel() - 1
    F = x.shape[1]
    if R <= 0 or F == 0:
        return out, arg
    dev = x.device
    cdt = torch.float64 if x.dtype == torch.float64 else torch.float32
    rows = _row_ids(rowptr)
    vals = x.to(cdt)[col.long()]  # widening is exact; the comparisons see the same order
    if minimum:
        vals = -vals
    idx = rows.unsqueeze(1).expand(-1, F)
    best = torch.full((R, F), float("-inf"), dtype=cdt, device=dev)
    best.scatter_reduce_(0, idx, vals, "amax", include_self=True)
    off = (torch.arange(rows.numel(), device=dev) - rowptr[:-1].long()[rows]).unsqueeze(1)
    cand = torch.where(vals == best[rows], off, _NO_SLOT)  # +0.0 == -0.0: a tie
    first = torch.full((R, F), _NO_SLOT, dtype=torch.long, device=dev)
    first.scatter_reduce_(0, idx, cand, "amin", include_self=True)
    has = first < _NO_SLOT
    tgt = slice(0, R) if row_map is None else row_map.long()
    if second:
        old = out[tgt].to(cdt)
        old_arg = arg[tgt]
        win = has & ((old_arg == -1) | (best > (-old if minimum else old)))
        new_out = torch.where(win, -best if minimum else best, old)
        new_arg = torch.where(win, -2 - first, old_arg.long())
    else:
        new_out = torch.where(has, -best if minimum else best, torch.zeros((), dtype=cdt))
        new_arg = torch.where(has, first, -1)
    out[tgt] = new_out.to(out.dtype)
    arg[tgt] = new_arg.to(arg.dtype)
    return out, arg


def segment_extreme_bwd(t_rowptr, t_col, rel, g, arg, out, halo=False, beta=0.0):
    """Backward of :func:`segment_extreme` over the transposed pattern: source row ``c``
    sums ``g[r, f]`` over its entries ``(r = t_col[k], rel[k])`` that ``arg[r, f]`` names
    (``-2 - rel[k]`` for the halo block). fp32 accumulate (fp64 for fp64)."""
    C = t_rowptr.numel() - 1
    if C <= 0 or g.shape[1] == 0:
        return out
    cdt = torch.float64 if g.dtype == torch.float64 else torch.float32
    src = _row_ids(t_rowptr)
    r = t_col.long()
    key = (-2 - rel.long()) if halo else rel.long()
    hit = arg[r].long() == key.unsqueeze(1)
    acc = torch.zeros(C, g.shape[1], dtype=cdt, device=g.device)
    acc.index_add_(0, src, torch.where(hit, g.to(cdt)[r], torch.zeros((), dtype=cdt)))
    if beta != 0.0:
        acc = acc + beta * out[:C].to(cdt)
    out[:C] = acc.to(out.dtype)
    return out


def segment_pna(rowptr, col, x, mean=None, sdev=None, vmax=None, amax=None, vmin=None,
                amin=None, eps=1e-5, second=False, final=True, prev_rowptr=None, row_map=None):
    """Fused mean / standard deviation / max / min of each CSR row's entries (cf. kernels.h),
    evaluated in two passes: the mean first, then the squared deviations about it. With
    ``n = max(entries of the row over all sources, 1)``: ``mean = sum x / n``,
    ``sdev = sqrt(max(sum (x - mean)^2, 0) / n + eps)``; the extremes are
    :func:`segment_extreme`. The pairs ``(mean, sdev)``, ``(vmax, amax)``, ``(vmin, amin)``
    are each optional. ``final=False`` leaves ``sdev`` = the sum of squared deviations M2;
    ``second``: the outputs hold such an incumbent of ``prev_rowptr``'s row counts, which
    this pass merges with its own ``(n, mean, M2)`` (the pairwise formula) and, with
    ``final``, finalises. fp32 (fp64 for fp64 input)."""
    R = rowptr.numel() - 1
    F = x.shape[1]
    if R <= 0 or F == 0:
        return
    for out, arg, minimum in ((vmax, amax, False), (vmin, amin, True)):
        if out is not None:
            segment_extreme(rowptr, col, x, out, arg, minimum, second, row_map)
    if mean is None:
        return
    cdt = torch.float64 if x.dtype == torch.float64 else torch.float32
    rows = _row_ids(rowptr)
    vals = x.to(cdt)[col.long()]
    nb = (rowptr[1:] - rowptr[:-1]).to(cdt).unsqueeze(1)
    mb = torch.zeros(R, F, dtype=cdt, device=x.device).index_add_(0, rows, vals)
    mb = mb / nb.clamp(min=1)
    qb = torch.zeros(R, F, dtype=cdt, device=x.device).index_add_(
        0, rows, (vals - mb[rows]).square())
    tgt = slice(0, R) if row_map is None else row_map.long()
    n = nb
    if second:
        na = (prev_rowptr[1:] - prev_rowptr[:-1])[tgt].to(cdt).unsqueeze(1)
        ma, qa = mean[tgt].to(cdt), sdev[tgt].to(cdt)
        n = na + nb
        w = nb / n.clamp(min=1)
        dl = mb - ma
        mb = ma + dl * w
        qb = qa + qb + dl * dl * (na * w)
    if final:
        qb = (qb.clamp(min=0) / n.clamp(min=1) + eps).sqrt()
    mean[tgt] = mb.to(mean.dtype)
    sdev[tgt] = qb.to(sdev.dtype)


def segment_pna_bwd(t_rowptr, t_col, rel, x, inv_deg, out, g_mean=None, g_std=None, mean=None,
                    sdev=None, g_max=None, amax=None, g_min=None, amin=None, halo=False,
                    beta=0.0):
    """Backward of :func:`segment_pna` over the transposed pattern (cf. kernels.h): source
    row ``c`` sums, over its entries ``(r = t_col[k], rel[k])``,
    ``inv_deg[r] (g_mean[r] + g_std[r] (x[c] - mean[r]) / sdev[r])`` and the ``g_max`` /
    ``g_min`` of the destinations whose ``amax`` / ``amin`` name the entry. ``None``
    gradients drop their terms. fp32 accumulate (fp64 for fp64)."""
    C = t_rowptr.numel() - 1
    F = out.shape[1]
    if C <= 0 or F == 0:
        return out
    cdt = torch.float64 if out.dtype == torch.float64 else torch.float32
    src = _row_ids(t_rowptr)
    r = t_col.long()
    key = ((-2 - rel.long()) if halo else rel.long()).unsqueeze(1)
    term = torch.zeros(r.numel(), F, dtype=cdt, device=out.device)
    if g_mean is not None or g_std is not None:
        b = torch.zeros_like(term)
        if g_mean is not None:
            b = b + g_mean.to(cdt)[r]
        if g_std is not None:
            b = b + g_std.to(cdt)[r] * ((x.to(cdt)[src] - mean.to(cdt)[r]) / sdev.to(cdt)[r])
        term = inv_deg.to(cdt)[r].unsqueeze(1) * b
    zero = torch.zeros((), dtype=cdt)
    for g, arg in ((g_max, amax), (g_min, amin)):
        if g is not None:
            term = term + torch.where(arg[r].long() == key, g.to(cdt)[r], zero)
    acc = torch.zeros(C, F, dtype=cdt, device=out.device).index_add_(0, src, term)
    if beta != 0.0:
        acc = acc + beta * out[:C].to(cdt)
    out[:C] = acc.to(out.dtype)
    return out


def segment_softmax(rowptr, col, x, t, out, lse, second=False, row_map=None):
    """Softmax aggregation of each CSR row's entries (cf. kernels.h): with ``s = t[f] *
    x[col[k], f]``, ``lse = log sum_k exp(s)`` (-inf for an empty row) and ``out = sum_k
    exp(s - lse) x[col[k]]`` (0 for an empty row), evaluated about the row maximum.
    ``second``: ``(out, lse)`` hold an incumbent, which enters as one more entry of value
    ``out`` and weight ``exp(lse)``; a row without an entry here keeps it bitwise. fp32
    (fp64 for fp64 input)."""
    R = rowptr.numel() - 1
    F = x.shape[1]
    if R <= 0 or F == 0:
        return out, lse
    cdt = torch.float64 if x.dtype == torch.float64 else torch.float32
    dev = x.device
    rows = _row_ids(rowptr)
    vals = x.to(cdt)[col.long()]
    s = vals * t.to(cdt)
    ninf = float("-inf")
    tgt = slice(0, R) if row_map is None else row_map.long()
    m = torch.full((R, F), ninf, dtype=cdt, device=dev)
    if second:
        m0, o0 = lse[tgt].to(cdt), out[tgt].to(cdt)
        m = m0.clone()
    m.scatter_reduce_(0, rows.unsqueeze(1).expand(-1, F), s, "amax", include_self=True)
    ms = torch.where(m == ninf, torch.zeros((), dtype=cdt, device=dev), m)  # empty rows
    w = torch.exp(s - ms[rows])
    l = torch.zeros(R, F, dtype=cdt, device=dev)
    acc = torch.zeros(R, F, dtype=cdt, device=dev)
    if second:  # the incumbent comes first
        k = torch.where(m0 == ninf, torch.zeros((), dtype=cdt, device=dev), torch.exp(m0 - ms))
        l += k
        acc += k * o0
    l.index_add_(0, rows, w)
    acc.index_add_(0, rows, w * vals)
    has = l > 0
    one = torch.ones((), dtype=cdt, device=dev)
    new_out = torch.where(has, acc / torch.where(has, l, one), torch.zeros((), dtype=cdt,
                                                                           device=dev))
    new_lse = torch.where(has, ms + torch.log(torch.where(has, l, one)),
                          torch.full((), ninf, dtype=cdt, device=dev))
    if second:
        visited = ((rowptr[1:] - rowptr[:-1]) > 0).unsqueeze(1)
        new_out = torch.where(visited, new_out, o0)
        new_lse = torch.where(visited, new_lse, m0)
    out[tgt] = new_out.to(out.dtype)
    lse[tgt] = new_lse.to(lse.dtype)
    return out, lse


def segment_softmax_bwd(t_rowptr, t_col, x, t, g, out_fwd, lse, dx, want_dt=True):
    """Backward of :func:`segment_softmax` over the transposed pattern of any subset of the
    entries, given the final ``(out_fwd, lse)`` (cf. kernels.h): per entry ``w = exp(t x[c] -
    lse[r])``, ``d = x[c] - out_fwd[r]``; ``dx[c] = sum w g[r] (1 + t d)`` and the one
    partial row ``sum w g[r] d^2`` of ``dt``. Returns ``(dx, [1, F] partials or None)``."""
    C = t_rowptr.numel() - 1
    F = dx.shape[1]
    cdt = torch.float64 if dx.dtype == torch.float64 else torch.float32
    part = torch.zeros(1, F, dtype=cdt, device=dx.device) if want_dt else None
    if C <= 0 or F == 0:
        return dx, part
    src = _row_ids(t_rowptr)
    r = t_col.long()
    tt = t.to(cdt)
    xs = x.to(cdt)[src]
    wg = torch.exp(tt * xs - lse.to(cdt)[r]) * g.to(cdt)[r]
    d = xs - out_fwd.to(cdt)[r]
    acc = torch.zeros(C, F, dtype=cdt, device=dx.device).index_add_(0, src, wg * (1 + tt * d))
    dx[:C] = acc.to(dx.dtype)
    if want_dt:
        part = (wg * d * d).sum(0, keepdim=True)
    return dx, part


def _gate(z):
    """``(s, s (1 - s))`` of ``s = sigmoid(z)`` from ``e = exp(-|z|)``, as the kernel forms
    them: finite for every finite ``z``, the derivative accurate in both tails."""
    e = torch.exp(-z.abs())
    r = 1.0 / (1.0 + e)
    return torch.where(z >= 0, r, e * r), e * r * r


def segment_gated(rowptr, col, k, q, v, out, ds=None, accumulate=False):
    """Gated aggregation of each CSR row's entries (cf. kernels.h): with ``s = sigmoid(k[r] +
    q[col[j]])``, ``out[r] = sum_j s v[col[j]]`` and, when ``ds`` is given, ``ds[r] = sum_j
    s (1 - s) v[col[j]]``; zeros for an empty row. ``accumulate``: ``out`` / ``ds`` hold an
    earlier pass's result, which this pass adds to; a row without an entry here keeps it
    bitwise. fp32 (fp64 for fp64 input)."""
    R = rowptr.numel() - 1
    F = k.shape[1]
    if R <= 0 or F == 0:
        return out, ds
    cdt = torch.float64 if k.dtype == torch.float64 else torch.float32
    rows = _row_ids(rowptr)
    c = col.long()
    s, d = _gate(k.to(cdt)[:R][rows] + q.to(cdt)[c])
    vv = v.to(cdt)[c]
    visited = ((rowptr[1:] - rowptr[:-1]) > 0).unsqueeze(1)
    for dst, w in ((out, s), (ds, d)):
        if dst is None:
            continue
        acc = torch.zeros(R, F, dtype=cdt, device=k.device).index_add_(0, rows, w * vv)
        if accumulate:
            acc = torch.where(visited, dst[:R].to(cdt) + acc, dst[:R].to(cdt))
        dst[:R] = acc.to(dst.dtype)
    return out, ds


def segment_gated_bwd_src(t_rowptr, t_col, k, q, v, g, dq, dv):
    """Source side of the backward of :func:`segment_gated` over the transposed pattern of
    any subset of the entries (cf. kernels.h): per entry ``r = t_col[j]`` of source row ``c``,
    ``s = sigmoid(k[r] + q[c])``; ``dv[c] = sum s g[r]`` and ``dq[c] = v[c] sum s (1 - s)
    g[r]``. Every row ``c`` is written. Returns ``(dq, dv)``."""
    C = t_rowptr.numel() - 1
    F = dq.shape[1]
    if C <= 0 or F == 0:
        return dq, dv
    cdt = torch.float64 if dq.dtype == torch.float64 else torch.float32
    src = _row_ids(t_rowptr)
    r = t_col.long()
    s, d = _gate(k.to(cdt)[r] + q.to(cdt)[:C][src])
    gg = g.to(cdt)[r]
    zero = lambda: torch.zeros(C, F, dtype=cdt, device=dq.device)  # noqa: E731
    dv[:C] = zero().index_add_(0, src, s * gg).to(dv.dtype)
    dq[:C] = (v.to(cdt)[:C] * zero().index_add_(0, src, d * gg)).to(dq.dtype)
    return dq, dv


def _edge_message(x, e, col, relu, eps, cdt):
    """``(z, m)`` per CSR slot: ``z = x[col] + e`` and ``m = (relu ? max(z, 0) : z) + eps``."""
    z = x.to(cdt)[col.long()] + e.to(cdt)
    return z, (torch.relu(z) if relu else z) + eps


def segment_softmax_edge(rowptr, col, x, e, t, out, lse, relu=True, eps=1e-7, second=False,
                         row_map=None):
    """Softmax aggregation of per-slot messages (cf. kernels.h): ``m_k = (relu ? max(z, 0) :
    z) + eps`` with ``z = x[col[k]] + e[k]``, ``lse = log sum_k exp(t m_k)`` and ``out = sum_k
    exp(t m_k - lse) m_k``. Empty rows, ``second`` and ``row_map`` as :func:`segment_softmax`,
    which this is once the messages stand as the source rows of an identity column map."""
    if rowptr.numel() - 1 <= 0 or x.shape[1] == 0:
        return out, lse
    cdt = torch.float64 if x.dtype == torch.float64 else torch.float32
    _, m = _edge_message(x, e, col, relu, eps, cdt)
    slots = torch.arange(col.numel(), device=col.device)
    return segment_softmax(rowptr, slots, m, t, out, lse, second, row_map)


def segment_softmax_edge_bwd(rowptr, col, x, e, t, g, out_fwd, lse, de, relu=True, eps=1e-7,
                             want_dt=True):
    """Destination-side backward of :func:`segment_softmax_edge` over any block of the
    entries, given the final ``(out_fwd, lse)`` (cf. kernels.h): per slot ``w = exp(t m -
    lse[r])``, ``d = m - out_fwd[r]``, ``de[k] = w g[r] (1 + t d)`` where ``!relu`` or ``z >
    0`` (else 0), and the one partial row ``sum w g[r] d^2`` of ``dt``. Returns ``(de, [1, F]
    partials or None)``."""
    F = x.shape[1]
    cdt = torch.float64 if x.dtype == torch.float64 else torch.float32
    part = torch.zeros(1, F, dtype=cdt, device=x.device) if want_dt else None
    nnz = col.numel()
    if nnz == 0 or F == 0:
        return de, part
    r = _row_ids(rowptr)
    tt = t.to(cdt)
    z, m = _edge_message(x, e, col, relu, eps, cdt)
    wg = torch.exp(tt * m - lse.to(cdt)[r]) * g.to(cdt)[r]
    d = m - out_fwd.to(cdt)[r]
    dm = wg * (1 + tt * d)
    if relu:
        dm = torch.where(z > 0, dm, torch.zeros((), dtype=cdt, device=x.device))
    de[:nnz] = dm.to(de.dtype)
    if want_dt:
        part = (wg * d * d).sum(0, keepdim=True)
    return de, part


def copy_rows(
    x: torch.Tensor,
    src_idx: Optional[torch.Tensor],
    dst_idx: Optional[torch.Tensor],
    out: torch.Tensor,
    accumulate: bool = False,
) -> torch.Tensor:
    n = (src_idx.numel() if src_idx is not None else
         dst_idx.numel() if dst_idx is not None else x.shape[0])
    if src_idx is not None:
        s = src_idx.long()
        vals = torch.zeros(n, x.shape[1], dtype=x.dtype, device=x.device)
        ok = s >= 0
        vals[ok] = x[s[ok]]
    else:
        vals = x[:n]
    if dst_idx is not None:
        d = dst_idx.long()
        keep = d >= 0
        d, vals = d[keep], vals[keep]
    else:
        d = torch.arange(n, device=x.device)
    if accumulate:
        out.index_add_(0, d, vals.to(out.dtype))
    else:
        out[d] = vals.to(out.dtype)
    return out


def masked_gather_rows(x, idx, mask, value, out):
    sel = mask == value
    out[sel] = x[idx[sel]]
    return out


def edge_softmax_fwd(rowptr: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    cdt = torch.float64 if s.dtype == torch.float64 else torch.float32
    s2 = s.to(cdt).reshape(s.shape[0], -1)
    rows = _row_ids(rowptr)
    R = rowptr.numel() - 1
    H = s2.shape[1]
    m = torch.full((R, H), float("-inf"), device=s.device, dtype=cdt)
    m = m.scatter_reduce(0, rows.unsqueeze(1).expand(-1, H), s2, reduce="amax")
    e = torch.exp(s2 - m[rows])
    den = torch.zeros(R, H, device=s.device, dtype=cdt).index_add_(0, rows, e)
    return (e / den[rows]).reshape(s.shape)


def edge_softmax_bwd(rowptr: torch.Tensor, alpha: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    cdt = torch.float64 if alpha.dtype == torch.float64 else torch.float32
    a2 = alpha.to(cdt).reshape(alpha.shape[0], -1)
    g2 = g.to(cdt).reshape(a2.shape)
    rows = _row_ids(rowptr)
    R = rowptr.numel() - 1
    dot = torch.zeros(R, a2.shape[1], device=alpha.device, dtype=cdt).index_add_(0, rows,
                                                                              a2 * g2)
    return (a2 * (g2 - dot[rows])).reshape(alpha.shape)


def _mask_to_words(keep: torch.Tensor) -> torch.Tensor:
    """Keep-mask -> int32 words in the kernels' layout: 512-element chunks, word j (64
    bit, little-endian int32 pair) of a chunk holds bit l = keep(8*l + j)."""
    flat = keep.reshape(-1)
    n = flat.numel()
    nch = (n + 511) // 512
    pad = torch.zeros(nch * 512, dtype=torch.bool, device=flat.device)
    pad[:n] = flat
    k = pad.view(nch, 64, 8).permute(0, 2, 1).to(torch.int64)  # [chunk, j, lane]
    lo = (k[:, :, :32] << torch.arange(32, device=k.device)).sum(-1)
    hi = (k[:, :, 32:] << torch.arange(32, device=k.device)).sum(-1)
    w = torch.stack([lo, hi], -1).reshape(-1)
    w = torch.where(w >= 2**31, w - 2**32, w)
    return w.to(torch.int32)


def _words_to_mask(bits: torch.Tensor, numel: int) -> torch.Tensor:
    nch = (numel + 511) // 512
    w = bits.reshape(-1)[: nch * 16].to(torch.int64) & 0xFFFFFFFF
    w = w.view(nch, 8, 2)
    lanes = torch.arange(32, device=w.device)
    lo = (w[:, :, 0:1] >> lanes) & 1
    hi = (w[:, :, 1:2] >> lanes) & 1
    k = torch.cat([lo, hi], -1)  # [chunk, j, lane]
    return k.permute(0, 2, 1).reshape(-1)[:numel].bool()


def bias_relu_pack(y: torch.Tensor, bias, bits, relu: bool) -> None:
    t = y.float()
    if bias is not None:
        t = t + bias.float()
    if relu:
        keep = t > 0
        t = torch.where(keep, t, torch.zeros((), device=t.device))
        if bits is not None:
            w = _mask_to_words(keep)
            bits.view(-1)[: w.numel()] = w
    y.copy_(t.to(y.dtype))


def relu_mask_bwd(g: torch.Tensor, bits: torch.Tensor) -> None:
    keep = _words_to_mask(bits, g.numel()).reshape(g.shape)
    g.masked_fill_(~keep, 0)


def row_scale_cols(x: torch.Tensor, s: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    out.copy_((x.float() * s.float().unsqueeze(1)).to(out.dtype))
    return out


def row_scale_colsum(x: torch.Tensor, s: torch.Tensor, out: torch.Tensor,
                     partial: torch.Tensor) -> torch.Tensor:
    nb = partial.shape[0]
    rpb = (x.shape[0] + nb - 1) // nb
    xf = x.float()
    partial.zero_()
    for b in range(nb):
        partial[b] = xf[b * rpb:(b + 1) * rpb].sum(0)
    return row_scale_cols(x, s, out)


def col_sum(g: torch.Tensor) -> torch.Tensor:
    return g.float().sum(0)


def pair_relu(rowptr, col, mode: int, rowterm, gat, gat2=None, rowmul=None, out=None):
    """CPU reference of the fused edge-MLP aggregation (csrc/kernels/edge_fused.hip)."""
    cdt = torch.float64 if gat.dtype == torch.float64 else torch.float32
    R = rowptr.numel() - 1
    rows = _row_ids(rowptr)
    c = col.long()
    pre = rowterm.to(cdt)[rows] + gat.to(cdt)[c]
    if mode == 0:
        val = pre.clamp_min(0)
    elif mode == 1:
        val = (pre > 0).to(cdt)
    else:
        val = torch.where(pre > 0, gat2.to(cdt)[c], torch.zeros((), dtype=cdt))
    acc = torch.zeros(R, gat.shape[1], dtype=cdt).index_add_(0, rows, val)
    if mode == 1:
        acc = acc * rowmul.to(cdt)[:R]
    if out is None:
        return acc.to(gat.dtype)
    out[:R].copy_(acc)
    return out


def _act(x, act: int):
    if act == 1:
        return x.clamp_min(0)
    if act == 2:
        return x * torch.sigmoid(x)
    if act == 3:
        return torch.where(x > 0, x, 0.2 * x)
    return x


def _act_grad(x, act: int):
    if act == 1:
        return (x > 0).to(x.dtype)
    if act == 2:
        s = torch.sigmoid(x)
        return s * (1 + x * (1 - s))
    if act == 3:
        return torch.where(x > 0, torch.ones_like(x), torch.full_like(x, 0.2))
    return torch.ones_like(x)


def gather_add_act(Y, P, src, Q, dst, gin, out, act: int):
    cdt = torch.float64 if out.dtype == torch.float64 else torch.float32
    E, F = out.shape
    pre = torch.zeros(E, F, dtype=cdt)
    if Y is not None:
        pre += Y[:E].to(cdt)
    if P is not None:
        pre += P.to(cdt)[src[:E].long()]
    if Q is not None:
        pre += Q.to(cdt)[dst[:E].long()]
    if gin is None:
        out.copy_(_act(pre, act))
    else:
        out.copy_(gin[:E].to(cdt) * _act_grad(pre, act))
    return out


def tile32_encode(keep: torch.Tensor) -> torch.Tensor:
    """Keep mask [M, N] -> int64 words in the dual-GEMM "tile32" layout
    (csrc/kernels/dual_gemm.hip): word[(rb * NT + t) * 16 + r] bit l = keep of
    (32 rb + (r & 3) + 8 (r >> 2) + 4 (l >> 5), 32 t + (l & 31)); rows padded to 256."""
    M, N = keep.shape
    NT = N // 32
    Mp = (M + 255) // 256 * 256
    k = torch.zeros(Mp, N, dtype=torch.bool)
    k[:M] = keep.cpu()
    lane = torch.arange(64)
    r = torch.arange(16)
    rows = (r.unsqueeze(1) & 3) + 8 * (r.unsqueeze(1) >> 2) + 4 * (lane.unsqueeze(0) >> 5)  # [16, 64]
    cols = lane & 31
    kt = k.view(Mp // 32, 32, NT, 32)                      # [rb, rr, t, cc]
    # non-adjacent advanced indices: the broadcast index dims come first -> [16, 64, rb, t]
    bits = kt[:, rows, :, cols.unsqueeze(0).expand(16, 64)]
    bits = bits.permute(2, 3, 0, 1).to(torch.int64)        # [rb, t, 16, 64]
    w = (bits << torch.arange(64, dtype=torch.int64)).sum(-1)  # wraps like uint64
    return w.reshape(-1)


def tile32_decode(words: torch.Tensor, M: int, N: int) -> torch.Tensor:
    NT = N // 32
    Mp = (M + 255) // 256 * 256
    w = words.cpu()[: Mp // 32 * NT * 16].view(Mp // 32, NT, 16, 1)
    bits = ((w >> torch.arange(64, dtype=torch.int64)) & 1).bool()  # [rb, t, 16, 64]
    lane = torch.arange(64)
    r = torch.arange(16)
    rows = (r.unsqueeze(1) & 3) + 8 * (r.unsqueeze(1) >> 2) + 4 * (lane.unsqueeze(0) >> 5)
    cols = (lane & 31).unsqueeze(0).expand(16, 64)
    out = torch.zeros(Mp // 32, 32, NT, 32, dtype=torch.bool)
    out[:, rows, :, cols] = bits.permute(2, 3, 0, 1)  # -> [16, 64, rb, t]
    return out.view(Mp, N)[:M]
