"""Autograd-aware sparse primitives built on the native kernels.

* :func:`aggregate` — CSR SpMM (sum / mean / edge-weighted, multi-head); backward is the
  same kernel on the cached transposed CSR (or on the same CSR for symmetric patterns).
  With an :class:`EdgeDrop` the sum / mean runs over a random subgraph drawn per call
  (DropEdge), fused into the aggregation kernel.
* :func:`aggregate_multi` — mean, max, min and standard deviation of the same neighbour
  rows in ONE gather pass (the PNA aggregators), as column blocks of one ``[R, A*F]`` tensor.
* :func:`softmax_aggregate` — the learnable softmax aggregation (per channel, the score is
  the value times a temperature) in one gather pass, with the temperature's gradient.
* :func:`softmax_aggregate_edge` — the same with a per-edge term in the message
  (``relu(x_j + e_ij) + eps``, GENConv with edge features), formed inside the gather pass;
  the backward writes the edge gradient once and sums it once for ``dx``.
* :func:`gated_aggregate` — the per-channel sigmoid-gated sum (``sum_j sigmoid(k_i + q_j)
  v_j``, ResGatedGraphConv / GatedGCN) in one gather pass; ``dk`` is an elementwise product
  with a second output of that pass, ``dq`` / ``dv`` one gather over the transposed pattern.
* :func:`gather` / :func:`scatter_sum` — vertex->edge gather and edge->vertex scatter-sum
  over a static :class:`~dgraph_amd.ops.csr.IndexMap`; each is the other's adjoint
  (the core contract of the reference, tests/test_NCCLCommPlan.py:100-111,297-307),
  and both are deterministic (segment sums, no float atomics).
* :func:`edge_softmax` — stable softmax over each destination's incoming edges.
* :func:`edge_dot` — one dot product per CSR entry and head from two vertex rows (SDDMM);
  backward is two edge-weighted SpMMs.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch
from torch.autograd import Function

from . import kernels as K
from .csr import CSR, IndexMap


class _AggregateFn(Function):
    @staticmethod
    def forward(ctx, x, csr: CSR, edge_weight, mean: bool, heads: int):
        row_scale = csr.inv_degree() if mean else None
        out = K.spmm(csr.rowptr, csr.col, x, edge_weight=edge_weight,
                     row_scale=row_scale, heads=heads)
        ctx.csr, ctx.mean, ctx.heads = csr, mean, heads
        ctx.save_for_backward(x if edge_weight is not None and edge_weight.requires_grad else None,
                              edge_weight)
        return out

    @staticmethod
    def backward(ctx, g):
        csr: CSR = ctx.csr
        x_saved, ew = ctx.saved_tensors
        g = g.contiguous()
        gx = gw = None
        col_scale = csr.inv_degree() if ctx.mean else None
        if ctx.needs_input_grad[0]:
            if ew is None and csr.symmetric:
                gx = K.spmm(csr.rowptr, csr.col, g, col_scale=col_scale, heads=ctx.heads)
            else:
                t = csr.transpose()
                ew_t = None if ew is None else ew.reshape(csr.nnz, ctx.heads)[t.perm].contiguous()
                gx = K.spmm(t.rowptr, t.col, g, edge_weight=ew_t, col_scale=col_scale,
                            heads=ctx.heads)
        if ew is not None and ctx.needs_input_grad[2]:
            # d w[j,h] = row_scale[r] * <g[r, h-slice], x[c_j, h-slice]>  (SDDMM): one
            # kernel on the GPU (fp32 scores, nothing [nnz, F] is written); on the CPU the
            # composed expression, in fp64 when the weights are
            gg, xx = g, x_saved
            if not g.is_cuda:
                cdt = torch.float64 if ew.dtype == torch.float64 else torch.float32
                gg, xx = g.to(cdt), x_saved.to(cdt)
            else:  # a contiguous view off a 4-element boundary: the kernel's vector path
                gg, xx = (t.clone() if t.data_ptr() % (4 * t.element_size()) else t
                          for t in (g, x_saved))
            gw = K.edge_dot(csr.rowptr, csr.col, gg, xx, heads=ctx.heads,
                            row_scale=csr.inv_degree() if ctx.mean else None)
            gw = gw.reshape(ew.shape).to(ew.dtype)
        return gx, None, gw, None, None


class _AggregateExtremeFn(Function):
    """Max / min over each row's entries. The forward records the winning CSR slot per
    ``(row, feature)`` (the first that attains the extremum); the backward routes the whole
    of ``g[r, f]`` to that slot's source row, as a gather over the transposed pattern."""

    @staticmethod
    def forward(ctx, x, csr: CSR, minimum: bool):
        out, arg = K.segment_extreme(csr.rowptr, csr.col, x, minimum=minimum)
        ctx.csr = csr
        ctx.save_for_backward(arg)
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(ctx, g, _g_arg=None):
        (arg,) = ctx.saved_tensors
        t, rel = ctx.csr.transpose_rel()
        return K.segment_extreme_bwd(t.rowptr, t.col, rel, g.contiguous(), arg), None, None


PNA_AGGREGATORS = ("mean", "max", "min", "std")


def check_aggregators(aggregators) -> tuple:
    """``aggregators`` as a tuple of distinct names out of :data:`PNA_AGGREGATORS`."""
    aggs = (aggregators,) if isinstance(aggregators, str) else tuple(aggregators)
    bad = [a for a in aggs if a not in PNA_AGGREGATORS]
    if bad or not aggs or len(set(aggs)) != len(aggs):
        raise ValueError(f"aggregators must be distinct names out of {PNA_AGGREGATORS}, "
                         f"got {aggs!r}")
    return aggs


def multi_blocks(buf: torch.Tensor, aggregators: tuple, F: int) -> dict:
    """The column blocks of a ``[R, A*F]`` buffer by aggregator name (views)."""
    return {a: buf[:, i * F:(i + 1) * F] for i, a in enumerate(aggregators)}


def vec_rows(x: torch.Tensor) -> torch.Tensor:
    """``x`` as the fused kernels take a row array: unit column stride, and on the GPU, for
    a width that is a multiple of 4, a row stride divisible by 4 and a 16-B aligned base
    (a copy only when the view is not)."""
    F = x.shape[1]
    if x.stride(1) != 1 and F > 1:
        return x.contiguous()
    if x.is_cuda and F % 4 == 0 and x.shape[0] > 1 and (
            x.stride(0) % 4 or x.data_ptr() % (4 * x.element_size())):
        return x.contiguous()
    return x


class _AggregateMultiFn(Function):
    """The PNA aggregators of each row's entries from one pass over the neighbour rows
    (K.segment_pna); the backward is one gather over the transposed pattern."""

    @staticmethod
    def forward(ctx, x, csr: CSR, aggregators: tuple, eps: float):
        R, F = csr.num_rows, x.shape[1]
        out = torch.empty(R, len(aggregators) * F, dtype=x.dtype, device=x.device)
        blk = multi_blocks(out, aggregators, F)
        mean, sdev = blk.get("mean"), blk.get("std")
        if mean is not None or sdev is not None:  # the moments come as a pair
            mean = torch.empty(R, F, dtype=x.dtype, device=x.device) if mean is None else mean
            sdev = torch.empty(R, F, dtype=x.dtype, device=x.device) if sdev is None else sdev
        args = {k: torch.empty(R, F, dtype=torch.int32, device=x.device)
                for k in ("max", "min") if k in blk}
        K.segment_pna(csr.rowptr, csr.col, x, mean=mean, sdev=sdev, vmax=blk.get("max"),
                      amax=args.get("max"), vmin=blk.get("min"), amin=args.get("min"), eps=eps)
        ctx.csr, ctx.aggregators = csr, aggregators
        # the moments that are blocks of ``out`` are saved with it, the others on their own
        ctx.save_for_backward(x, out, None if "mean" in blk else mean,
                              None if "std" in blk else sdev, args.get("max"), args.get("min"))
        return out

    @staticmethod
    def backward(ctx, g):
        x, out, mean, sdev, amax, amin = ctx.saved_tensors
        csr: CSR = ctx.csr
        blk = multi_blocks(out.detach(), ctx.aggregators, x.shape[1])
        mean, sdev = blk.get("mean", mean), blk.get("std", sdev)
        gb = multi_blocks(g.contiguous(), ctx.aggregators, x.shape[1])
        t, rel = csr.transpose_rel()
        inv = csr.inv_degree()
        if x.dtype == torch.float64:
            inv = 1.0 / csr.degree().clamp(min=1).double()
        gx = K.segment_pna_bwd(t.rowptr, t.col, rel, x, inv, g_mean=gb.get("mean"),
                               g_std=gb.get("std"), mean=mean, sdev=sdev, g_max=gb.get("max"),
                               amax=amax, g_min=gb.get("min"), amin=amin)
        return gx, None, None, None


def aggregate_multi(x: torch.Tensor, csr: CSR, aggregators=PNA_AGGREGATORS,
                    eps: float = 1e-5) -> torch.Tensor:
    """Several aggregations of the same neighbour rows at once: ``[R, A*F]``, one ``F``-wide
    column block per name in ``aggregators`` (any distinct subset of ``"mean"``, ``"max"``,
    ``"min"``, ``"std"``, in the order given), so the result feeds one GEMM without a
    ``cat``. ``mean`` / ``max`` / ``min`` are :func:`aggregate`'s; ``std`` is the population
    standard deviation ``sqrt(mean((x_j - mean)^2) + eps)`` (``sqrt(eps)`` for an empty row,
    PyG's value). On the GPU (fp32) one kernel gathers each neighbour row once for all of
    them, and one kernel computes the gradient."""
    aggs = check_aggregators(aggregators)
    if aggs == ("mean",):
        return aggregate(x, csr, reduce="mean")
    return _AggregateMultiFn.apply(vec_rows(x), csr, aggs, float(eps))


def as_temperature(t, x: torch.Tensor) -> torch.Tensor:
    """The temperature of a softmax aggregation as a tensor: a float becomes a ``[1]`` tensor
    of ``x``'s dtype on its device; a tensor must be 0-d, ``[1]`` or ``[F]``."""
    if not isinstance(t, torch.Tensor):
        return torch.full((1,), float(t), dtype=x.dtype, device=x.device)
    if t.numel() != 1 and (t.dim() != 1 or t.numel() != x.shape[1]):
        raise ValueError(f"t must be a scalar, [1] or [{x.shape[1]}], got {tuple(t.shape)}")
    return t


def temperature_grad(partials: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """``dt`` in ``t``'s shape and dtype from the ``[P, F]`` partial rows of the backward
    kernel (a scalar temperature receives the sum over the channels)."""
    dt = partials.sum(0)
    if t.numel() == 1:
        dt = dt.sum()
    return dt.reshape(t.shape).to(t.dtype)


class _SoftmaxAggregateFn(Function):
    """Softmax aggregation (K.segment_softmax). ``(out, lse)`` is all the forward keeps; the
    backward recomputes every weight in one gather over the transposed pattern, which gives
    ``dx`` and the partial rows of ``dt`` together."""

    @staticmethod
    def forward(ctx, x, t, csr: CSR):
        out, lse = K.segment_softmax(csr.rowptr, csr.col, x, t)
        ctx.csr = csr
        ctx.save_for_backward(x, t, out, lse)
        return out

    @staticmethod
    def backward(ctx, g):
        x, t, out, lse = ctx.saved_tensors
        tr = ctx.csr.transpose()
        want_dt = ctx.needs_input_grad[1]
        dx, part = K.segment_softmax_bwd(tr.rowptr, tr.col, x, t, vec_rows(g), out, lse,
                                         want_dt=want_dt)
        return dx, (temperature_grad(part, t) if want_dt else None), None


def softmax_aggregate(x: torch.Tensor, csr: CSR, t=1.0) -> torch.Tensor:
    """Softmax aggregation (PyG's ``SoftmaxAggregation``, the aggregator of ``GENConv``):
    ``out[r, f] = sum_j softmax_j(t_f x[j, f]) x[j, f]`` over the entries ``j`` of row ``r``
    (0 for an empty row). The softmax is per channel and its score is the value itself:
    ``t = 0`` is the mean, ``t -> +inf`` / ``-inf`` the max / min. ``t``: a float, a 0-d or
    ``[1]`` tensor, or an ``[F]`` tensor; it may require grad (a scalar receives the sum of
    the per-channel gradient). On the GPU (fp32) one kernel gathers each neighbour row once
    and writes nothing per edge, and one kernel computes ``dx`` and ``dt``."""
    return _SoftmaxAggregateFn.apply(vec_rows(x), as_temperature(t, x), csr)


class _GatedAggregateFn(Function):
    """Gated aggregation (K.segment_gated). The forward keeps ``ds = sum_j s (1 - s) v_j``
    from the same pass, which is the whole destination side of the backward (``dk = g *
    ds``); the source side recomputes every gate in one gather over the transposed pattern,
    which gives ``dq`` and ``dv`` together."""

    @staticmethod
    def forward(ctx, k, q, v, csr: CSR):
        out, ds = K.segment_gated(csr.rowptr, csr.col, k, q, v,
                                  want_ds=ctx.needs_input_grad[0])
        ctx.csr = csr
        ctx.save_for_backward(k, q, v, ds)
        return out

    @staticmethod
    def backward(ctx, g):
        k, q, v, ds = ctx.saved_tensors
        g = vec_rows(g)
        dk = g * ds if ctx.needs_input_grad[0] else None
        dq = dv = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            tr = ctx.csr.transpose()
            dq, dv = K.segment_gated_bwd_src(tr.rowptr, tr.col, k, q, v, g)
        return dk, dq, dv, None


def gated_aggregate(k: torch.Tensor, q: torch.Tensor, v: torch.Tensor, csr: CSR) -> torch.Tensor:
    """Gated aggregation (the neighbourhood sum of PyG's ``ResGatedGraphConv`` and of
    GatedGCN): ``out[r, f] = sum_j sigmoid(k[r, f] + q[j, f]) v[j, f]`` over the entries ``j``
    of row ``r`` (0 for an empty row), a sigmoid gate per channel. ``k``: ``[csr.num_rows,
    F]``; ``q``, ``v``: ``[csr.num_cols, F]``; each may be a column view of a wider buffer
    (the ``[k | q | v]`` of one projection). On the GPU (fp32) one kernel gathers each
    neighbour's ``q`` and ``v`` rows once and writes nothing per edge; ``dk`` is an
    elementwise product with a second output of that pass, and one kernel over the transposed
    pattern computes ``dq`` and ``dv``."""
    if k.dim() != 2 or q.shape != v.shape or q.dim() != 2 or q.shape[1] != k.shape[1]:
        raise ValueError(f"gated_aggregate: k [R, F], q and v [C, F] expected, got "
                         f"{tuple(k.shape)}, {tuple(q.shape)}, {tuple(v.shape)}")
    if k.shape[0] != csr.num_rows or q.shape[0] != csr.num_cols:
        raise ValueError(f"gated_aggregate: k needs {csr.num_rows} rows and q / v "
                         f"{csr.num_cols}, got {k.shape[0]} and {q.shape[0]}")
    return _GatedAggregateFn.apply(vec_rows(k), vec_rows(q), vec_rows(v), csr)


@dataclass
class EdgeDrop:
    """DropEdge (Rong et al., ICLR 2020; PyG's ``dropout_edge``) for one aggregation call:
    every edge is removed with probability ``p``, a fresh subgraph per ``seed``. The pattern
    is never rebuilt and no mask is stored: the keep decision of an edge is a pure function
    of ``(seed, destination id, source id)`` (:func:`~dgraph_amd.ops.philox.edge_keep_mask`),
    regenerated by the forward and by the transposed pass.

    ``seed``: a 1-element int64 tensor that the kernels read from device memory (so a
    captured step draws a new subgraph per replay; a Python int is wrapped); it must hold its
    value until the backward has run. ``undirected``: both directions of an edge share one
    fate (PyG's ``force_undirected``), so an undirected graph stays undirected. Parallel
    entries with equal ``(dst, src)`` always share one fate. The result is the aggregation
    over the subgraph: no ``1 / (1 - p)`` rescale."""

    p: float
    seed: torch.Tensor
    undirected: bool = False

    def __post_init__(self):
        self.p = float(self.p)
        if not 0.0 <= self.p < 1.0:
            raise ValueError(f"EdgeDrop: p must lie in [0, 1), got {self.p}")
        if not isinstance(self.seed, torch.Tensor):
            self.seed = torch.tensor([int(self.seed)], dtype=torch.int64)
        if self.seed.numel() != 1 or self.seed.dtype != torch.int64:
            raise ValueError("EdgeDrop: seed must be a 1-element int64 tensor")


def inv_kept(kept: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """``1 / max(kept, 1)``: the row scale of the mean over the kept entries."""
    return 1.0 / kept.clamp(min=1).to(torch.float64 if dtype == torch.float64 else torch.float32)


class _AggregateDropFn(Function):
    """Sum / mean over the kept entries of each row (K.spmm_drop). The forward saves only the
    kept degrees (for mean); the backward is the same kernel over the transposed pattern with
    ``transposed=True``, which regenerates the same decisions from the vertex ids."""

    @staticmethod
    def forward(ctx, x, csr: CSR, drop: EdgeDrop, mean: bool, row_ids, col_ids):
        ids = dict(seed=drop.seed, p=drop.p, undirected=drop.undirected)
        scale = None
        if mean:
            kept = K.kept_degree(csr.rowptr, csr.col, row_ids=row_ids, col_ids=col_ids,
                                 num_cols=x.shape[0], **ids)
            scale = inv_kept(kept, x.dtype)
        out = K.spmm_drop(csr.rowptr, csr.col, x, row_scale=scale, row_ids=row_ids,
                          col_ids=col_ids, **ids)
        ctx.csr, ctx.drop, ctx.mean, ctx.ids, ctx.x_rows = csr, drop, mean, (row_ids, col_ids), \
            x.shape[0]
        ctx.save_for_backward(kept if mean else None)
        return out

    @staticmethod
    def backward(ctx, g):
        (kept,) = ctx.saved_tensors
        drop: EdgeDrop = ctx.drop
        row_ids, col_ids = ctx.ids
        # a symmetric pattern is its own transpose (CSR.transpose returns it): read as
        # "rows are sources" it lists each source's destinations, whichever way the key is
        # formed, so transposed=True is all either case needs
        t = ctx.csr.transpose()
        g = vec_rows(g)
        gx = K.spmm_drop(t.rowptr, t.col, g, seed=drop.seed, p=drop.p,
                         undirected=drop.undirected, transposed=True,
                         col_scale=inv_kept(kept, g.dtype) if ctx.mean else None,
                         row_ids=col_ids, col_ids=row_ids)
        if ctx.x_rows != t.num_rows:  # rows no column reaches
            gx = torch.cat([gx, gx.new_zeros(ctx.x_rows - t.num_rows, gx.shape[1])])
        return gx, None, None, None, None, None


def aggregate(
    x: torch.Tensor,
    csr: CSR,
    edge_weight: Optional[torch.Tensor] = None,
    reduce: str = "sum",
    heads: int = 1,
    drop: Optional[EdgeDrop] = None,
    row_ids: Optional[torch.Tensor] = None,
    col_ids: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """``out[r] = reduce_{j in N(r)} w_j * x[j]`` over the CSR rows.

    ``drop``: an :class:`EdgeDrop`; the ``"sum"`` / ``"mean"`` then runs over a random
    subgraph drawn from its seed (``"mean"`` divides by the number of KEPT entries,
    ``max(kept, 1)``; a row that lost every entry gives 0), on the GPU in one fused fp32 kernel
    that never loads the row of a dropped entry. ``row_ids`` / ``col_ids`` (int64, one per CSR
    row / per row of ``x``) are the vertex ids the decision is keyed by; by default the row
    and column numbers. A ``symmetric`` CSR runs its backward on itself. ``drop=None`` or
    ``p == 0`` is the plain call, the same kernels and the same bits. Not supported under
    ``drop`` (``ValueError``): edge weights, ``heads > 1``, any other ``reduce``; bf16 rows,
    hub splitting, the fused executors and the attention layers do not take it either. A GCN
    renormalised by kept degrees would combine :func:`~dgraph_amd.ops.kernels.kept_degree`
    with ``row_scale`` / ``col_scale`` of :func:`~dgraph_amd.ops.kernels.spmm_drop`.

    ``edge_weight`` is ``[nnz]`` or ``[nnz, heads]`` in CSR slot order; with heads > 1
    the feature dim is split into ``heads`` equal slices, each scaled by its head weight.

    ``reduce="max"`` / ``"min"``: the elementwise extremum over a row's entries (0 for an
    empty row), unweighted and single-head. Its gradient goes to ONE entry per
    ``(row, feature)``: the first in CSR slot order that attains the extremum.

    ``reduce="std"``: the population standard deviation over a row's entries,
    ``sqrt(mean((x_j - mean)^2) + 1e-5)``, unweighted and single-head: the ``"std"`` block of
    :func:`aggregate_multi`, which computes several of these from one pass.

    ``reduce="softmax"``: :func:`softmax_aggregate` at temperature 1, unweighted and
    single-head.
    """
    if drop is not None and drop.p > 0.0:
        if reduce not in ("sum", "mean"):
            raise ValueError(f"drop supports reduce 'sum' / 'mean', got {reduce!r}")
        if edge_weight is not None:
            raise ValueError("drop takes no edge weights")
        if heads != 1:
            raise ValueError(f"drop takes one head, got heads={heads}")
        return _AggregateDropFn.apply(vec_rows(x), csr, drop, reduce == "mean", row_ids,
                                      col_ids)
    if reduce == "softmax":
        if edge_weight is not None:
            raise ValueError("reduce='softmax' takes no edge weights")
        if heads != 1:
            raise ValueError(f"reduce='softmax' takes one head, got heads={heads}")
        return softmax_aggregate(x, csr, 1.0)
    if reduce == "std":
        if edge_weight is not None:
            raise ValueError("reduce='std' takes no edge weights")
        if heads != 1:
            raise ValueError(f"reduce='std' takes one head, got heads={heads}")
        return aggregate_multi(x, csr, ("std",))
    if reduce in ("max", "min"):
        if edge_weight is not None:
            raise ValueError(f"reduce={reduce!r} takes no edge weights")
        if heads != 1:
            raise ValueError(f"reduce={reduce!r} takes one head, got heads={heads}")
        if x.stride(1) != 1 and x.shape[1] > 1:  # a row stride is fine, a feature stride not
            x = x.contiguous()
        return _AggregateExtremeFn.apply(x, csr, reduce == "min")[0]
    if reduce not in ("sum", "mean"):
        raise ValueError(f"unsupported reduce {reduce!r}")
    ew = None
    if edge_weight is not None:
        ew = edge_weight.reshape(csr.nnz, heads)  # native path casts to fp32 itself
        if ew.dtype not in (torch.float32, torch.float64):
            ew = ew.float()
    return _AggregateFn.apply(x.contiguous(), csr, ew, reduce == "mean", heads)


def _slot_transpose(csr: CSR) -> CSR:
    """The transposed pattern WITH its slot map (``perm``: its slots as ``csr``'s slots). A
    ``symmetric`` CSR's :meth:`CSR.transpose` is the pattern alone, so one is built (and
    cached by :meth:`CSR.transpose_rel`)."""
    t = csr.transpose()
    if t is csr or not t._perm_to_parent or t._transpose is not csr:
        t = csr.transpose_rel()[0]
    return t


def edge_dot_grads(csr: CSR, a, b, w, heads: int, want_a: bool = True, want_b: bool = True,
                   da_out: Optional[torch.Tensor] = None, beta: float = 0.0):
    """The adjoint of ``s = edge_dot(a, b)`` applied to ``w = scale * dL/ds`` (``[nnz,
    heads]``), as two edge-weighted SpMMs: ``da[r] = sum_k w_k b[col[k]]`` over ``csr`` (into
    ``da_out`` with ``beta`` when given) and ``db[c] = sum_k w_k a[r(k)]`` over its transpose
    (``[csr.num_cols, F]``)."""
    da = db = None
    if want_a:
        da = K.spmm(csr.rowptr, csr.col, b, da_out, edge_weight=w, heads=heads, beta=beta)
    if want_b:
        t = _slot_transpose(csr)
        db = K.spmm(t.rowptr, t.col, a, edge_weight=w[t.perm].contiguous(), heads=heads)
    return da, db


# out-degree above which a source's de rows are summed as separate segment waves
EDGE_SUM_HUB_CAP = 2048


def sum_edge_rows(csr: CSR, de: torch.Tensor, out: Optional[torch.Tensor] = None,
                  hub_cap: int = EDGE_SUM_HUB_CAP) -> torch.Tensor:
    """``dx[c] = sum_{k: col[k] = c} de[k]``: the per-slot rows ``de`` (``[nnz, F]`` in
    ``csr``'s slot order) summed per source, ``[csr.num_cols, F]``. A plain row-sum SpMM over
    the slot-transposed pattern, whose slot map is the column array and ``de`` the source
    matrix; a source of more than ``hub_cap`` entries is summed in segments."""
    tt = _slot_transpose(csr)
    return K.spmm(tt.rowptr, tt.perm, de, out, split=tt.hub_split(hub_cap))


class _SoftmaxAggregateEdgeFn(Function):
    """Softmax aggregation of per-edge messages (K.segment_softmax_edge). ``(out, lse)`` is
    all the forward keeps beside its inputs; the backward recomputes every message and weight
    in one pass over the same pattern, which writes ``de`` and the partial rows of ``dt``;
    ``dx`` is the row sum of ``de`` over the slot-transposed pattern."""

    @staticmethod
    def forward(ctx, x, edge, t, csr: CSR, relu: bool, eps: float):
        out, lse = K.segment_softmax_edge(csr.rowptr, csr.col, x, edge, t, relu=relu, eps=eps)
        ctx.csr, ctx.relu, ctx.eps = csr, relu, eps
        ctx.save_for_backward(x, edge, t, out, lse)
        return out

    @staticmethod
    def backward(ctx, g):
        x, edge, t, out, lse = ctx.saved_tensors
        csr: CSR = ctx.csr
        want_dt = ctx.needs_input_grad[2]
        de, part = K.segment_softmax_edge_bwd(csr.rowptr, csr.col, x, edge, t, vec_rows(g), out,
                                              lse, relu=ctx.relu, eps=ctx.eps, want_dt=want_dt)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = sum_edge_rows(csr, de)
            if x.shape[0] != csr.num_cols:  # rows no column reaches
                dx = torch.cat([dx, dx.new_zeros(x.shape[0] - csr.num_cols, dx.shape[1])])
        return (dx, de if ctx.needs_input_grad[1] else None,
                temperature_grad(part, t) if want_dt else None, None, None, None)


def softmax_aggregate_edge(x: torch.Tensor, edge: torch.Tensor, csr: CSR, t=1.0,
                           relu: bool = True, eps: float = 1e-7) -> torch.Tensor:
    """Softmax aggregation of messages that depend on the edge (PyG's ``GENConv(edge_dim=)``
    with ``aggr="softmax"``): for slot ``k`` of row ``r``, ``m_k = relu(x[col[k]] + edge[k]) +
    eps`` (``relu=False``: no relu) and ``out[r, f] = sum_k softmax_k(t_f m_k) m_k`` (0 for an
    empty row). ``edge`` is ``[csr.nnz, F]`` in the SLOT order of ``csr``; values in the order
    of the edge list the CSR was built from go through ``csr.permute_edges`` first. ``t`` as in
    :func:`softmax_aggregate`. Autograd covers ``x``, ``edge`` and ``t`` (a scalar receives the
    sum of the per-channel gradient). On the GPU (fp32) one kernel forms every message in
    registers between the gather and the softmax and writes nothing per edge; the backward
    writes the edge gradient once and sums it once for ``dx``."""
    if x.dim() != 2 or edge.dim() != 2 or tuple(edge.shape) != (csr.nnz, x.shape[1]):
        raise ValueError(f"softmax_aggregate_edge: edge must be [{csr.nnz}, {x.shape[-1]}] in "
                         f"csr's slot order, got {tuple(edge.shape)}")
    if x.shape[0] < csr.num_cols:
        raise ValueError(f"softmax_aggregate_edge: x has {x.shape[0]} rows, the pattern "
                         f"{csr.num_cols} columns")
    return _SoftmaxAggregateEdgeFn.apply(vec_rows(x), vec_rows(edge), as_temperature(t, x), csr,
                                         bool(relu), float(eps))


class _EdgeDotFn(Function):
    """Per-edge dot products (K.edge_dot); the backward is two edge-weighted SpMMs, one over
    the pattern and one over its transpose."""

    @staticmethod
    def forward(ctx, a, b, csr: CSR, heads: int, scale: float):
        s = K.edge_dot(csr.rowptr, csr.col, a, b, heads=heads, scale=scale)
        ctx.csr, ctx.heads, ctx.scale = csr, heads, scale
        ctx.save_for_backward(a, b)
        return s

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        csr: CSR = ctx.csr
        w = g.reshape(csr.nnz, ctx.heads)
        w = (w * ctx.scale if ctx.scale != 1.0 else w).contiguous()
        da, db = edge_dot_grads(csr, a, b, w, ctx.heads, ctx.needs_input_grad[0],
                                ctx.needs_input_grad[1])
        if db is not None and b.shape[0] != csr.num_cols:  # rows no column reaches
            db = torch.cat([db, db.new_zeros(b.shape[0] - csr.num_cols, b.shape[1])])
        return da, db, None, None, None


def check_edge_dot(a: torch.Tensor, b: torch.Tensor, num_rows: int, num_cols: int,
                   heads: int) -> None:
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1] or a.dtype != b.dtype:
        raise ValueError(f"edge_dot: a and b must be 2-D of one width and dtype, got "
                         f"{tuple(a.shape)} {a.dtype} and {tuple(b.shape)} {b.dtype}")
    if heads < 1 or a.shape[1] % heads != 0:
        raise ValueError(f"edge_dot: heads={heads} must divide the width {a.shape[1]}")
    if a.shape[0] != num_rows:
        raise ValueError(f"edge_dot: a has {a.shape[0]} rows, the pattern {num_rows}")
    if b.shape[0] < num_cols:
        raise ValueError(f"edge_dot: b has {b.shape[0]} rows, the pattern {num_cols} columns")


def edge_dot(a: torch.Tensor, b: torch.Tensor, csr: CSR, heads: int = 1,
             scale: float = 1.0) -> torch.Tensor:
    """One score per CSR entry and head (the SDDMM shape):
    ``s[k, h] = scale * <a[r(k), h-slice], b[col[k], h-slice]>`` for every slot ``k`` of
    ``csr``, ``r(k)`` the row that holds it; ``[nnz, heads]`` in CSR slot order (fp32 on the
    GPU, accumulated in fp32 from fp32 or bf16 rows). ``a``: ``[csr.num_rows, F]``, ``b``:
    ``[>= csr.num_cols, F]``; ``a is b`` scores a square pattern with one embedding
    (``<z_i, z_j>``) and receives the sum of both gradients. On the GPU one kernel reads each
    row once per entry and writes nothing per edge but the scores; the backward is two
    edge-weighted SpMMs. No double backward."""
    heads = int(heads)
    check_edge_dot(a, b, csr.num_rows, csr.num_cols, heads)
    if a is b:
        a = b = vec_rows(a)
    else:
        a, b = vec_rows(a), vec_rows(b)
    return _EdgeDotFn.apply(a, b, csr, heads, float(scale))


class _GatherFn(Function):
    @staticmethod
    def forward(ctx, x, imap: IndexMap):
        ctx.imap = imap
        ctx.n = x.shape[0]
        return K.gather_rows(x, imap.idx)

    @staticmethod
    def backward(ctx, g):
        t = ctx.imap.transpose_csr()
        gx = K.spmm(t.rowptr, t.col, g.contiguous(), split=ctx.imap.transpose_split())
        return gx, None


class _ScatterSumFn(Function):
    @staticmethod
    def forward(ctx, x, imap: IndexMap):
        ctx.imap = imap
        t = imap.transpose_csr()
        return K.spmm(t.rowptr, t.col, x.contiguous(), split=imap.transpose_split())

    @staticmethod
    def backward(ctx, g):
        return K.gather_rows(g.contiguous(), ctx.imap.idx), None


def gather(x: torch.Tensor, imap: IndexMap) -> torch.Tensor:
    """``y[i] = x[idx[i]]``; backward is the deterministic scatter-sum."""
    return _GatherFn.apply(x, imap)


def scatter_sum(x: torch.Tensor, imap: IndexMap) -> torch.Tensor:
    """``y[v] = sum_{i: idx[i]=v} x[i]`` (``imap.num_src`` output rows)."""
    return _ScatterSumFn.apply(x, imap)


class _EdgeSoftmaxFn(Function):
    @staticmethod
    def forward(ctx, scores, rowptr):
        alpha = K.edge_softmax_fwd(rowptr, scores)
        ctx.save_for_backward(rowptr, alpha)
        return alpha

    @staticmethod
    def backward(ctx, g):
        rowptr, alpha = ctx.saved_tensors
        return K.edge_softmax_bwd(rowptr, alpha, g), None


def edge_softmax(scores: torch.Tensor, csr: CSR) -> torch.Tensor:
    """Softmax of ``scores[nnz(, H)]`` (CSR slot order) over each row's edges."""
    return _EdgeSoftmaxFn.apply(scores, csr.rowptr)
