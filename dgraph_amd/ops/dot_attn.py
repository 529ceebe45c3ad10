"""Fused fp32 scaled dot-product graph attention with its exact adjoint (TransformerConv).

For one relation (destination rows i, source columns j over ``[local sources | halo rows]``)
and per head h (channels ``[hD, (h+1)D)`` of ``C = heads * D``)::

    e_ij  = scale * <q_i[head h], k_j[head h]>            (scale: 1 / sqrt(D) by default)
    out_i[head h] = sum_j softmax_j(e_ij) v_j[head h]     (an empty row gives 0)

``k`` / ``v`` are this rank's source rows, ``kh`` / ``vh`` the received halo rows; the kernels
read them as two sources (never concatenated), each with its own row stride, so ``k`` and ``v``
(and ``kh`` / ``vh``) may be the column halves of one ``[N, 2C]`` buffer. The op does no
communication: the caller exchanges the halo rows (models/transformer_conv.py).

GPU (fp32, C in 64/128/256, heads in 1/2/4/8 with C / heads >= 8): the three kernels of
csrc/kernels/dot_attn_f32.h — forward with a running maximum (k_j and v_j gathered once,
nothing per edge stored), backward destination side (``dq``), backward source side over the
transposed pattern (``dk``, ``dv``; once for the local rows, once for the halo rows). The
backward's ``c_i = <g_i, out_i>`` per head is one elementwise pass over the saved output.
Anything else on the GPU raises ``ValueError``. CPU: the same math in plain PyTorch
autograd at fp64 (the numerics oracle), returned in the input dtype.

With ``edge=`` (``[E, C]``, one row per CSR slot, added to the edge's key and value) the op
runs the edge variant of the three kernels (csrc/kernels/dot_attn_edge_f32.hip) instead: the
forward and the destination side stream the edge rows in slot order, the destination side writes the per-edge
gradient and two weights per slot and head, and the source side reads those weights through
``GatPattern.t_slot``. :func:`dot_attention_parts` / :func:`dot_attention_halo` take no edge
features.

With ``dropout_p > 0`` (PyG's ``TransformerConv(dropout=p)`` in training) the attention
coefficients are dropped after the softmax: ``out_i = sum_j alpha_ij keep_ij / (1 - p) v_j``
with ``alpha`` the softmax over ALL edges of the row. The keep decision of an edge is a
stateless function of ``(seed, CSR slot, head)`` (Philox4x32-10, ``ops/philox.py`` and
``csrc/kernels/philox.h``), so the three kernels of csrc/kernels/dot_attn_drop_f32.hip
regenerate the same mask with none stored (the source side through ``GatPattern.t_slot``) and
the CPU path regenerates it bit for bit. The seed is a 1-element int64 tensor that the kernels
read from device memory: a captured step gets a fresh mask per replay when the caller rewrites
it. Out of scope: dropout together with ``edge=``, in :func:`dot_attention_parts` /
:func:`dot_attention_halo` (the carry forward), in the GAT / GATv2 ops (``philox.h`` is
written so that they can adopt it), in bf16, and a fused feature-dropout epilogue.

The forward can also start from an earlier pass's softmax state (``dot_attn_fwd_carry_f32``),
which gives one softmax over a union of edge sets, one set per launch:
:func:`dot_attention_parts` attends over several edge sets that have their own q / k / v, and
:func:`dot_attention_halo` takes the halo exchange inside the op (a :class:`HaloPlan`), attends
over the interior edges while it is in flight and folds the halo edges in when it lands.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch.autograd import Function

from .. import _native
from .gat import GatPattern

SUPPORTED = "float32, C in (64, 128, 256), heads in (1, 2, 4, 8) with C / heads >= 8"


def shape_ok(C: int, heads: int) -> bool:
    return C in (64, 128, 256) and heads in (1, 2, 4, 8) and (C // 4) // heads >= 2


def _reference(q, k, v, kh, vh, pat: GatPattern, heads: int, scale: float, edge=None,
               keep=None, dropout_p: float = 0.0):
    """The relation's attention output [R, C], differentiable plain PyTorch. ``edge`` [E, C]
    (one row per CSR slot) is added to the gathered key and value rows; ``keep`` [E, heads]
    (bool, one row per CSR slot) drops coefficients after the normalisation, the kept ones
    scaled by ``1 / (1 - dropout_p)``."""
    R, C = pat.R, q.shape[1]
    D = C // heads
    ka = k if kh is None else torch.cat([k[:pat.nsplit], kh], 0)
    va = v if vh is None else torch.cat([v[:pat.nsplit], vh], 0)
    rowptr = pat.rowptr.to(q.device)
    cols = pat.col.long().to(q.device)
    rows = torch.repeat_interleave(torch.arange(R, device=q.device), rowptr[1:] - rowptr[:-1])
    E = rows.numel()
    ke, ve = ka[cols], va[cols]
    if edge is not None:
        ke, ve = ke + edge, ve + edge
    e = (q[rows].view(E, heads, D) * ke.view(E, heads, D)).sum(-1) * scale
    m = torch.full((R, heads), -float("inf"), dtype=e.dtype, device=q.device).index_reduce(
        0, rows, e.detach(), "amax", include_self=True)
    p = torch.exp(e - m[rows])
    den = torch.zeros(R, heads, dtype=e.dtype, device=q.device).index_add(0, rows, p)
    alpha = p / den[rows]
    if keep is not None:
        alpha = alpha * (keep.to(alpha.dtype) / (1.0 - dropout_p))
    msg = (ve.view(E, heads, D) * alpha.unsqueeze(-1)).reshape(E, C)
    return torch.zeros(R, C, dtype=q.dtype, device=q.device).index_add(0, rows, msg)


def _rows(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """``t`` as the kernels can read it (unit column stride, 16-B aligned rows) — itself when
    it already is, e.g. a column half of a [N, 2C] buffer."""
    if t is None:
        return None
    if t.shape[0] == 0 or (t.stride(1) == 1 and t.stride(0) % 4 == 0 and
                           t.stride(0) >= t.shape[1] and t.data_ptr() % 16 == 0):
        return t
    return t.contiguous()


def _out_stats(R: int, C: int, heads: int, device):
    """The forward's ``out [R, C]`` and statistics ``m``, ``l`` ``[R, heads]``, uninitialised."""
    out = torch.empty(R, C, dtype=torch.float32, device=device)
    m = torch.empty(R, heads, dtype=torch.float32, device=device)
    return out, m, torch.empty_like(m)


def _src_side(pat: GatPattern, k, v, kh, vh, bwd_src):
    """``dk, dv, dkh, dvh`` of the backward's source side: the local rows, then the halo rows
    over the tail of the transposed row pointer. ``bwd_src(t_rowptr, k, v, dk, dv)`` runs one
    side's kernel. Rows past the pattern's columns have no entries: their gradient is zero
    (``zeros``; ``empty`` when the kernel writes every row)."""
    C = k.shape[1]

    def side(t_rowptr, ks, vs, ncol):
        alloc = torch.empty if ks.shape[0] == ncol else torch.zeros
        dks = alloc(ks.shape[0], C, dtype=torch.float32, device=ks.device)
        dvs = alloc(ks.shape[0], C, dtype=torch.float32, device=ks.device)
        bwd_src(t_rowptr, ks, vs, dks, dvs)
        return dks, dvs

    if kh is None:
        nloc = pat.nsplit + pat.H
        return (*side(pat.t_rowptr[:nloc + 1], k, v, nloc), None, None)
    return (*side(pat.t_rowptr[:pat.nsplit + 1], k, v, pat.nsplit),
            *side(pat.t_rowptr[pat.nsplit:], kh, vh, pat.H))


class _DotAttnFn(Function):
    @staticmethod
    def forward(ctx, q, k, v, kh, vh, pat: GatPattern, heads: int, scale: float):
        ops = _native.ops()
        q, k, v, kh, vh = (_rows(t) for t in (q, k, v, kh, vh))
        R, C = pat.R, q.shape[1]
        out, m, l = _out_stats(R, C, heads, q.device)
        ops.dot_attn_fwd_f32(pat.rowptr, pat.col, q, k, v, kh, vh, pat.nsplit, out, 0.0, m, l,
                             heads, scale)
        ctx.pat, ctx.heads, ctx.scale = pat, heads, scale
        ctx.save_for_backward(q, k, v, kh, vh, out, m, l)
        return out

    @staticmethod
    def backward(ctx, g):
        q, k, v, kh, vh, out, m, l = ctx.saved_tensors
        pat, Hh, scale = ctx.pat, ctx.heads, ctx.scale
        ops = _native.ops()
        R, C = out.shape
        g = _rows(g)
        # c_i^h = <g_i^h, o_i^h> = sum_j alpha_ij <g_i^h, v_j^h> (out is this call's own sum)
        c = (g * out).reshape(R, Hh, C // Hh).sum(-1)
        dq = torch.empty_like(out)
        ops.dot_attn_bwd_dst_f32(pat.rowptr, pat.col, q, k, v, kh, vh, pat.nsplit, m, l, g, c,
                                 dq, Hh, scale)
        dk, dv, dkh, dvh = _src_side(pat, k, v, kh, vh, lambda rp, ks, vs, dks, dvs:
                                     ops.dot_attn_bwd_src_f32(rp, pat.t_col, q, g, ks, vs, m, l,
                                                              c, dks, dvs, Hh, scale))
        return dq, dk, dv, dkh, dvh, None, None, None


class _DotAttnEdgeFn(Function):
    """The attention with ``edge`` added to key and value (dot_attn_edge_f32.hip). The
    destination side of the backward also writes the per-edge gradient and the per-slot
    weights ``w``, which the source side reads through ``pat.t_slot`` instead of recomputing
    them."""

    @staticmethod
    def forward(ctx, q, k, v, kh, vh, edge, pat: GatPattern, heads: int, scale: float):
        ops = _native.ops()
        q, k, v, kh, vh, edge = (_rows(t) for t in (q, k, v, kh, vh, edge))
        R, C = pat.R, q.shape[1]
        out, m, l = _out_stats(R, C, heads, q.device)
        ops.dot_attn_edge_fwd_f32(pat.rowptr, pat.col, q, k, v, kh, vh, pat.nsplit, edge, out,
                                  0.0, m, l, heads, scale)
        ctx.pat, ctx.heads, ctx.scale = pat, heads, scale
        ctx.save_for_backward(q, k, v, kh, vh, edge, out, m, l)
        return out

    @staticmethod
    def backward(ctx, g):
        q, k, v, kh, vh, edge, out, m, l = ctx.saved_tensors
        pat, Hh, scale = ctx.pat, ctx.heads, ctx.scale
        ops = _native.ops()
        R, C = out.shape
        E = pat.col.numel()
        g = _rows(g)
        c = (g * out).reshape(R, Hh, C // Hh).sum(-1)
        dq = torch.empty_like(out)
        # every slot has exactly one writer (the pattern's rows cover all of its entries)
        dee = torch.empty(E, C, dtype=torch.float32, device=g.device)
        w = torch.empty(E, 2 * Hh, dtype=torch.float32, device=g.device)
        ops.dot_attn_edge_bwd_dst_f32(pat.rowptr, pat.col, q, k, v, kh, vh, pat.nsplit, edge,
                                      m, l, g, c, dq, dee, w, Hh, scale)
        dk, dv, dkh, dvh = _src_side(pat, k, v, kh, vh, lambda rp, ks, vs, dks, dvs:
                                     ops.dot_attn_edge_bwd_src_f32(rp, pat.t_col, pat.t_slot, q,
                                                                   g, w, dks, dvs, Hh, scale))
        return dq, dk, dv, dkh, dvh, dee, None, None, None


class _DotAttnDropFn(Function):
    """The attention with dropout on the coefficients (dot_attn_drop_f32.hip). No mask is
    saved: the seed tensor is, and the backward kernels regenerate the forward's bits from it
    (the source side through ``pat.t_slot``)."""

    @staticmethod
    def forward(ctx, q, k, v, kh, vh, seed, pat: GatPattern, heads: int, scale: float,
                p: float):
        ops = _native.ops()
        q, k, v, kh, vh = (_rows(t) for t in (q, k, v, kh, vh))
        R, C = pat.R, q.shape[1]
        out, m, l = _out_stats(R, C, heads, q.device)
        ops.dot_attn_drop_fwd_f32(pat.rowptr, pat.col, q, k, v, kh, vh, pat.nsplit, out, m, l,
                                  seed, p, heads, scale)
        ctx.pat, ctx.heads, ctx.scale, ctx.p = pat, heads, scale, p
        ctx.save_for_backward(q, k, v, kh, vh, seed, out, m, l)
        return out

    @staticmethod
    def backward(ctx, g):
        q, k, v, kh, vh, seed, out, m, l = ctx.saved_tensors
        pat, Hh, scale, p = ctx.pat, ctx.heads, ctx.scale, ctx.p
        ops = _native.ops()
        R, C = out.shape
        g = _rows(g)
        # c_i^h = <g_i^h, o_i^h> = sum_j alpha_ij m'_ij <g_i^h, v_j^h>: still the saved output's
        c = (g * out).reshape(R, Hh, C // Hh).sum(-1)
        dq = torch.empty_like(out)
        ops.dot_attn_drop_bwd_dst_f32(pat.rowptr, pat.col, q, k, v, kh, vh, pat.nsplit, m, l, g,
                                      c, dq, seed, p, Hh, scale)
        dk, dv, dkh, dvh = _src_side(pat, k, v, kh, vh, lambda rp, ks, vs, dks, dvs:
                                     ops.dot_attn_drop_bwd_src_f32(rp, pat.t_col, pat.t_slot, q,
                                                                   g, ks, vs, m, l, c, dks, dvs,
                                                                   seed, p, Hh, scale))
        return dq, dk, dv, dkh, dvh, None, None, None, None, None


def dot_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, pat: GatPattern,
                  kh: Optional[torch.Tensor] = None, vh: Optional[torch.Tensor] = None,
                  scale: Optional[float] = None, *, heads: int = 1,
                  edge: Optional[torch.Tensor] = None, dropout_p: float = 0.0,
                  dropout_seed: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out[R, C]`` of the scaled dot-product attention of ``q [R, C]`` over ``pat``
    (autograd). Columns below ``pat.nsplit`` read ``k`` / ``v``, the others row
    ``column - pat.nsplit`` of ``kh`` / ``vh`` (without them: ``k`` / ``v`` hold every
    column's row). ``heads`` is a keyword argument (the tensors stay 2-D, heads are
    contiguous column blocks); ``scale`` defaults to ``1 / sqrt(C / heads)``.

    ``edge [E, C]`` (fp32 on the GPU): one row per CSR slot of ``pat`` (the order of
    ``pat.col``), added to the edge's key and to its value (PyG's ``TransformerConv`` with
    ``edge_dim``); its gradient is returned like any other. Without it nothing changes.

    ``dropout_p`` in ``(0, 1)``: dropout on the attention coefficients, after the softmax
    (the module docstring). ``dropout_seed``: a 1-element int64 tensor on ``q``'s device that
    fixes the mask; ``None`` draws one from the device's torch generator (reproducible under
    ``torch.manual_seed``, no host sync). ``dropout_p = 0`` (the default) is exactly the call
    without the two arguments; the seed is then ignored. Not available with ``edge=``."""
    heads = int(heads)
    dropout_p = float(dropout_p)
    if not 0.0 <= dropout_p < 1.0:
        raise ValueError(f"dot_attention: dropout_p must lie in [0, 1), got {dropout_p}")
    if dropout_p > 0.0 and edge is not None:
        raise ValueError("dot_attention: dropout_p > 0 together with edge= is not supported "
                         "(the edge-feature kernels take no dropout)")
    if q.dim() != 2 or k.dim() != 2 or k.shape != v.shape or k.shape[1] != q.shape[1]:
        raise ValueError("dot_attention: q [R, C] and k, v [N, C] expected")
    C = q.shape[1]
    if heads < 1 or C % heads:
        raise ValueError(f"dot_attention: width {C} is not divisible by heads {heads}")
    if (kh is None) != (vh is None):
        raise ValueError("dot_attention: kh and vh come together")
    if q.shape[0] != pat.R:
        raise ValueError(f"dot_attention: q has {q.shape[0]} rows, the pattern {pat.R}")
    if kh is None:
        if k.shape[0] < pat.nsplit + pat.H:
            raise ValueError("dot_attention: k / v have fewer rows than the pattern's columns")
    elif k.shape[0] != pat.nsplit or kh.shape[0] < pat.H or kh.shape != vh.shape or \
            kh.shape[1] != C:
        raise ValueError("dot_attention: k / v must have pat.nsplit rows and kh / vh the "
                         "pattern's halo rows")
    if edge is not None and (edge.dim() != 2 or edge.shape[0] != pat.col.numel() or
                             edge.shape[1] != C):
        raise ValueError(f"dot_attention: edge must be [{pat.col.numel()}, {C}] (one row per "
                         f"entry of the pattern), got {tuple(edge.shape)}")
    if scale is None:
        scale = 1.0 / math.sqrt(C // heads)
    scale = float(scale)
    if dropout_p > 0.0:
        if dropout_seed is None:
            dropout_seed = torch.randint(0, 2 ** 62, (1,), device=q.device)
        elif not isinstance(dropout_seed, torch.Tensor) or dropout_seed.numel() != 1 or \
                dropout_seed.dtype != torch.int64 or dropout_seed.device != q.device:
            raise ValueError("dot_attention: dropout_seed must be a 1-element int64 tensor on "
                             f"{q.device}")
    if not q.is_cuda:
        dt = q.dtype
        up = lambda t: None if t is None else t.double()  # noqa: E731
        if dropout_p > 0.0:
            from .philox import attn_keep_mask

            keep = attn_keep_mask(dropout_seed, pat.col.numel(), heads, dropout_p)
            return _reference(up(q), up(k), up(v), up(kh), up(vh), pat, heads, scale,
                              keep=keep, dropout_p=dropout_p).to(dt)
        if edge is None:
            return _reference(up(q), up(k), up(v), up(kh), up(vh), pat, heads, scale).to(dt)
        return _reference(up(q), up(k), up(v), up(kh), up(vh), pat, heads, scale,
                          up(edge)).to(dt)
    if any(t is not None and t.dtype != torch.float32 for t in (q, k, v, kh, vh)) or \
            not shape_ok(C, heads):
        raise ValueError(f"dot_attention: unsupported on the GPU: dtype {q.dtype}, C = {C}, "
                         f"heads = {heads} (supported: {SUPPORTED})")
    if dropout_p > 0.0:
        return _DotAttnDropFn.apply(q, k, v, kh, vh, dropout_seed.reshape(1), pat, heads,
                                    scale, dropout_p)
    if edge is None:
        return _DotAttnFn.apply(q, k, v, kh, vh, pat, heads, scale)
    if edge.dtype != torch.float32:
        raise ValueError(f"dot_attention: unsupported on the GPU: edge dtype {edge.dtype} "
                         f"(supported: {SUPPORTED})")
    return _DotAttnEdgeFn.apply(q, k, v, kh, vh, edge, pat, heads, scale)


# ------------------------------------------------------- one softmax over several edge sets
def _reference_parts(parts, heads: int, scale: float):
    """One softmax per destination and head over the union of the parts' edges
    (differentiable plain PyTorch); ``parts``: ``(q, k, v, pat)`` with one-source patterns."""
    q0, pat0 = parts[0][0], parts[0][3]
    R, C = pat0.R, q0.shape[1]
    D = C // heads
    dev = q0.device
    es, vs, rs = [], [], []
    for q, k, v, pat in parts:
        rowptr = pat.rowptr.to(dev)
        cols = pat.col.long().to(dev)
        rows = torch.repeat_interleave(torch.arange(R, device=dev), rowptr[1:] - rowptr[:-1])
        E = rows.numel()
        es.append((q[rows].view(E, heads, D) * k[cols].view(E, heads, D)).sum(-1) * scale)
        vs.append(v[cols].view(E, heads, D))
        rs.append(rows)
    e, ve, rows = torch.cat(es), torch.cat(vs), torch.cat(rs)
    m = torch.full((R, heads), -float("inf"), dtype=e.dtype, device=dev).index_reduce(
        0, rows, e.detach(), "amax", include_self=True)
    p = torch.exp(e - m[rows])
    den = torch.zeros(R, heads, dtype=e.dtype, device=dev).index_add(0, rows, p)
    alpha = p / den[rows]
    msg = (ve * alpha.unsqueeze(-1)).reshape(-1, C)
    return torch.zeros(R, C, dtype=q0.dtype, device=dev).index_add(0, rows, msg)


class _DotAttnPartsFn(Function):
    """The plain forward over the first part, the carry forward over each further part on the
    same (out, m, l); the backward kernels recompute alpha per edge from the final m, 1 / l
    and c, so they run per part as they are."""

    @staticmethod
    def forward(ctx, pats, heads: int, scale: float, *qkv):
        ops = _native.ops()
        qkv = tuple(_rows(t) for t in qkv)
        R, C = pats[0].R, qkv[0].shape[1]
        dev = qkv[0].device
        out, m, l = _out_stats(R, C, heads, dev)
        for p, pat in enumerate(pats):
            q, k, v = qkv[3 * p:3 * p + 3]
            if p == 0:
                ops.dot_attn_fwd_f32(pat.rowptr, pat.col, q, k, v, None, None, pat.nsplit, out,
                                     0.0, m, l, heads, scale)
            else:
                ops.dot_attn_fwd_carry_f32(pat.rowptr, pat.col, q, k, v, None, None,
                                           pat.nsplit, out, m, l, heads, scale)
        ctx.pats, ctx.heads, ctx.scale = pats, heads, scale
        ctx.save_for_backward(out, m, l, *qkv)
        return out

    @staticmethod
    def backward(ctx, g):
        out, m, l, *qkv = ctx.saved_tensors
        Hh, scale = ctx.heads, ctx.scale
        ops = _native.ops()
        R, C = out.shape
        g = _rows(g)
        c = (g * out).reshape(R, Hh, C // Hh).sum(-1)  # of the final out: all parts' edges
        grads = []
        for p, pat in enumerate(ctx.pats):
            q, k, v = qkv[3 * p:3 * p + 3]
            dq = torch.empty_like(out)
            ops.dot_attn_bwd_dst_f32(pat.rowptr, pat.col, q, k, v, None, None, pat.nsplit, m, l,
                                     g, c, dq, Hh, scale)
            ncol = pat.nsplit + pat.H  # rows past the pattern's columns have no entries
            alloc = torch.empty if k.shape[0] == ncol else torch.zeros
            dk = alloc(k.shape[0], C, dtype=torch.float32, device=g.device)
            dv = alloc(k.shape[0], C, dtype=torch.float32, device=g.device)
            ops.dot_attn_bwd_src_f32(pat.t_rowptr[:ncol + 1], pat.t_col, q, g, k, v, m, l, c,
                                     dk, dv, Hh, scale)
            grads += [dq, dk, dv]
        return (None, None, None, *grads)


def dot_attention_parts(parts, scale: Optional[float] = None, *, heads: int = 1) -> torch.Tensor:
    """``out[R, C]``: attention with ONE softmax per destination row and head over the union
    of several edge sets, each with its own operands (autograd reaches all of them).

    ``parts``: a sequence of ``(q_p [R, C], k_p [N_p, C], v_p [N_p, C], pat_p)``; every
    ``pat_p`` is a pattern over the same ``R`` rows whose columns all read ``k_p`` / ``v_p``.
    ``out_i[h] = sum_p sum_{j in pat_p(i)} alpha v_p,j[h]`` with ``alpha`` the softmax over
    all those edges of ``scale <q_p,i[h], k_p,j[h]>``. GPU: the plain forward over the first
    part, the carry forward (``dot_attn_fwd_carry_f32``) over each further one. A single part
    is :func:`dot_attention` on that pattern."""
    heads = int(heads)
    parts = [tuple(p) for p in parts]
    if not parts or any(len(p) != 4 for p in parts):
        raise ValueError("dot_attention_parts: a non-empty sequence of (q, k, v, pattern)")
    R, C = parts[0][3].R, parts[0][0].shape[-1]
    for q, k, v, pat in parts:
        if q.dim() != 2 or k.dim() != 2 or k.shape != v.shape or k.shape[1] != q.shape[1] or \
                q.shape[1] != C:
            raise ValueError("dot_attention_parts: q [R, C] and k, v [N, C] of one width "
                             "expected in every part")
        if pat.R != R or q.shape[0] != R:
            raise ValueError("dot_attention_parts: every part's q and pattern must have the "
                             f"same {R} rows")
        if k.shape[0] < pat.nsplit + pat.H:
            raise ValueError("dot_attention_parts: k / v have fewer rows than the pattern's "
                             "columns")
    if heads < 1 or C % heads:
        raise ValueError(f"dot_attention_parts: width {C} is not divisible by heads {heads}")
    if scale is None:
        scale = 1.0 / math.sqrt(C // heads)
    scale = float(scale)
    q0 = parts[0][0]
    tensors = [t for p in parts for t in p[:3]]
    if not q0.is_cuda:
        dt = q0.dtype
        up = [(q.double(), k.double(), v.double(), pat) for q, k, v, pat in parts]
        return _reference_parts(up, heads, scale).to(dt)
    if any(t.dtype != torch.float32 for t in tensors) or not shape_ok(C, heads):
        raise ValueError(f"dot_attention_parts: unsupported on the GPU: dtype {q0.dtype}, "
                         f"C = {C}, heads = {heads} (supported: {SUPPORTED})")
    return _DotAttnPartsFn.apply(tuple(p[3] for p in parts), heads, scale, *tensors)


# ------------------------------------------------- attention with the halo exchange inside
class _PlanExchangeFn(Function):
    """The plan's all-to-all-v, synchronous; backward: its reverse."""

    @staticmethod
    def forward(ctx, send, plan):
        ctx.plan = plan
        return plan.a2a(send.contiguous())

    @staticmethod
    def backward(ctx, g):
        return ctx.plan.a2a_rev(g.contiguous()), None


class HaloPlan:
    """What one halo exchange of a relation needs, built once: the forward all-to-all-v
    (``a2a``), its reverse (``a2a_rev``) and the send rows' :class:`IndexMap` (``send_map``:
    its transposed segment sum adds the returned gradients without atomics).

    ``HaloPlan(a2a, send_idx, num_rows)`` wraps an :class:`AllToAllV` directly (one process
    can drive it over the loopback transport); :meth:`from_pattern` takes them from a
    communication pattern, sharing the objects :class:`~dgraph_amd.parallel.halo.AsyncHalo`
    caches on it. ``a2a`` is ``None`` for an engine without an asynchronous all-to-all-v."""

    def __init__(self, a2a, send_idx=None, num_rows: int = 0, *, a2a_rev=None, send_map=None,
                 comm=None, pattern=None):
        from .csr import IndexMap

        self.a2a = a2a
        self.a2a_rev = a2a_rev if a2a_rev is not None or a2a is None else a2a.reversed()
        self.send_map = send_map if send_map is not None else IndexMap(send_idx, num_rows)
        self.comm, self.pattern = comm, pattern

    @staticmethod
    def from_pattern(comm, pattern, num_rows: int) -> "HaloPlan":
        from ..parallel.halo import _send_map

        engine = getattr(comm, "_engine", None)
        a2a = rev = None
        if engine is not None and hasattr(engine, "alltoallv"):
            a2a = pattern._cache.get("a2a")
            if a2a is None:
                a2a = engine.alltoallv(pattern.send_splits(), pattern.recv_splits())
                pattern._cache["a2a"] = a2a
                pattern._cache["a2a_rev"] = a2a.reversed()
            rev = pattern._cache["a2a_rev"]
        return HaloPlan(a2a, a2a_rev=rev, send_map=_send_map(pattern, num_rows), comm=comm,
                        pattern=pattern)

    def exchange(self, x: torch.Tensor) -> torch.Tensor:
        """The synchronous, autograd-aware exchange of ``x``'s send rows -> the halo rows."""
        if self.comm is not None:
            from ..parallel.halo import HaloExchange

            return HaloExchange(self.comm)(x, self.pattern)
        from .aggregate import gather

        return _PlanExchangeFn.apply(gather(x, self.send_map), self)


class _DotAttnHaloFn(Function):
    """Both exchanges of the relation's ``[k | v]`` rows live in this one Function: the
    interior edges are attended over while the forward exchange is on the links (the halo
    edges are folded in by the carry forward), and in backward the halo rows' gradient is
    computed first so its reverse exchange runs under ``dq`` and the local ``dk`` / ``dv``.
    Every call issues exactly one exchange forward and one backward, whatever this rank
    sends or receives."""

    @staticmethod
    def forward(ctx, q, kv, pat: GatPattern, plan: HaloPlan, heads: int, scale: float):
        from . import kernels as K

        ops = _native.ops()
        q, kv = _rows(q), _rows(kv)
        R, C = pat.R, q.shape[1]
        send = K.gather_rows(kv, plan.send_map.idx)
        recv, work = plan.a2a(send, async_op=True)
        inner, outer = pat.split()
        out, m, l = _out_stats(R, C, heads, q.device)
        ops.dot_attn_fwd_f32(inner.rowptr, inner.col, q, kv[:, :C], kv[:, C:], None, None,
                             inner.nsplit, out, 0.0, m, l, heads, scale)
        work.wait()
        ops.dot_attn_fwd_carry_f32(outer.rowptr, outer.col, q, recv[:, :C], recv[:, C:], None,
                                   None, outer.nsplit, out, m, l, heads, scale)
        ctx.pat, ctx.plan, ctx.heads, ctx.scale = pat, plan, heads, scale
        ctx.save_for_backward(q, kv, recv, out, m, l)
        return out

    @staticmethod
    def backward(ctx, g):
        from . import kernels as K

        q, kv, recv, out, m, l = ctx.saved_tensors
        pat, plan, Hh, scale = ctx.pat, ctx.plan, ctx.heads, ctx.scale
        ops = _native.ops()
        R, C = out.shape
        Ns, H = pat.nsplit, pat.H
        g = _rows(g)
        c = (g * out).reshape(R, Hh, C // Hh).sum(-1)
        # the halo rows first: their gradient goes back to the owners under what follows
        gh = torch.empty(H, 2 * C, dtype=torch.float32, device=g.device)
        ops.dot_attn_bwd_src_f32(pat.t_rowptr[Ns:], pat.t_col, q, g, recv[:, :C], recv[:, C:],
                                 m, l, c, gh[:, :C], gh[:, C:], Hh, scale)
        back, work = plan.a2a_rev(gh, async_op=True)
        dq = torch.empty_like(out)
        kh, vh = (recv[:, :C], recv[:, C:]) if H else (None, None)
        ops.dot_attn_bwd_dst_f32(pat.rowptr, pat.col, q, kv[:, :C], kv[:, C:], kh, vh, Ns, m, l,
                                 g, c, dq, Hh, scale)
        gkv = torch.empty(Ns, 2 * C, dtype=torch.float32, device=g.device)
        ops.dot_attn_bwd_src_f32(pat.t_rowptr[:Ns + 1], pat.t_col, q, g, kv[:, :C], kv[:, C:],
                                 m, l, c, gkv[:, :C], gkv[:, C:], Hh, scale)
        work.wait()
        st = plan.send_map.transpose_csr()  # a row sent to several peers: a fixed-order sum
        K.spmm(st.rowptr, st.col, back, gkv, beta=1.0)
        return dq, gkv, None, None, None, None


def dot_attention_halo(q: torch.Tensor, kv: torch.Tensor, pat: GatPattern, plan: HaloPlan,
                       scale: Optional[float] = None, *, heads: int = 1) -> torch.Tensor:
    """:func:`dot_attention` of ``q [R, C]`` over ``pat`` with this rank's ``kv [Ns, 2C]``
    (``[k | v]`` rows of its ``Ns = pat.nsplit`` local sources) and the halo rows fetched
    through ``plan`` inside the op (autograd; one exchange forward, one backward, on every
    rank of the plan whether or not it sends or receives rows).

    GPU fp32 with an asynchronous all-to-all-v: the interior edges are attended over while
    the exchange is in flight and the halo edges folded in when it lands; in backward the
    reverse exchange runs under ``dq`` and the local rows' ``dk`` / ``dv``. Otherwise (CPU
    tensors, an engine without an asynchronous all-to-all-v): the synchronous exchange, then
    :func:`dot_attention` — the same result, nothing overlapped."""
    heads = int(heads)
    if q.dim() != 2 or kv.dim() != 2 or kv.shape[1] != 2 * q.shape[1]:
        raise ValueError("dot_attention_halo: q [R, C] and kv [Ns, 2C] expected")
    C = q.shape[1]
    if heads < 1 or C % heads:
        raise ValueError(f"dot_attention_halo: width {C} is not divisible by heads {heads}")
    if q.shape[0] != pat.R or kv.shape[0] != pat.nsplit:
        raise ValueError("dot_attention_halo: q must have the pattern's rows and kv its "
                         f"{pat.nsplit} local source rows")
    if plan.send_map.num_src != kv.shape[0]:
        raise ValueError("dot_attention_halo: the plan's send rows index another row count")
    if plan.a2a is not None and plan.a2a.total_recv != pat.H:
        raise ValueError(f"dot_attention_halo: the plan receives {plan.a2a.total_recv} rows, "
                         f"the pattern has {pat.H} halo rows")
    if not q.is_cuda or plan.a2a is None:
        halo = plan.exchange(kv)
        return dot_attention(q, kv[:, :C], kv[:, C:], pat, halo[:, :C], halo[:, C:], scale,
                             heads=heads)
    if q.dtype != torch.float32 or kv.dtype != torch.float32 or not shape_ok(C, heads):
        raise ValueError(f"dot_attention_halo: unsupported on the GPU: dtype {q.dtype}, "
                         f"C = {C}, heads = {heads} (supported: {SUPPORTED})")
    if scale is None:
        scale = 1.0 / math.sqrt(C // heads)
    return _DotAttnHaloFn.apply(q, kv, pat, plan, heads, float(scale))
