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
csrc/kernels/dot_attn_f32.hip — forward with a running maximum (k_j and v_j gathered once,
nothing per edge stored), backward destination side (``dq``), backward source side over the
transposed pattern (``dk``, ``dv``; once for the local rows, once for the halo rows). The
backward's ``c_i = <g_i, out_i>`` per head is one elementwise pass over the saved output.
Anything else on the GPU raises ``ValueError``. CPU: the same math in plain PyTorch
autograd at fp64 (the numerics oracle), returned in the input dtype.
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


def _reference(q, k, v, kh, vh, pat: GatPattern, heads: int, scale: float):
    """The relation's attention output [R, C], differentiable plain PyTorch."""
    R, C = pat.R, q.shape[1]
    D = C // heads
    ka = k if kh is None else torch.cat([k[:pat.nsplit], kh], 0)
    va = v if vh is None else torch.cat([v[:pat.nsplit], vh], 0)
    rowptr = pat.rowptr.to(q.device)
    cols = pat.col.long().to(q.device)
    rows = torch.repeat_interleave(torch.arange(R, device=q.device), rowptr[1:] - rowptr[:-1])
    E = rows.numel()
    e = (q[rows].view(E, heads, D) * ka[cols].view(E, heads, D)).sum(-1) * scale
    m = torch.full((R, heads), -float("inf"), dtype=e.dtype, device=q.device).index_reduce(
        0, rows, e.detach(), "amax", include_self=True)
    p = torch.exp(e - m[rows])
    den = torch.zeros(R, heads, dtype=e.dtype, device=q.device).index_add(0, rows, p)
    alpha = p / den[rows]
    msg = (va[cols].view(E, heads, D) * alpha.unsqueeze(-1)).reshape(E, C)
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


class _DotAttnFn(Function):
    @staticmethod
    def forward(ctx, q, k, v, kh, vh, pat: GatPattern, heads: int, scale: float):
        ops = _native.ops()
        q, k, v, kh, vh = (_rows(t) for t in (q, k, v, kh, vh))
        R, C = pat.R, q.shape[1]
        out = torch.empty(R, C, dtype=torch.float32, device=q.device)
        m = torch.empty(R, heads, dtype=torch.float32, device=q.device)
        l = torch.empty_like(m)
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
        # the source side: the local rows, then the halo rows over the tail of the transposed
        # row pointer; rows past the pattern's columns have no entries
        nloc = pat.nsplit if kh is not None else pat.nsplit + pat.H
        alloc = torch.empty if k.shape[0] == nloc else torch.zeros
        dk = alloc(k.shape[0], C, dtype=torch.float32, device=g.device)
        dv = alloc(k.shape[0], C, dtype=torch.float32, device=g.device)
        ops.dot_attn_bwd_src_f32(pat.t_rowptr[:nloc + 1], pat.t_col, q, g, k, v, m, l, c, dk,
                                 dv, Hh, scale)
        dkh = dvh = None
        if kh is not None:
            alloc = torch.empty if kh.shape[0] == pat.H else torch.zeros
            dkh = alloc(kh.shape[0], C, dtype=torch.float32, device=g.device)
            dvh = alloc(kh.shape[0], C, dtype=torch.float32, device=g.device)
            ops.dot_attn_bwd_src_f32(pat.t_rowptr[pat.nsplit:], pat.t_col, q, g, kh, vh, m, l,
                                     c, dkh, dvh, Hh, scale)
        return dq, dk, dv, dkh, dvh, None, None, None


def dot_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, pat: GatPattern,
                  kh: Optional[torch.Tensor] = None, vh: Optional[torch.Tensor] = None,
                  scale: Optional[float] = None, *, heads: int = 1) -> torch.Tensor:
    """``out[R, C]`` of the scaled dot-product attention of ``q [R, C]`` over ``pat``
    (autograd). Columns below ``pat.nsplit`` read ``k`` / ``v``, the others row
    ``column - pat.nsplit`` of ``kh`` / ``vh`` (without them: ``k`` / ``v`` hold every
    column's row). ``heads`` is a keyword argument (the tensors stay 2-D, heads are
    contiguous column blocks); ``scale`` defaults to ``1 / sqrt(C / heads)``."""
    heads = int(heads)
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
    if scale is None:
        scale = 1.0 / math.sqrt(C // heads)
    scale = float(scale)
    if not q.is_cuda:
        dt = q.dtype
        up = lambda t: None if t is None else t.double()  # noqa: E731
        return _reference(up(q), up(k), up(v), up(kh), up(vh), pat, heads, scale).to(dt)
    if any(t is not None and t.dtype != torch.float32 for t in (q, k, v, kh, vh)) or \
            not shape_ok(C, heads):
        raise ValueError(f"dot_attention: unsupported on the GPU: dtype {q.dtype}, C = {C}, "
                         f"heads = {heads} (supported: {SUPPORTED})")
    return _DotAttnFn.apply(q, k, v, kh, vh, pat, heads, scale)
