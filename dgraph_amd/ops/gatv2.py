"""Fused fp32 GATv2 graph attention with its exact adjoint (GATv2Conv; Brody et al., "How
attentive are graph attention networks?").

For one relation (destination rows i, source columns j over ``[local sources | halo rows]``)
and per head h (channels ``[hD, (h+1)D)`` of ``C = heads * D``)::

    e_ij  = sum_{c in head h} att_c * LeakyReLU(xd_i + xs_j)_c
    out_i[head h] = sum_j softmax_j(e_ij) xs_j[head h]      (an empty row gives 0)

``xd`` are the destination-transformed rows, ``xs`` this rank's source-transformed rows and
``xsh`` the received halo rows; the kernels read the latter two as two sources (never
concatenated), each operand with its own row stride, so ``xd`` and ``xs`` may be the column
halves of one ``[N, 2C]`` buffer. The nonlinearity sits inside the projection, so the score
does not split into a destination scalar plus a source scalar (ops/gat.py): it needs the
whole ``xs_j`` row per edge — which is also the message. The op does no communication: the
caller exchanges the halo rows (models/gatv2_conv.py).

GPU (fp32, C in 64/128/256, heads in 1/2/4/8 with C / heads >= 8): the three kernels of
csrc/kernels/gatv2_f32.hip — forward with a running maximum (``xs_j`` gathered once, nothing
per edge stored), backward destination side (``dxd`` and the partial rows of ``datt``, summed
by the fixed-order column sum), backward source side over the transposed pattern (``dxs``;
once for the local rows, once for the halo rows). The backward's ``c_i = <g_i, out_i>`` per
head is one elementwise pass over the saved output. Anything else on the GPU raises
``ValueError``. CPU: the same math in plain PyTorch autograd at fp64 (the numerics oracle),
returned in the input dtype.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F
from torch.autograd import Function

from .. import _native
from .dot_attn import _rows, shape_ok
from .gat import GatPattern

SUPPORTED = "float32, C in (64, 128, 256), heads in (1, 2, 4, 8) with C / heads >= 8"


def _reference(xd, xs, xsh, att, pat: GatPattern, heads: int, slope: float):
    """The relation's attention output [R, C], differentiable plain PyTorch."""
    R, C = pat.R, xd.shape[1]
    D = C // heads
    ra = xs if xsh is None else torch.cat([xs[:pat.nsplit], xsh], 0)
    rowptr = pat.rowptr.to(xd.device)
    cols = pat.col.long().to(xd.device)
    rows = torch.repeat_interleave(torch.arange(R, device=xd.device), rowptr[1:] - rowptr[:-1])
    E = rows.numel()
    re = ra[cols]
    act = F.leaky_relu(xd[rows] + re, slope)  # (its derivative at 0 is ``slope``)
    e = (act.view(E, heads, D) * att.view(1, heads, D)).sum(-1)
    m = torch.full((R, heads), -float("inf"), dtype=e.dtype, device=xd.device).index_reduce(
        0, rows, e.detach(), "amax", include_self=True)
    p = torch.exp(e - m[rows])
    den = torch.zeros(R, heads, dtype=e.dtype, device=xd.device).index_add(0, rows, p)
    alpha = p / den[rows]
    msg = (re.view(E, heads, D) * alpha.unsqueeze(-1)).reshape(E, C)
    return torch.zeros(R, C, dtype=xd.dtype, device=xd.device).index_add(0, rows, msg)


class _GATv2Fn(Function):
    @staticmethod
    def forward(ctx, xd, xs, xsh, att, pat: GatPattern, heads: int, slope: float):
        ops = _native.ops()
        xd, xs, xsh = (_rows(t) for t in (xd, xs, xsh))
        if att.data_ptr() % 16 or not att.is_contiguous():
            att = att.contiguous().clone()
        R, C = pat.R, xd.shape[1]
        out = torch.empty(R, C, dtype=torch.float32, device=xd.device)
        m = torch.empty(R, heads, dtype=torch.float32, device=xd.device)
        l = torch.empty_like(m)
        ops.gatv2_fwd_f32(pat.rowptr, pat.col, xd, xs, xsh, pat.nsplit, att, out, 0.0, m, l,
                          heads, slope)
        ctx.pat, ctx.heads, ctx.slope = pat, heads, slope
        ctx.save_for_backward(xd, xs, xsh, att, out, m, l)
        return out

    @staticmethod
    def backward(ctx, g):
        xd, xs, xsh, att, out, m, l = ctx.saved_tensors
        pat, Hh, slope = ctx.pat, ctx.heads, ctx.slope
        ops = _native.ops()
        R, C = out.shape
        g = _rows(g)
        # c_i^h = <g_i^h, o_i^h> = sum_j alpha_ij <g_i^h, xs_j^h> (out is this call's own sum)
        c = (g * out).reshape(R, Hh, C // Hh).sum(-1)
        dxd = torch.empty_like(out)
        # datt leaves the kernel as one partial row per workgroup (fixed partition)
        P = ops.gatv2_da_parts(R, C)
        da_part = torch.empty(P, C, dtype=torch.float32, device=g.device)
        ops.gatv2_bwd_dst_f32(pat.rowptr, pat.col, xd, xs, xsh, pat.nsplit, att, m, l, g, c,
                              dxd, da_part, Hh, slope)
        datt = ops.col_sum(da_part) if P else torch.zeros(C, dtype=torch.float32,
                                                          device=g.device)
        # the source side: the local rows, then the halo rows over the tail of the transposed
        # row pointer; rows past the pattern's columns have no entries
        nloc = pat.nsplit if xsh is not None else pat.nsplit + pat.H
        alloc = torch.empty if xs.shape[0] == nloc else torch.zeros
        dxs = alloc(xs.shape[0], C, dtype=torch.float32, device=g.device)
        ops.gatv2_bwd_src_f32(pat.t_rowptr[:nloc + 1], pat.t_col, xd, g, xs, att, m, l, c, dxs,
                              Hh, slope)
        dxsh = None
        if xsh is not None:
            alloc = torch.empty if xsh.shape[0] == pat.H else torch.zeros
            dxsh = alloc(xsh.shape[0], C, dtype=torch.float32, device=g.device)
            ops.gatv2_bwd_src_f32(pat.t_rowptr[pat.nsplit:], pat.t_col, xd, g, xsh, att, m, l,
                                  c, dxsh, Hh, slope)
        return dxd, dxs, dxsh, datt, None, None, None


def gatv2_attention(xd: torch.Tensor, xs: torch.Tensor, att: torch.Tensor, pat: GatPattern,
                    xsh: Optional[torch.Tensor] = None, *, heads: int = 1,
                    negative_slope: float = 0.2) -> torch.Tensor:
    """``out[R, C]`` of the GATv2 attention of ``xd [R, C]`` over ``pat`` (autograd in ``xd``,
    ``xs``, ``xsh`` and ``att``). Columns below ``pat.nsplit`` read ``xs``, the others row
    ``column - pat.nsplit`` of ``xsh`` (without it: ``xs`` holds every column's row). ``att``
    is ``[C]`` or ``[heads, D]``; ``heads`` is a keyword argument (the tensors stay 2-D, heads
    are contiguous column blocks)."""
    heads = int(heads)
    if xd.dim() != 2 or xs.dim() != 2 or xs.shape[1] != xd.shape[1]:
        raise ValueError("gatv2_attention: xd [R, C] and xs [N, C] expected")
    C = xd.shape[1]
    if heads < 1 or C % heads:
        raise ValueError(f"gatv2_attention: width {C} is not divisible by heads {heads}")
    if att.numel() != C or tuple(att.shape) not in ((C,), (heads, C // heads)):
        raise ValueError(f"gatv2_attention: att must be [{C}] or [{heads}, {C // heads}], got "
                         f"{tuple(att.shape)}")
    if xd.shape[0] != pat.R:
        raise ValueError(f"gatv2_attention: xd has {xd.shape[0]} rows, the pattern {pat.R}")
    if xsh is None:
        if xs.shape[0] < pat.nsplit + pat.H:
            raise ValueError("gatv2_attention: xs has fewer rows than the pattern's columns "
                             "(halo columns need xsh)")
    elif xs.shape[0] != pat.nsplit or xsh.dim() != 2 or xsh.shape[0] < pat.H or \
            xsh.shape[1] != C:
        raise ValueError("gatv2_attention: xs must have pat.nsplit rows and xsh the "
                         "pattern's halo rows")
    slope = float(negative_slope)
    a = att.reshape(C)
    if not xd.is_cuda:
        dt = xd.dtype
        up = lambda t: None if t is None else t.double()  # noqa: E731
        return _reference(up(xd), up(xs), up(xsh), up(a), pat, heads, slope).to(dt)
    if any(t is not None and t.dtype != torch.float32 for t in (xd, xs, xsh, att)) or \
            not shape_ok(C, heads):
        raise ValueError(f"gatv2_attention: unsupported on the GPU: dtype {xd.dtype}, C = {C}, "
                         f"heads = {heads} (supported: {SUPPORTED})")
    return _GATv2Fn.apply(xd, xs, xsh, a, pat, heads, slope)
