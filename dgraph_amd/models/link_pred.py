"""Link prediction on top of the per-edge dot product: an inner-product decoder, GAE's
reconstruction loss and structured negatives.

* :class:`InnerProductDecoder` scores every entry of a pattern as ``<z_i, z_j>`` per head
  (:func:`~dgraph_amd.ops.aggregate.edge_dot`, or
  :func:`~dgraph_amd.parallel.dist_graph.dist_edge_dot` on a :class:`DistGraph`, where ``z_j``
  may be a halo row). On the GPU that is one kernel that writes nothing per edge but the
  scores, and a backward of two edge-weighted SpMMs; ``z`` takes both gradients.
* :func:`recon_loss` is the binary cross-entropy with logits over the scores of a positive and
  of a negative pattern (Kipf & Welling, "Variational Graph Auto-Encoders", 2016, without the
  KL term). The elementwise loss is plain torch on ``[nnz, heads]`` scores.
* :func:`negative_pattern` draws ``k`` uniformly random columns for every non-empty row of a
  pattern and returns them as a :class:`CSR`: negatives with the positives' row structure,
  built on the host once and then scored exactly like the positives.

Out of scope here: edge-score functions other than the dot product (add, L2 distance, MLP
decoders), a fused score-plus-loss kernel, double backward, a column-chunked halo exchange of
the distributed score, negatives that cross partitions (a :class:`DistGraph` of negatives is
the caller's to build), and the wiring into ``GraphSAGE``, the fused executor or ``bench.py``.
"""
from __future__ import annotations

from typing import Optional, Union

import torch
import torch.nn as nn
import torch.nn.functional as Fn

from ..ops.aggregate import edge_dot
from ..ops.csr import CSR
from ..parallel.dist_graph import DistGraph, dist_edge_dot


class InnerProductDecoder(nn.Module):
    """``forward(z, pattern)``: ``[nnz, heads]`` scores ``<z_i^h, z_j^h>`` of the pattern's
    entries ``(i, j)`` (``heads`` equal column slices of ``z``), in CSR slot order; for a
    :class:`DistGraph` the interior block's scores, then the halo block's. ``sigmoid=True``
    returns probabilities instead of logits."""

    def __init__(self, heads: int = 1):
        super().__init__()
        self.heads = int(heads)

    def forward(self, z: torch.Tensor, pattern: Union[CSR, DistGraph],
                sigmoid: bool = False) -> torch.Tensor:
        if isinstance(pattern, DistGraph):
            s = dist_edge_dot(z, z, pattern, heads=self.heads)
        else:
            s = edge_dot(z, z, pattern, heads=self.heads)
        return torch.sigmoid(s) if sigmoid else s


def recon_loss(z: torch.Tensor, pos: Union[CSR, DistGraph], neg: Union[CSR, DistGraph],
               decoder: Optional[InnerProductDecoder] = None) -> torch.Tensor:
    """GAE's reconstruction loss: ``mean(-log sigmoid(s_pos)) + mean(-log(1 - sigmoid(s_neg)))``
    over the scores of the two patterns, as binary cross-entropy with logits (stable for any
    score). The means are over this rank's entries (and heads). An empty pattern contributes
    0."""
    dec = decoder if decoder is not None else InnerProductDecoder()
    loss = z.new_zeros((), dtype=torch.float64 if z.dtype == torch.float64 else torch.float32)
    for pattern, target in ((pos, 1.0), (neg, 0.0)):
        s = dec(z, pattern)
        if s.numel():
            loss = loss + Fn.binary_cross_entropy_with_logits(s, torch.full_like(s, target))
    return loss


def negative_pattern(csr: CSR, k: int, generator: Optional[torch.Generator] = None) -> CSR:
    """``k`` uniformly random columns (with replacement, out of ``csr.num_cols``) for every
    non-empty row of ``csr``, as a CSR over the same rows and columns on ``csr``'s device;
    empty rows stay empty. Drawn on the host (``generator``: a CPU generator), once."""
    k = int(k)
    if k < 0:
        raise ValueError(f"negative_pattern: k must be >= 0, got {k}")
    deg = (csr.degree().cpu() > 0).long() * k
    rowptr = torch.zeros(csr.num_rows + 1, dtype=torch.long)
    torch.cumsum(deg, 0, out=rowptr[1:])
    n = int(rowptr[-1])
    col = torch.randint(0, max(csr.num_cols, 1), (n,), generator=generator)
    return CSR(rowptr.to(csr.device), col.to(csr.col.dtype).to(csr.device), csr.num_cols)
