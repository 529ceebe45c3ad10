"""Residual gated graph convolution (Bresson & Laurent, "Residual Gated Graph ConvNets"; PyG's
``ResGatedGraphConv``, the aggregation of GatedGCN) on a vertex-partitioned graph.

``CommAwareResGatedGraphConv`` computes, for every local vertex ``i``::

    out_i = W_skip x_i + bias + sum_j sigmoid(W_key x_i + W_query x_j) * (W_value x_j)

over the in-neighbours ``j``, local and halo; the gate is elementwise, one per channel and
edge. The parameters are named and shaped as PyG's (``lin_key``, ``lin_query``, ``lin_value``
with bias, ``lin_skip`` without, ``bias``), so a PyG ``state_dict`` loads.

MI355X formulation:

* the three projections are ONE GEMM over the concatenated weights, giving ``[k | q | v]``;
  ``k`` and ``[q | v]`` are column views of that result (the kernels take a row stride per
  operand), so nothing is copied;
* the aggregation is ONE gather pass per block of the partition
  (:func:`~dgraph_amd.parallel.dist_graph.dist_gated_aggregate`): each neighbour's ``q`` and
  ``v`` rows are read once, the gate is formed in registers and nothing ``[E, C]`` is written;
  the halo exchange carries the ``[q | v]`` send rows as one message under the interior pass;
* the backward keeps one ``[L, C]`` tensor from the forward pass (``sum_j s (1 - s) v_j``):
  ``dk`` is its elementwise product with the incoming gradient, and ``d[q | v]`` is one gather
  over the transposed pattern per block, the halo block's rows going home as one message.

Out of scope here: ``edge_dim`` (edge features in the gate), gate activations other than the
sigmoid, bf16, and the wiring into the fused executor or ``bench.py``.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..parallel.dist_graph import DistGraph, dist_gated_aggregate


class CommAwareResGatedGraphConv(nn.Module):
    def __init__(self, in_channels: int, out_channels: int, root_weight: bool = True,
                 bias: bool = True, comm=None):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.root_weight = root_weight
        self.comm = comm
        self.lin_key = nn.Linear(in_channels, out_channels)
        self.lin_query = nn.Linear(in_channels, out_channels)
        self.lin_value = nn.Linear(in_channels, out_channels)
        if root_weight:
            self.lin_skip = nn.Linear(in_channels, out_channels, bias=False)
        else:
            self.register_module("lin_skip", None)
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_channels))
        else:
            self.register_parameter("bias", None)

    def reset_parameters(self):
        for m in (self.lin_key, self.lin_query, self.lin_value, self.lin_skip):
            if m is not None:
                m.reset_parameters()
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def forward(self, x: torch.Tensor, graph: DistGraph) -> torch.Tensor:
        C = self.out_channels
        lins = (self.lin_key, self.lin_query, self.lin_value)
        h = F.linear(x, torch.cat([m.weight for m in lins], 0),
                     torch.cat([m.bias for m in lins], 0))  # [k | q | v]
        out = dist_gated_aggregate(h[:, :C], h[:, C:], graph)
        if self.lin_skip is not None:
            out = out + self.lin_skip(x)
        if self.bias is not None:
            out = out + self.bias
        return out
