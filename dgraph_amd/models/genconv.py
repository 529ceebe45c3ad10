"""GENeralized graph convolution with softmax aggregation (DeeperGCN; PyG's ``GENConv`` with
``aggr="softmax"`` and no edge features) on a vertex-partitioned graph.

``CommAwareGENConv`` computes, for every local vertex ``i``::

    msg_j = relu(x_j) + eps                      # per source vertex, eps = 1e-7
    h_i   = sum_j softmax_j(t * msg_j) msg_j + x_i    over the in-neighbours j, per channel
    out_i = MLP(h_i)          # Linear(C, expansion*C) -> LayerNorm -> ReLU -> Linear(., C)

with ``x_j -> lin_src x_j`` and ``x_i -> lin_dst x_i`` when ``in_channels != out_channels``
(as PyG), and the temperature ``t`` a float, or with ``learn_t`` a parameter of shape ``[1]``
(``channelwise_t``: ``[out_channels]``). ``t = 0`` is the mean aggregator, a large ``|t|``
approaches max / min.

MI355X formulation:

* the message depends on the source vertex alone, so it is formed once per vertex (plain
  torch) and the halo exchange carries ``msg``, not ``x``;
* the aggregation is ONE gather pass per block of the partition
  (:func:`~dgraph_amd.parallel.dist_graph.dist_softmax_aggregate`: a running maximum per
  element, nothing written per edge, one halo exchange hidden under the interior pass); the
  backward recomputes every weight from ``(out, lse)`` and gives ``dx`` and ``dt`` from one
  kernel per block;
* ``t`` is a replicated parameter: its gradient is this rank's part and is all-reduced with
  the other weight gradients.

Out of scope here: ``powermean`` and the other GENConv aggregators, edge features, message
norm, bf16, fusing ``relu + eps`` into the gather, and the wiring into ``GraphSAGE``, the
fused executor or ``bench.py``.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..parallel.dist_graph import DistGraph, dist_softmax_aggregate


class CommAwareGENConv(nn.Module):
    def __init__(self, in_channels: int, out_channels: int, t: float = 1.0,
                 learn_t: bool = False, channelwise_t: bool = False, eps: float = 1e-7,
                 expansion: int = 2, norm: bool = True, bias: bool = False, comm=None):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.eps = eps
        self.comm = comm
        self.init_t = float(t)
        if learn_t:
            self.t = nn.Parameter(torch.full((out_channels if channelwise_t else 1,),
                                             self.init_t))
        else:
            self.t = self.init_t
        if in_channels != out_channels:
            self.lin_src = nn.Linear(in_channels, out_channels, bias=bias)
            self.lin_dst = nn.Linear(in_channels, out_channels, bias=bias)
        else:
            self.register_module("lin_src", None)
            self.register_module("lin_dst", None)
        hidden = expansion * out_channels
        layers = [nn.Linear(out_channels, hidden, bias=bias)]
        if norm:
            layers.append(nn.LayerNorm(hidden))
        layers += [nn.ReLU(), nn.Linear(hidden, out_channels, bias=bias)]
        self.mlp = nn.Sequential(*layers)

    def reset_parameters(self):
        for m in self.modules():
            if m is not self and hasattr(m, "reset_parameters"):
                m.reset_parameters()
        if isinstance(self.t, nn.Parameter):
            nn.init.constant_(self.t, self.init_t)

    def forward(self, x: torch.Tensor, graph: DistGraph) -> torch.Tensor:
        xs = x if self.lin_src is None else self.lin_src(x)
        msg = torch.relu(xs) + self.eps
        h = dist_softmax_aggregate(msg, graph, self.t)
        h = h + (x if self.lin_dst is None else self.lin_dst(x))
        return self.mlp(h)
