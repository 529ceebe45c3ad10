"""GENeralized graph convolution with softmax aggregation (DeeperGCN; PyG's ``GENConv`` with
``aggr="softmax"``, with or without edge features) on a vertex-partitioned graph.

``CommAwareGENConv`` computes, for every local vertex ``i``::

    msg_j = relu(x_j) + eps                      # per source vertex, eps = 1e-7
    h_i   = sum_j softmax_j(t * msg_j) msg_j + x_i    over the in-neighbours j, per channel
    out_i = MLP(h_i)          # Linear(C, expansion*C) -> LayerNorm -> ReLU -> Linear(., C)

with ``x_j -> lin_src x_j`` and ``x_i -> lin_dst x_i`` when ``in_channels != out_channels``
(as PyG), and the temperature ``t`` a float, or with ``learn_t`` a parameter of shape ``[1]``
(``channelwise_t``: ``[out_channels]``). ``t = 0`` is the mean aggregator, a large ``|t|``
approaches max / min.

With ``edge_dim`` the message depends on the edge, as PyG's ``GENConv(edge_dim=)``::

    msg_ij = relu(x_j + e_ij) + eps              # per edge i <- j

with ``e_ij -> lin_edge e_ij`` when ``edge_dim != out_channels``. ``forward`` then takes
``edge_attr``, the pair ``(interior block, halo block)`` of ``[nnz_block, edge_dim]`` rows in
the slot order of ``graph.interior`` / ``graph.halo`` (per-slot rows of the unsplit pattern are
cut into the pair by :meth:`~dgraph_amd.ops.csr.CSR.split_edge_values`).

MI355X formulation:

* the message depends on the source vertex alone, so it is formed once per vertex (plain
  torch) and the halo exchange carries ``msg``, not ``x``;
* the aggregation is ONE gather pass per block of the partition
  (:func:`~dgraph_amd.parallel.dist_graph.dist_softmax_aggregate`: a running maximum per
  element, nothing written per edge, one halo exchange hidden under the interior pass); the
  backward recomputes every weight from ``(out, lse)`` and gives ``dx`` and ``dt`` from one
  kernel per block;
* with ``edge_dim`` the message cannot be formed per vertex: the exchange carries
  ``lin_src x`` and ``x_j + e_ij``, ``relu`` and ``+ eps`` run per slot inside the gather
  (:func:`~dgraph_amd.parallel.dist_graph.dist_softmax_aggregate_edge`), so nothing ``[E,
  C]`` is written forward beyond the projected edge rows; the backward writes the edge
  gradient once (``lin_edge``'s weight gradient reads it) and sums it once for ``dx``;
* ``t`` is a replicated parameter: its gradient is this rank's part and is all-reduced with
  the other weight gradients.

Out of scope here: ``powermean`` and the other GENConv aggregators, message norm, bf16 (edge
rows included), fusing ``relu + eps`` into the gather of the layer WITHOUT edge features, and
the wiring into ``GraphSAGE``, the fused executor or ``bench.py``.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..parallel.dist_graph import (DistGraph, dist_softmax_aggregate,
                                   dist_softmax_aggregate_edge)


class CommAwareGENConv(nn.Module):
    def __init__(self, in_channels: int, out_channels: int, t: float = 1.0,
                 learn_t: bool = False, channelwise_t: bool = False, eps: float = 1e-7,
                 expansion: int = 2, norm: bool = True, bias: bool = False, comm=None,
                 edge_dim=None):
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
        self.edge_dim = edge_dim
        if edge_dim is not None and edge_dim != out_channels:
            self.lin_edge = nn.Linear(edge_dim, out_channels, bias=bias)
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

    def _edge_rows(self, edge_attr):
        """The ``(interior, halo)`` edge blocks at ``out_channels`` width."""
        if not isinstance(edge_attr, (tuple, list)) or len(edge_attr) != 2:
            raise ValueError("edge_attr must be the pair (interior block, halo block)")
        rows = []
        for e in edge_attr:
            if e is not None:
                if e.dim() != 2 or e.shape[1] != self.edge_dim:
                    raise ValueError(f"edge_attr blocks must be [nnz_block, {self.edge_dim}], "
                                     f"got {tuple(e.shape)}")
                if self.edge_dim != self.out_channels:
                    e = self.lin_edge(e)
            rows.append(e)
        return rows

    def forward(self, x: torch.Tensor, graph: DistGraph, edge_attr=None) -> torch.Tensor:
        if (edge_attr is None) != (self.edge_dim is None):
            raise ValueError("edge_attr must be given exactly when edge_dim is set "
                             f"(edge_dim={self.edge_dim})")
        xs = x if self.lin_src is None else self.lin_src(x)
        if edge_attr is None:
            msg = torch.relu(xs) + self.eps
            h = dist_softmax_aggregate(msg, graph, self.t)
        else:
            h = dist_softmax_aggregate_edge(xs, *self._edge_rows(edge_attr), graph, self.t,
                                            relu=True, eps=self.eps)
        h = h + (x if self.lin_dst is None else self.lin_dst(x))
        return self.mlp(h)
