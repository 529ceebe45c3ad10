"""Principal Neighbourhood Aggregation layer (PyG's ``PNAConv`` without towers, edge
features and the pre-MLP) on a vertex-partitioned graph.

``CommAwarePNAConv`` computes, for every local vertex ``i`` with ``d_i = max(in-degree, 1)``::

    agg_i = [aggr_1(x_j) | ... | aggr_A(x_j)]  over the in-neighbours j     # [A*F]
    out_i = W_root x_i + sum_s scale_s(d_i) * (W_s agg_i) + b

with the aggregators out of ``mean``, ``max``, ``min``, ``std`` and the scalers
``identity = 1``, ``amplification = log(d + 1) / delta``, ``attenuation = delta / log(d + 1)``.
This equals PyG's concatenation of the ``S`` scaled copies of ``agg_i`` followed by one
Linear over ``A*S*F`` inputs (the weights port: ``W_s`` are that Linear's column blocks,
scaler-major).

MI355X formulation:

* all aggregators come from ONE pass over the neighbour rows
  (:func:`~dgraph_amd.parallel.dist_graph.dist_aggregate_multi`: one fused kernel per block
  of the partition, one halo exchange) as the column blocks of one ``[L, A*F]`` buffer;
* the scalers depend on the row alone, so they commute with the linear map: ONE GEMM
  ``agg [W_1 | ... | W_S]`` and a row-scaled sum of its ``S`` column blocks; the
  ``[L, A*S*F]`` tensor is never built;
* ``delta`` defaults to the mean of ``log(d + 1)`` over all vertices of the graph: one
  all-reduce of ``(sum, count)`` over the graph's group at first use, cached on the graph.

Out of scope here: bf16, edge features, towers, the pre-MLP over ``[x_i | x_j]``, and the
wiring into ``GraphSAGE``, the fused executor or ``bench.py``.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as Fn

from ..ops.aggregate import check_aggregators
from ..parallel.dist_graph import DistGraph, dist_aggregate_multi

SCALERS = ("identity", "amplification", "attenuation")


def avg_deg_log(graph: DistGraph) -> float:
    """Mean of ``log(d + 1)``, ``d = max(in-degree, 1)``, over ALL vertices of the
    partitioned graph (collective at first use; cached on ``graph``)."""
    cached = getattr(graph, "_pna_avg_deg_log", None)
    if cached is not None:
        return cached
    import torch.distributed as dist

    d = graph.degree().clamp(min=1).double()
    tot = torch.stack([torch.log(d + 1.0).sum(), torch.tensor(float(d.numel()), dtype=d.dtype,
                                                              device=d.device)])
    # a graph without an exchange plan is whole: its own vertices are all there are
    if graph.a2a is not None and dist.is_initialized() \
            and dist.get_world_size(graph.a2a.group) > 1:
        dist.all_reduce(tot, group=graph.a2a.group)
    graph._pna_avg_deg_log = float(tot[0] / tot[1].clamp(min=1.0))
    return graph._pna_avg_deg_log


class CommAwarePNAConv(nn.Module):
    def __init__(self, in_channels: int, out_channels: int,
                 aggregators=("mean", "max", "min", "std"),
                 scalers=("identity", "amplification", "attenuation"),
                 avg_deg_log: Optional[float] = None, comm=None, bias: bool = True,
                 root_weight: bool = True, eps: float = 1e-5):
        super().__init__()
        self.aggregators = check_aggregators(aggregators)
        self.scalers = (scalers,) if isinstance(scalers, str) else tuple(scalers)
        if not self.scalers or any(s not in SCALERS for s in self.scalers) \
                or len(set(self.scalers)) != len(self.scalers):
            raise ValueError(f"scalers must be distinct names out of {SCALERS}, "
                             f"got {self.scalers!r}")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.avg_deg_log = None if avg_deg_log is None else float(avg_deg_log)
        self.comm = comm
        self.eps = eps
        A, S = len(self.aggregators), len(self.scalers)
        # rows [W_s1 ; W_s2 ; ...]: the S maps [A*F -> out] stacked, so ONE GEMM gives the
        # S column blocks that the scalers weigh
        self.lin = nn.Linear(A * in_channels, S * out_channels, bias=False)
        if root_weight:
            self.lin_root = nn.Linear(in_channels, out_channels, bias=False)
        else:
            self.register_module("lin_root", None)
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        # PyG's one Linear over A*S*F inputs: the same fan-in for every block
        A, S = len(self.aggregators), len(self.scalers)
        bound = 1.0 / math.sqrt(A * S * self.in_channels)
        nn.init.uniform_(self.lin.weight, -bound, bound)
        if self.lin_root is not None:
            self.lin_root.reset_parameters()
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def _scales(self, graph: DistGraph, dtype) -> list:
        """Per-row factor of every scaler (``None`` for identity), cached on the graph."""
        delta = self.avg_deg_log if self.avg_deg_log is not None else \
            avg_deg_log(graph)
        key = ("_pna_scales", delta, dtype)
        cache = graph.__dict__.setdefault("_pna_scale_cache", {})
        if key not in cache:
            logd = torch.log(graph.degree().clamp(min=1).double() + 1.0)
            cache[key] = {"identity": None,
                          "amplification": (logd / delta).to(dtype).unsqueeze(1),
                          "attenuation": (delta / logd).to(dtype).unsqueeze(1)}
        return [cache[key][s] for s in self.scalers]

    def forward(self, x: torch.Tensor, graph: DistGraph) -> torch.Tensor:
        agg = dist_aggregate_multi(x, graph, self.aggregators, self.eps)  # [L, A*F]
        y = Fn.linear(agg, self.lin.weight)                               # [L, S*out]
        C = self.out_channels
        out = self.lin_root(x) if self.lin_root is not None else None
        for k, sc in enumerate(self._scales(graph, y.dtype)):
            yk = y[:, k * C:(k + 1) * C]
            yk = yk if sc is None else yk * sc
            out = yk if out is None else out + yk
        if self.bias is not None:
            out = out + self.bias
        return out
