"""GATv2 graph attention layer (Brody et al., "How attentive are graph attention networks?";
PyG's ``GATv2Conv``) on a distributed relation.

``CommAwareGATv2Conv`` computes, for every destination vertex ``i`` of one relation and per
head ``h`` (``out_channels = heads * D``, heads concatenated as in ``CommAwareGAT``)::

    l_i = W_dst x_i + b_dst        r_j = W_src x_j + b_src
    e_ij[h] = att[h] . LeakyReLU(l_i[h] + r_j[h])
    out_i[h] = sum_j softmax_j(e_ij[h]) r_j[h]   (+ W_res x_i) (+ bias)

The nonlinearity sits between the projection and the attention vector, so the ranking of the
neighbours depends on the destination ("dynamic" attention), which the additive score of
``CommAwareGAT`` (``LeakyReLU(s_i + s_j)`` of two scalars) cannot express.

MI355X formulation (with a :class:`~dgraph_amd.data.hetero.RelationGraph`):

* with one input (``x_j`` absent) and unshared weights, the two projections are ONE GEMM into
  one ``[N, 2C]`` buffer ``[l | r]``; the attention kernels read its column halves in place
  (row stride ``2C``);
* with more than one rank, ONE halo exchange moves the ``r`` rows of remote sources, C columns
  wide (:class:`~dgraph_amd.parallel.halo.HaloExchange`; its adjoint returns their gradient
  in backward), issued on every rank whether or not it receives rows; the received rows are
  read as a second source, never concatenated with the local ones;
* the attention itself is :func:`~dgraph_amd.ops.gatv2.gatv2_attention`: three fused kernels,
  no per-edge tensor (GPU fp32), or its fp64 plain-PyTorch evaluation (CPU).

Out of scope here: wiring the layer into ``CommAwareRGAT``, the lean ``HeteroGraph`` path or
the OGB-LSC trainer; bf16; edge features; attention dropout; averaging the heads instead of
concatenating them; adding self loops (the caller's graph decides).
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops.gat import GatPattern
from ..ops.gatv2 import gatv2_attention
from .rgat import _world


class CommAwareGATv2Conv(nn.Module):
    def __init__(self, in_channels: int, out_channels: int, comm=None, heads: int = 1,
                 negative_slope: float = 0.2, bias: bool = True, residual: bool = False,
                 share_weights: bool = False, hetero: bool = False):
        super().__init__()
        if out_channels % heads:
            raise ValueError("out_channels must be divisible by heads")
        self.comm = comm
        self.heads = heads
        self.negative_slope = negative_slope
        self.residual = residual
        self.share_weights = share_weights
        self.hetero = hetero
        self.out_channels = out_channels
        self.lin_src = nn.Linear(in_channels, out_channels)
        self.lin_dst = self.lin_src if share_weights else nn.Linear(in_channels, out_channels)
        self.att = nn.Parameter(torch.empty(heads, out_channels // heads))
        nn.init.xavier_uniform_(self.att)  # glorot
        if residual:
            self.res_net = nn.Linear(in_channels, out_channels, bias=False)
        else:
            self.register_module("res_net", None)
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_channels))
        else:
            self.register_parameter("bias", None)
        self._halo = None

    @staticmethod
    def _pattern(graph) -> GatPattern:
        """The relation's attention pattern and its transpose, built once per graph."""
        pat = graph._cache.get("gatv2_pattern")
        if pat is None:
            pat = GatPattern(graph.csr.rowptr, graph.csr.col, graph.num_local_src,
                             graph.num_halo)
            graph._cache["gatv2_pattern"] = pat
        return pat

    def forward(self, x, graph, x_j=None):
        C = self.out_channels
        xj = x_j if (self.hetero and x_j is not None) else x
        if xj is x and not self.share_weights:
            # one GEMM for both projections: [l | r] = x [W_dst ; W_src]^T + [b_dst | b_src]
            lr = F.linear(x, torch.cat([self.lin_dst.weight, self.lin_src.weight], 0),
                          torch.cat([self.lin_dst.bias, self.lin_src.bias], 0))
            xd, xs = lr[:, :C], lr[:, C:]
        else:
            xs = self.lin_src(xj)
            xd = xs if xj is x else self.lin_dst(x)
        xsh = None
        if _world(self.comm) > 1:  # collective on every rank of the relation's group
            from ..parallel.halo import HaloExchange

            if self._halo is None:
                self._halo = HaloExchange(self.comm)
            xsh = self._halo(xs, graph.pattern)
        out = gatv2_attention(xd, xs, self.att, self._pattern(graph), xsh, heads=self.heads,
                              negative_slope=self.negative_slope)
        if self.res_net is not None:
            out = out + self.res_net(x)
        if self.bias is not None:
            out = out + self.bias
        return out
