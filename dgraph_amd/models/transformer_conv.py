"""Scaled dot-product graph attention layer (PyG's ``TransformerConv``, the UniMP layer) on
a distributed relation.

``CommAwareTransformerConv`` computes, for every destination vertex ``i`` of one relation and
per head ``h`` (``out_channels = heads * D``, heads concatenated as in ``CommAwareGAT``)::

    q_i = W_q x_i + b_q        [k_j | v_j] = W_kv x_j + b_kv
    out_i[h] = sum_j softmax_j(<q_i[h], k_j[h]> / sqrt(D)) v_j[h]  (+ W_skip x_i) (+ bias)

MI355X formulation (with a :class:`~dgraph_amd.data.hetero.RelationGraph`):

* keys and values come from ONE GEMM into one ``[N, 2C]`` buffer; the attention kernels read
  its two column halves in place (row stride ``2C``);
* with more than one rank, ONE halo exchange moves the ``[k | v]`` rows of remote sources
  (:class:`~dgraph_amd.parallel.halo.HaloExchange`; its adjoint returns their gradient in
  backward), issued on every rank whether or not it receives rows; the received rows are
  read as a second source, never concatenated with the local ones;
* the attention itself is :func:`~dgraph_amd.ops.dot_attn.dot_attention`: three fused
  kernels, no per-edge tensor (GPU fp32), or its fp64 plain-PyTorch evaluation (CPU);
* ``overlap=True`` (more than one rank) moves the exchange inside the attention op
  (:func:`~dgraph_amd.ops.dot_attn.dot_attention_halo`): the interior edges are attended
  over while the ``[k | v]`` rows are on the links and the halo edges are folded into the
  same softmax when they land (the kernel's carry-in forward); in backward the halo rows'
  gradient is computed first and returns to its owners under ``dq`` and the local ``dk`` /
  ``dv``. Still one exchange forward and one backward on every rank. The default is the
  synchronous exchange: the overlapped path has only been timed against a link model on
  one GPU (PERFORMANCE.md), not on a multi-GPU node;
* ``edge_dim=`` (PyG's ``edge_dim``, the UniMP edge term): ``edge_attr [E_local, edge_dim]``
  in the relation's CSR slot order (:func:`~dgraph_amd.data.hetero.relation_edge_order`
  gives that order for a global edge list) is projected by ``lin_edge`` (no bias) to
  ``[E_local, C]`` and added to the edge's key and to its value inside the attention kernels
  (``dot_attention(..., edge=)``, csrc/kernels/dot_attn_edge_f32.hip). Edge features live
  with the destination's rank and never travel: still one exchange forward and one backward;
* ``dropout=`` (PyG's ``dropout``, as UniMP trains): in training the attention coefficients are
  dropped after the softmax inside the kernels (``dot_attention(..., dropout_p=)``,
  csrc/kernels/dot_attn_drop_f32.hip). No mask is stored: the keep decision of an edge is a
  stateless function of a per-call seed, the edge's CSR slot and the head. The layer draws
  the seed from the device's torch generator (no host sync) and, with more than one rank,
  offsets it per rank, so equal torch seeds on all ranks do not give edges with equal local
  slot numbers the same bits. ``forward(..., dropout_seed=)`` fixes the seed (tests, captured
  steps). Evaluation mode and ``dropout=0`` are exactly the layer without it.

Out of scope here: the same overlap for the GAT and GATv2 layers (their kernels have no carry-in
forward yet); edge features together with ``overlap=True`` (the carry-in forward and the
parts / halo ops take none), in the GAT / GATv2 layers, or projected from ``edge_dim``
columns inside the kernel (which would avoid the ``[E, C]`` tensor); wiring the layer into
``CommAwareRGAT``, the lean ``HeteroGraph`` path, GraphCast or the OGB-LSC trainer; bf16;
PyG's ``beta`` gate between the skip and the attention output; attention dropout together
with ``overlap=True`` or ``edge_dim`` (the carry-in forward, the parts / halo ops and the
edge-feature kernels take none) or in the GAT / GATv2 layers; a fused feature-dropout epilogue.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from ..ops.dot_attn import HaloPlan, dot_attention, dot_attention_halo
from ..ops.gat import GatPattern
from .rgat import _world


class CommAwareTransformerConv(nn.Module):
    def __init__(self, in_channels: int, out_channels: int, comm=None, heads: int = 1,
                 bias: bool = True, root_weight: bool = True, hetero: bool = False,
                 overlap: bool = False, edge_dim: Optional[int] = None, dropout: float = 0.0):
        super().__init__()
        if out_channels % heads:
            raise ValueError("out_channels must be divisible by heads")
        dropout = float(dropout)
        if not 0.0 <= dropout < 1.0:
            raise ValueError(f"dropout must lie in [0, 1), got {dropout}")
        if dropout > 0.0 and (overlap or edge_dim is not None):
            raise ValueError("dropout with overlap=True or edge_dim is not supported: the "
                             "overlapped attention op and the edge-feature kernels take no "
                             "attention dropout")
        self.dropout = dropout
        if edge_dim is not None and overlap:
            raise ValueError("edge_dim with overlap=True is not supported: the overlapped "
                             "attention op takes no edge features")
        self.comm = comm
        self.heads = heads
        self.hetero = hetero
        self.overlap = overlap
        self.out_channels = out_channels
        self.lin_query = nn.Linear(in_channels, out_channels)
        self.lin_kv = nn.Linear(in_channels, 2 * out_channels)  # rows [W_k ; W_v]
        self.edge_dim = edge_dim
        if edge_dim is not None:  # (no attribute at all otherwise: state_dict keys as before)
            self.lin_edge = nn.Linear(edge_dim, out_channels, bias=False)
        if root_weight:
            self.lin_skip = nn.Linear(in_channels, out_channels, bias=False)
        else:
            self.register_module("lin_skip", None)
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_channels))
        else:
            self.register_parameter("bias", None)
        self._halo = None

    @staticmethod
    def _pattern(graph) -> GatPattern:
        """The relation's attention pattern and its transpose, built once per graph."""
        pat = graph._cache.get("dot_attn_pattern")
        if pat is None:
            pat = GatPattern(graph.csr.rowptr, graph.csr.col, graph.num_local_src,
                             graph.num_halo)
            graph._cache["dot_attn_pattern"] = pat
        return pat

    _RANK_MIX = 0x9E3779B97F4A7C15  # per-rank seed offset (mod 2^62): the 64-bit golden ratio

    def _dropout_seed(self, device, dropout_seed=None) -> torch.Tensor:
        """This call's seed tensor: the given one, or one drawn from ``device``'s torch
        generator, plus the rank's offset (a tensor add, no sync)."""
        if dropout_seed is None:
            dropout_seed = torch.randint(0, 2 ** 62, (1,), device=device)
        if _world(self.comm) > 1:
            dropout_seed = dropout_seed + (self.comm.get_rank() * self._RANK_MIX) % 2 ** 62
        return dropout_seed

    def forward(self, x, graph, x_j=None, edge_attr=None, dropout_seed=None):
        C = self.out_channels
        if (edge_attr is None) != (self.edge_dim is None):
            raise ValueError("edge_attr is given exactly when the layer has edge_dim")
        edge = None if edge_attr is None else self.lin_edge(edge_attr)
        q = self.lin_query(x)
        kv = self.lin_kv(x_j if (self.hetero and x_j is not None) else x)
        pat = self._pattern(graph)
        if _world(self.comm) > 1 and self.overlap:  # the exchange runs inside the op
            plan = graph._cache.get("dot_attn_halo_plan")
            if plan is None or plan.send_map.num_src != kv.shape[0]:
                plan = HaloPlan.from_pattern(self.comm, graph.pattern, kv.shape[0])
                graph._cache["dot_attn_halo_plan"] = plan
            out = dot_attention_halo(q, kv, pat, plan, heads=self.heads)
        else:
            kh = vh = None
            if _world(self.comm) > 1:  # collective on every rank of the relation's group
                from ..parallel.halo import HaloExchange

                if self._halo is None:
                    self._halo = HaloExchange(self.comm)
                halo = self._halo(kv, graph.pattern)
                kh, vh = halo[:, :C], halo[:, C:]
            if self.training and self.dropout > 0.0:
                out = dot_attention(q, kv[:, :C], kv[:, C:], pat, kh, vh, heads=self.heads,
                                    dropout_p=self.dropout,
                                    dropout_seed=self._dropout_seed(q.device, dropout_seed))
            elif edge is None:
                out = dot_attention(q, kv[:, :C], kv[:, C:], pat, kh, vh, heads=self.heads)
            else:
                out = dot_attention(q, kv[:, :C], kv[:, C:], pat, kh, vh, heads=self.heads,
                                    edge=edge)
        if self.lin_skip is not None:
            out = out + self.lin_skip(x)
        if self.bias is not None:
            out = out + self.bias
        return out
