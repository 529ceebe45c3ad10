"""Per-rank partitioned graph with halo-overlapped aggregation.

This is the hot path of vertex-partitioned full-graph training (P1-P3, §5.7 design 1).
The local CSR (rows = owned vertices, columns = owned vertices ++ halo rows) is split
once into an *interior* part (columns < L) and a *halo* part (columns >= L). Then

    aggregate(x):   pack send rows (native gather) -> RCCL all-to-all-v on the comm stream
                    || interior SpMM on the compute stream -> wait -> halo SpMM (beta=1)
    aggregate_T(g): halo^T SpMM -> reverse all-to-all-v || interior^T SpMM -> wait ->
                    segment-sum of the received rows into their owners (beta=1)

so the interior aggregation hides the exchange, and there is no host sync and no float
atomic anywhere. ``aggregate_T`` is the exact adjoint of ``aggregate``. The reference
serialised every exchange with compute and synced the host per exchange (§3.2 notes).
"""
from __future__ import annotations

import os
import weakref
from dataclasses import dataclass
from typing import List, Optional

import torch
from torch.autograd import Function

from ..comm.alltoallv import AllToAllV
from ..ops import kernels as K
from ..ops.aggregate import (EdgeDrop, as_temperature, check_aggregators, inv_kept,
                             multi_blocks, vec_rows)
from ..ops.csr import CSR, IndexMap


# Hub-row split threshold for the SpMM (ops.csr.CSR.hub_split): rows with more entries
# run their tails as separate segment waves. 0 disables.
SPMM_HUB_CAP = int(os.environ.get("DGRAPH_SPMM_HUB_CAP", "2048"))


def _hs(csr: CSR):
    return csr.hub_split(SPMM_HUB_CAP) if SPMM_HUB_CAP > 0 else None


def _select_columns(csr: CSR, cols: torch.Tensor, ncols: int) -> CSR:
    """``csr`` restricted to the entries whose column is in ``cols`` (row order and the
    order within a row kept). Two passes over row chunks of ~2^26 entries: count, then
    copy into the exact-size column array (bounded temporaries at 10^9+ entries, no
    concatenation copy)."""
    dev = csr.device
    keep = torch.zeros(ncols, dtype=torch.bool, device=dev)
    keep[cols] = True
    R = csr.num_rows
    nnz = max(csr.col.numel(), 1)
    step = max(1, int(R * (1 << 26) // nnz))
    chunks = [(r0, min(R, r0 + step)) for r0 in range(0, R, step)]
    deg = torch.zeros(R, dtype=torch.long, device=dev)
    for r0, r1 in chunks:
        a, b = int(csr.rowptr[r0]), int(csr.rowptr[r1])
        if b == a:
            continue
        m = keep[csr.col[a:b].long()]
        rows = torch.repeat_interleave(torch.arange(r0, r1, device=dev),
                                       csr.rowptr[r0 + 1:r1 + 1] - csr.rowptr[r0:r1],
                                       output_size=b - a)
        deg[r0:r1] = torch.bincount(rows[m] - r0, minlength=r1 - r0)
        del m, rows
    rowptr = torch.zeros(R + 1, dtype=torch.long, device=dev)
    torch.cumsum(deg, 0, out=rowptr[1:])
    del deg
    col = torch.empty(int(rowptr[-1]), dtype=csr.col.dtype, device=dev)
    for r0, r1 in chunks:
        a, b = int(csr.rowptr[r0]), int(csr.rowptr[r1])
        if b == a:
            continue
        c = csr.col[a:b]
        col[int(rowptr[r0]):int(rowptr[r1])] = c[keep[c.long()]]
        del c
    return CSR(rowptr, col, csr.num_cols, None, symmetric=False)


def _cache_lookup(cache: dict, rows: torch.Tensor):
    """Plan-cache hit for the row-index tensor ``rows``: the SAME live tensor object (a
    weak reference, never the address, which a freed tensor's successor can reuse) at the
    same version counter (an in-place edit of ``rows`` misses). Building a sub-plan on a
    miss is collective, so the key must not depend on allocator state that can differ
    between ranks."""
    ref = cache.get("ref")
    if ref is not None and ref() is rows and cache.get("version") == rows._version:
        return cache["plan"]
    return None


def _cache_store(cache: dict, rows: torch.Tensor, plan) -> None:
    cache.clear()
    cache.update(ref=weakref.ref(rows), version=rows._version, plan=plan)


class DistGraph:
    def __init__(
        self,
        csr: CSR,
        num_local: int,
        num_halo: int,
        send_local_idx: Optional[torch.Tensor] = None,
        send_splits: Optional[List[int]] = None,
        recv_splits: Optional[List[int]] = None,
        group=None,
        symmetric: bool = False,
        overlap: bool = True,
        chunk_bytes: Optional[int] = None,
    ):
        assert csr.num_rows == num_local, "CSR rows must be the local vertices"
        assert csr.num_cols == num_local + num_halo
        self.L, self.H = int(num_local), int(num_halo)
        self.csr = csr
        self.inv_deg = csr.inv_degree()
        self.symmetric = symmetric
        self.overlap = overlap
        # per-peer message size above which an exchange is cut into column chunks
        self.chunk_bytes = int(os.environ.get("DGRAPH_HALO_CHUNK_BYTES", str(32 << 20))) \
            if chunk_bytes is None else int(chunk_bytes)
        self._restrict_cache = {}
        self._restrict_fwd_cache = {}
        self._static_cache = {}
        self._support_cache = {}
        # edges (nonzeros) aggregated by every call so far, forward and transposed:
        # bench.py reports the per-step delta as ``edges_aggregated_per_step``
        self.edges_aggregated = 0
        # optional int64 [L + H]: the global ids of the local rows, then of the halo rows
        # (build_partition returns ``offsets`` and ``halo_gids``), which the DropEdge
        # decision of aggregate_drop is keyed by; W = 1, 2, 3 then drop exactly the same
        # edges. None: the local numbering 0 .. L + H, which is still consistent between the
        # forward and the backward of a rank, but not across partitions.
        self.vertex_ids: Optional[torch.Tensor] = None
        if self.H > 0 or (send_local_idx is not None and send_local_idx.numel() > 0):
            self.interior, self.halo = csr.split_columns(self.L)
            self.interior.symmetric = symmetric
            self.send_map = IndexMap(send_local_idx.to(csr.device), self.L)
            self.a2a = AllToAllV(send_splits, recv_splits, group)
            self.a2a_rev = self.a2a.reversed()
            if self.a2a.total_recv != self.H:
                raise ValueError(f"recv splits sum {self.a2a.total_recv} != halo {self.H}")
        else:
            self.interior, self.halo = csr, None
            self.interior.symmetric = symmetric
            self.send_map = None
            self.a2a = self.a2a_rev = None
        # drop the un-split copy's column array when split (memory: 288 GB budget)
        if self.halo is not None:
            self.csr = None
        from ..utils.diagnostics import maybe_validate

        maybe_validate(self)  # DGRAPH_CHECK_PLANS=1: once per plan, not per call

    @property
    def device(self):
        return self.interior.device if self.interior is not None else self._device

    @property
    def nnz(self) -> int:
        """Message edges aggregated at this rank's vertices (interior + halo)."""
        if self.interior is None:
            return self._nnz
        return self.interior.nnz + (self.halo.nnz if self.halo is not None else 0)

    def release_csr(self) -> None:
        """Drop the interior / halo CSRs (and everything cached from them). For an executor
        that built its own adjacency from them (models/sage_fused.py keeps a rank's interior
        and halo entries in ONE array) and needs only the exchange plans from here on: at
        the papers100M shape the split copy is 6.5 GB per rank at W = 2. The aggregation
        methods of this object cannot be used afterwards."""
        if self.interior is None:
            return
        self._device = self.interior.device
        self._nnz = self.nnz
        self._had_halo = self.halo is not None
        self.interior = None
        self.halo = None
        self._restrict_cache.clear()
        self._restrict_fwd_cache.clear()
        self._support_cache.clear()

    @staticmethod
    def from_pattern(cp, num_nbr_rows: Optional[int] = None, group=None,
                     symmetric: bool = False) -> "DistGraph":
        """From a :class:`CommunicationPattern` (its local_edge_list = (central, nbr))."""
        le = cp.local_edge_list
        L_n = cp.num_local_neighbor_vertices or cp.num_local_vertices
        if L_n != cp.num_local_vertices:
            raise ValueError("DistGraph needs a homogeneous pattern (use plan ops for bipartite)")
        csr = CSR.from_coo(le[:, 0], le[:, 1], cp.num_local_vertices,
                           cp.num_local_vertices + cp.num_halo_vertices)
        return DistGraph(csr, cp.num_local_vertices, cp.num_halo_vertices, cp.send_local_idx,
                         cp.send_splits(), cp.recv_splits(), group, symmetric)

    # ------------------------------------------------------------------ non-autograd
    def _static_halo(self, x: torch.Tensor) -> Optional[torch.Tensor]:
        """Halo rows of a read-only input (the vertex features), replicated once and kept:
        partition-time halo replication of inputs, as DistDGL-style partitions store them.
        Keyed by storage, shape and the tensor's version counter, so an in-place update of
        ``x`` re-exchanges."""
        c = self._static_cache
        if c.get("ref") is not None and c["ref"]() is x and c["version"] == x._version:
            return c["recv"]
        # a weak reference, not the address: a freed tensor's storage can be reused
        c.clear()
        cb = self.static_halo_block(x.shape[1], x.element_size())
        if cb >= x.shape[1]:
            recv = self.a2a(K.gather_rows(x, self.send_map.idx))
        else:
            # a large halo (structureless graph): packed and exchanged in column blocks, so
            # the transient send/receive buffers stay small next to the kept halo rows
            recv = torch.empty(self.a2a.total_recv, x.shape[1], dtype=x.dtype, device=x.device)
            for c0 in range(0, x.shape[1], cb):
                c1 = min(c0 + cb, x.shape[1])
                recv[:, c0:c1] = self.a2a(K.gather_rows(x[:, c0:c1], self.send_map.idx))
        c.update(ref=weakref.ref(x), version=x._version, recv=recv)
        return c["recv"]

    STATIC_BLOCK_BYTES = 4 << 30

    def static_halo_block(self, F: int, elem: int = 4) -> int:
        """Column-block width of the static halo exchange: whole rows unless the packed send
        rows exceed ``STATIC_BLOCK_BYTES``. Its transient (send + receive blocks) is
        ``(n_send + H) * block * elem`` bytes on top of the kept ``H * F`` halo rows."""
        n_send = self.send_map.idx.numel() if self.send_map is not None else 0
        if n_send * F * elem <= self.STATIC_BLOCK_BYTES:
            return F
        cb = max(16, (self.STATIC_BLOCK_BYTES // max(n_send * elem, 1)) // 16 * 16)
        return min(cb, F)

    def aggregate(self, x: torch.Tensor, mean: bool = True,
                  out: Optional[torch.Tensor] = None, static: bool = False,
                  halo_rows: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Mean (or sum) over in-neighbours, local and halo. ``static=True`` marks ``x``
        as a read-only input whose halo rows may be exchanged once and reused.
        ``halo_rows``: the halo rows' values ``[H, F]`` computed on this rank (halo
        recomputation, :mod:`~dgraph_amd.parallel.halo_recompute`): no exchange."""
        rs = self.inv_deg if mean else None
        self.edges_aggregated += self.nnz
        if self.halo is None:
            return K.spmm(self.interior.rowptr, self.interior.col, x, out, row_scale=rs,
                          split=_hs(self.interior))
        if static or halo_rows is not None:
            recv = self._static_halo(x) if halo_rows is None else halo_rows
            out = K.spmm(self.interior.rowptr, self.interior.col, x, out, row_scale=rs,
                         split=_hs(self.interior))
            hc = self.halo.compact_rows()
            K.spmm(hc.rowptr, hc.col, recv, out, row_scale=rs, beta=1.0, split=_hs(hc),
                   row_map=hc.row_map)
            return out
        if out is None:
            out = torch.empty(self.L, x.shape[1], dtype=x.dtype, device=x.device)
        # column chunks: chunk k's halo SpMM runs while chunk k+1 is on the links
        pend = []
        for c0, c1 in self._col_chunks(self.a2a, x.shape[1], x.element_size()):
            xc = x if (c0, c1) == (0, x.shape[1]) else x[:, c0:c1]
            recv, work = self.a2a(K.gather_rows(xc, self.send_map.idx), async_op=True)
            if not self.overlap:
                work.wait()
            pend.append((c0, c1, recv, work))
        K.spmm(self.interior.rowptr, self.interior.col, x, out, row_scale=rs,
               split=_hs(self.interior))
        hc = self.halo.compact_rows()
        for c0, c1, recv, work in pend:
            work.wait()
            oc = out if (c0, c1) == (0, x.shape[1]) else out[:, c0:c1]
            K.spmm(hc.rowptr, hc.col, recv, oc, row_scale=rs, beta=1.0, split=_hs(hc),
                   row_map=hc.row_map)
        return out

    def _col_chunks(self, a2a, F: int, esize: int):
        """Column ranges of one exchange: a single range unless the largest per-peer
        message exceeds 2 x ``chunk_bytes``; then chunks of whole 64-column blocks, each
        per-peer message of a chunk >= ``chunk_bytes`` / 2 (RCCL's per-call cost stays
        negligible; xGMI is point-to-point, so a peer message is one link's load)."""
        cb = self.chunk_bytes
        peer = max(max(a2a.send_splits, default=0), max(a2a.recv_splits, default=0))
        per_peer = peer * F * esize
        if cb <= 0 or per_peer <= 2 * cb or F < 128:
            return [(0, F)]
        n = min(-(-per_peer // cb), F // 64)
        w = -(-F // n)
        w = -(-w // 64) * 64
        return [(c, min(c + w, F)) for c in range(0, F, w)]

    # row blocks of the fused pre-scale + bias-gradient column sums (row_scale_colsum)
    COLSUM_BLOCKS = 1024

    @staticmethod
    def _spmm_col_scaled(csr: CSR, g: torch.Tensor, cs: torch.Tensor, out, scratch,
                         colsum: Optional[list] = None):
        """``A g`` with a column scale. With a ``scratch`` buffer (a free workspace slot)
        the scale is applied to column slices of ``g`` first (one streaming pass) and the
        SpMM runs unweighted: a per-edge scale gather costs the gather-bound kernel a
        second scattered load per neighbour (+25-55 % per pass, benchmarks/bench_spmm.py
        --mean col)."""
        rows, F = g.shape
        S = 0 if scratch is None else min(F, (scratch.numel() // max(rows, 1)) // 64 * 64)
        if S < 64 or g.dtype != torch.bfloat16 or not g.is_cuda:
            out = K.spmm(csr.rowptr, csr.col, g, out, col_scale=cs, split=_hs(csr))
            if colsum is not None:
                colsum.append(K.col_sum(g))
            return out
        if out is None:
            out = torch.empty(csr.num_rows, F, dtype=g.dtype, device=g.device)
        aligned = g.data_ptr() % 16 == 0 and scratch.data_ptr() % 16 == 0 and F % 8 == 0
        # ``colsum`` (a list): append the fp32 column sums of g, formed by the scale pass
        partial = None
        if colsum is not None and aligned and F <= 2048:
            partial = torch.empty(min(DistGraph.COLSUM_BLOCKS, max(rows, 1)), F,
                                  dtype=torch.float32, device=g.device)
        for c0 in range(0, F, S):
            w = min(S, F - c0)
            buf = scratch[: rows * w].view(rows, w)
            if partial is not None and w % 8 == 0 and w <= 256:
                K.row_scale_colsum(g[:, c0:c0 + w], cs, buf, partial[:, c0:c0 + w])
            elif aligned and w % 8 == 0:
                if partial is not None:
                    partial[:, c0:c0 + w].zero_()
                    partial[0, c0:c0 + w] = K.col_sum(g[:, c0:c0 + w])
                K.row_scale_cols(g[:, c0:c0 + w], cs, buf)
            else:
                torch.mul(g[:, c0:c0 + w], cs.unsqueeze(1), out=buf)
            K.spmm(csr.rowptr, csr.col, buf, out[:, c0:c0 + w], split=_hs(csr))
        if colsum is not None:
            colsum.append(partial.sum(0) if partial is not None else K.col_sum(g))
        return out

    def _interior_T(self, it: CSR, g, cs, out, scratch, colsum):
        if cs is not None and scratch is not None:
            return self._spmm_col_scaled(it, g, cs, out, scratch.reshape(-1), colsum)
        out = K.spmm(it.rowptr, it.col, g, out, col_scale=cs, split=_hs(it))
        if colsum is not None:
            colsum.append(K.col_sum(g))
        return out

    def aggregate_T(self, g: torch.Tensor, mean: bool = True,
                    out: Optional[torch.Tensor] = None,
                    scratch: Optional[torch.Tensor] = None, overlap=None,
                    halo_out: Optional[torch.Tensor] = None,
                    colsum: Optional[list] = None, support=None) -> torch.Tensor:
        """Transposed aggregation (the backward of :meth:`aggregate`). ``scratch``: an
        optional free buffer (any shape, same dtype as ``g``) for the pre-scaled path.
        ``overlap``: a callable of independent work, run after the reverse exchange and
        the interior SpMM are issued and before the exchange is waited for.
        ``halo_out``: ``[H, F]`` buffer that receives the halo rows' gradient, which then
        stays on this rank (halo recomputation: the rows were computed here) — no
        exchange, no owner-side segment sum. ``colsum``: a list that receives the fp32
        column sums of ``g`` (a bias gradient) before ``overlap`` runs — formed by the
        pre-scale pass when there is one, else by a column-sum pass."""
        cs = self.inv_deg if mean else None
        g = g.contiguous()
        it = self.interior if self.interior.symmetric else self.interior.transpose()
        if support is not None:
            # ``support`` = grad_support(rows): g is zero outside S, so only the interior
            # entries with a source in S contribute
            it = support[1]
        self.edges_aggregated += it.nnz + (self.halo.nnz if self.halo is not None else 0)
        if halo_out is not None and self.halo is not None:
            K.spmm(self.halo.transpose().rowptr, self.halo.transpose().col, g, halo_out,
                   col_scale=cs, split=_hs(self.halo.transpose()))
            out = self._interior_T(it, g, cs, out, scratch, colsum)
            if overlap is not None:
                overlap()
            return out
        if self.halo is None:
            out = self._interior_T(it, g, cs, out, scratch, colsum)
            if overlap is not None:
                overlap()
            return out
        ht = self.halo.transpose()
        F = g.shape[1]
        pend = []
        for c0, c1 in self._col_chunks(self.a2a_rev, F, g.element_size()):
            gc = g if (c0, c1) == (0, F) else g[:, c0:c1]
            hg = K.spmm(ht.rowptr, ht.col, gc, col_scale=cs, split=_hs(ht))
            sg, work = self.a2a_rev(hg, async_op=True)
            if not self.overlap:
                work.wait()
            pend.append((c0, c1, sg, work))
        out = self._interior_T(it, g, cs, out, scratch, colsum)
        if overlap is not None:
            overlap()  # independent work queued behind the exchange (e.g. a weight grad)
        st = self.send_map.transpose_csr().compact_rows()
        for c0, c1, sg, work in pend:
            work.wait()
            oc = out if (c0, c1) == (0, F) else out[:, c0:c1]
            K.spmm(st.rowptr, st.col, sg, oc, beta=1.0, split=_hs(st), row_map=st.row_map)
        return out

    def aggregate_extreme(self, x: torch.Tensor, minimum: bool = False,
                          out: Optional[torch.Tensor] = None,
                          halo_rows: Optional[torch.Tensor] = None):
        """Elementwise max (``minimum``: min) over in-neighbours, local and halo, on the
        schedule of :meth:`aggregate`: the interior pass runs while the halo rows are on the
        links, then the halo block is applied as a second source. Returns ``(out, arg)``;
        ``arg[r, f]`` (int32) names the winning entry: ``>= 0`` its offset in the interior
        row, ``<= -2`` the halo row's entry ``-2 - arg``, ``-1`` no entry. Interior entries
        come first: a halo entry wins only if strictly better. ``halo_rows`` as in
        :meth:`aggregate` (no exchange)."""
        self.edges_aggregated += self.nnz
        F = x.shape[1]
        it = self.interior
        if out is None:
            out = torch.empty(self.L, F, dtype=x.dtype, device=x.device)
        arg = torch.empty(out.shape[0], F, dtype=torch.int32, device=x.device)
        if self.halo is None:
            return K.segment_extreme(it.rowptr, it.col, x, out, arg, minimum=minimum)
        hc = self.halo.compact_rows()
        if halo_rows is not None:
            K.segment_extreme(it.rowptr, it.col, x, out, arg, minimum=minimum)
            return K.segment_extreme(hc.rowptr, hc.col, halo_rows, out, arg, minimum=minimum,
                                     second=True, row_map=hc.row_map)
        # the exchanges depend on the plan alone (a rank with sends and no halo row posts
        # them too); column chunks as in aggregate()
        pend = []
        for c0, c1 in self._col_chunks(self.a2a, F, x.element_size()):
            xc = x if (c0, c1) == (0, F) else x[:, c0:c1]
            recv, work = self.a2a(K.gather_rows(xc, self.send_map.idx), async_op=True)
            if not self.overlap:
                work.wait()
            pend.append((c0, c1, recv, work))
        K.segment_extreme(it.rowptr, it.col, x, out, arg, minimum=minimum)
        for c0, c1, recv, work in pend:
            work.wait()
            whole = (c0, c1) == (0, F)
            K.segment_extreme(hc.rowptr, hc.col, recv, out if whole else out[:, c0:c1],
                              arg if whole else arg[:, c0:c1], minimum=minimum, second=True,
                              row_map=hc.row_map)
        return out, arg

    def aggregate_extreme_T(self, g: torch.Tensor, arg: torch.Tensor,
                            out: Optional[torch.Tensor] = None,
                            halo_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Backward of :meth:`aggregate_extreme`: ``g[r, f]`` goes, whole, to the source of
        the entry ``arg[r, f]`` names. Interior winners are gathered over the interior's
        transposed pattern (always the real transpose: ``arg`` is not symmetric even when
        the pattern is), halo winners over the halo block's into ``[H, F]`` rows, which
        then take the reverse path of :meth:`aggregate_T` (reverse exchange, owner-side
        segment sum). ``halo_out``: ``[H, F]`` buffer that keeps the halo gradient here."""
        g = g.contiguous()
        F = g.shape[1]
        it, irel = self.interior.transpose_rel()
        self.edges_aggregated += it.nnz + (self.halo.nnz if self.halo is not None else 0)
        if self.halo is None:
            return K.segment_extreme_bwd(it.rowptr, it.col, irel, g, arg, out)
        ht, hrel = self.halo.transpose_rel()
        if halo_out is not None:
            K.segment_extreme_bwd(ht.rowptr, ht.col, hrel, g, arg, halo_out, halo=True)
            return K.segment_extreme_bwd(it.rowptr, it.col, irel, g, arg, out)
        pend = []
        for c0, c1 in self._col_chunks(self.a2a_rev, F, g.element_size()):
            whole = (c0, c1) == (0, F)
            hg = K.segment_extreme_bwd(ht.rowptr, ht.col, hrel, g if whole else g[:, c0:c1],
                                       arg if whole else arg[:, c0:c1], halo=True)
            sg, work = self.a2a_rev(hg, async_op=True)
            if not self.overlap:
                work.wait()
            pend.append((c0, c1, sg, work))
        out = K.segment_extreme_bwd(it.rowptr, it.col, irel, g, arg, out)
        st = self.send_map.transpose_csr().compact_rows()
        for c0, c1, sg, work in pend:
            work.wait()
            oc = out if (c0, c1) == (0, F) else out[:, c0:c1]
            K.spmm(st.rowptr, st.col, sg, oc, beta=1.0, split=_hs(st), row_map=st.row_map)
        return out

    def _drop_ids(self):
        """``(ids of the local rows [L], ids of the halo rows [H])`` the DropEdge decision is
        keyed by, or ``(None, None)`` for the local numbering (halo row j is L + j)."""
        v = self.vertex_ids
        if v is None:
            return None, None
        if v.dtype != torch.int64 or v.dim() != 1 or v.numel() != self.L + self.H:
            raise ValueError(f"vertex_ids must be int64 [{self.L + self.H}] (local rows, then "
                             f"halo rows), got {v.dtype} {tuple(v.shape)}")
        if v.device != self.device:
            v = self.vertex_ids = v.to(self.device)
        return v[:self.L], v[self.L:]

    def aggregate_drop(self, x: torch.Tensor, drop, mean: bool = True,
                       out: Optional[torch.Tensor] = None):
        """Sum / mean over the in-neighbours that ``drop`` (an
        :class:`~dgraph_amd.ops.aggregate.EdgeDrop`) keeps, local and halo, on the schedule
        of :meth:`aggregate`: the exchange is posted, the kept degrees are counted over the
        interior block and then over the compacted halo block, the interior pass runs while
        the halo rows are on the links, and the halo pass adds to it (``beta = 1``), both with
        ``row_scale = 1 / max(kept, 1)`` for mean. Returns ``(out, kept)``; ``kept`` (int32
        ``[L]``, ``None`` for sum) is what :meth:`aggregate_drop_T` needs. The decision is
        keyed by :attr:`vertex_ids`. Whole rows in one exchange: no column chunks, no
        ``static=`` / ``halo_rows=``; fp32 rows on the GPU."""
        self.edges_aggregated += self.nnz  # entries visited, kept or not
        kw = dict(seed=drop.seed, p=drop.p, undirected=drop.undirected)
        loc, hal = self._drop_ids()
        it, hc = self.interior, None
        x = vec_rows(x)
        if out is None:
            out = torch.empty(self.L, x.shape[1], dtype=x.dtype, device=x.device)
        if self.halo is not None:
            # the exchange depends on the plan alone (a rank with sends and no halo row
            # posts it too)
            recv, work = self.a2a(K.gather_rows(x, self.send_map.idx), async_op=True)
            if not self.overlap:
                work.wait()
            hc = self.halo.compact_rows()
        kept = rs = None
        if mean:
            kept = K.kept_degree(it.rowptr, it.col, row_ids=loc, col_ids=loc, num_cols=self.L,
                                 **kw)
            if hc is not None:
                K.kept_degree(hc.rowptr, hc.col, kept, accumulate=True, row_map=hc.row_map,
                              row_ids=loc, col_ids=hal, num_cols=self.H, col_base=self.L, **kw)
            rs = inv_kept(kept, x.dtype)
        K.spmm_drop(it.rowptr, it.col, x, out, row_scale=rs, row_ids=loc, col_ids=loc, **kw)
        if hc is not None:
            work.wait()
            K.spmm_drop(hc.rowptr, hc.col, recv, out, row_scale=rs, beta=1.0,
                        row_map=hc.row_map, row_ids=loc, col_ids=hal, col_base=self.L, **kw)
        return out, kept

    def aggregate_drop_T(self, g: torch.Tensor, drop, mean: bool = True,
                         kept: Optional[torch.Tensor] = None,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Transposed :meth:`aggregate_drop` (its backward, with the same ``drop``) on the
        schedule of :meth:`aggregate_T`: halo-transposed pass, reverse exchange,
        interior-transposed pass, owner-side segment sum. The passes run over the transposed
        blocks with ``transposed=True``, which regenerates the forward's decisions from the
        vertex ids; a ``symmetric`` interior runs on itself. ``kept``: the forward's kept
        degrees (mean)."""
        if mean and kept is None:
            raise ValueError("aggregate_drop_T: mean needs the forward's kept degrees")
        kw = dict(seed=drop.seed, p=drop.p, undirected=drop.undirected, transposed=True)
        loc, hal = self._drop_ids()
        g = vec_rows(g)
        cs = inv_kept(kept, g.dtype) if mean else None
        it = self.interior.transpose()  # the interior itself when symmetric
        self.edges_aggregated += it.nnz + (self.halo.nnz if self.halo is not None else 0)
        if self.halo is not None:
            ht = self.halo.transpose()
            hg = K.spmm_drop(ht.rowptr, ht.col, g, col_scale=cs, row_ids=hal, col_ids=loc,
                             row_base=self.L, **kw)
            sg, work = self.a2a_rev(hg, async_op=True)
            if not self.overlap:
                work.wait()
        out = K.spmm_drop(it.rowptr, it.col, g, out, col_scale=cs, row_ids=loc, col_ids=loc,
                          **kw)
        if self.halo is not None:
            work.wait()
            st = self.send_map.transpose_csr().compact_rows()
            K.spmm(st.rowptr, st.col, sg, out, beta=1.0, split=_hs(st), row_map=st.row_map)
        return out

    def degree(self) -> torch.Tensor:
        """Total in-degree of every local vertex (interior + halo entries), int64."""
        deg = self.interior.degree()
        return deg + self.halo.degree() if self.halo is not None else deg

    def _inv_deg_as(self, dtype) -> torch.Tensor:
        if dtype == torch.float64:  # the CPU reference at full precision
            return 1.0 / self.degree().clamp(min=1).double()
        return self.inv_deg

    def aggregate_multi(self, x: torch.Tensor, aggregators=("mean", "max", "min", "std"),
                        eps: float = 1e-5, halo_rows: Optional[torch.Tensor] = None):
        """Mean / max / min / standard deviation over in-neighbours, local and halo, from
        ONE pass per block over the neighbour rows (:func:`~dgraph_amd.ops.kernels.
        segment_pna`), on the schedule of :meth:`aggregate_extreme`: the interior pass runs
        (non-final) while the halo rows are on the links, then the halo block is merged in
        as a second source over all ``L`` rows, which finalises them. Returns ``(out,
        saved)``: ``out`` is ``[L, A*F]``, one column block per name in ``aggregators``;
        ``saved`` is what :meth:`aggregate_multi_T` needs (``mean``, ``sdev``, ``amax``,
        ``amin`` and ``halo``, the halo rows this pass read: the std term of the gradient
        needs ``x`` of the halo sources). ``halo_rows`` as in :meth:`aggregate`."""
        aggs = check_aggregators(aggregators)
        self.edges_aggregated += self.nnz
        L, F = self.L, x.shape[1]
        it = self.interior
        new = lambda dt: torch.empty(L, F, dtype=dt, device=x.device)  # noqa: E731
        out = torch.empty(L, len(aggs) * F, dtype=x.dtype, device=x.device)
        blk = multi_blocks(out, aggs, F)
        o = dict(mean=blk.get("mean"), sdev=blk.get("std"), vmax=blk.get("max"),
                 vmin=blk.get("min"), amax=None, amin=None)
        if o["mean"] is not None or o["sdev"] is not None:
            o["mean"] = new(x.dtype) if o["mean"] is None else o["mean"]
            o["sdev"] = new(x.dtype) if o["sdev"] is None else o["sdev"]
        if o["vmax"] is not None:
            o["amax"] = new(torch.int32)
        if o["vmin"] is not None:
            o["amin"] = new(torch.int32)
        saved = dict(mean=o["mean"], sdev=o["sdev"], amax=o["amax"], amin=o["amin"], halo=None)
        # a halo block with no entry (a rank that only sends) changes nothing: the interior
        # pass is then final; the exchanges are posted all the same
        two = self.halo is not None and self.halo.nnz > 0
        if self.halo is None or halo_rows is not None:
            K.segment_pna(it.rowptr, it.col, x, eps=eps, final=not two, **o)
            if two:
                K.segment_pna(self.halo.rowptr, self.halo.col, halo_rows, eps=eps, second=True,
                              prev_rowptr=it.rowptr, **o)
            saved["halo"] = halo_rows
            return out, saved
        pend = []
        for c0, c1 in self._col_chunks(self.a2a, F, x.element_size()):
            xc = x if (c0, c1) == (0, F) else x[:, c0:c1]
            recv, work = self.a2a(K.gather_rows(xc, self.send_map.idx), async_op=True)
            if not self.overlap:
                work.wait()
            pend.append((c0, c1, recv, work))
        K.segment_pna(it.rowptr, it.col, x, eps=eps, final=not two, **o)
        for c0, c1, recv, work in pend:
            work.wait()
            if two:
                oc = o if (c0, c1) == (0, F) else \
                    {k: None if v is None else v[:, c0:c1] for k, v in o.items()}
                K.segment_pna(self.halo.rowptr, self.halo.col, recv, eps=eps, second=True,
                              prev_rowptr=it.rowptr, **oc)
        saved["halo"] = pend[0][2] if len(pend) == 1 else torch.cat([p[2] for p in pend], 1)
        return out, saved

    def aggregate_multi_T(self, g: torch.Tensor, x: torch.Tensor, saved: dict,
                          aggregators=("mean", "max", "min", "std"),
                          out: Optional[torch.Tensor] = None,
                          halo_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Backward of :meth:`aggregate_multi` (``g``: ``[L, A*F]``, ``x`` and ``saved``:
        the forward's input and second result). The moments' gradient and the interior
        winners are gathered over the interior's transposed pattern with ``x``, the halo
        block's over its transposed pattern with the kept halo rows into ``[H, F]`` rows,
        which then take the reverse path of :meth:`aggregate_extreme_T` (reverse exchange,
        owner-side segment sum). ``halo_out``: ``[H, F]`` buffer that keeps the halo
        gradient here."""
        aggs = check_aggregators(aggregators)
        F = x.shape[1]
        gb = multi_blocks(g.contiguous(), aggs, F)
        it, irel = self.interior.transpose_rel()
        self.edges_aggregated += it.nnz + (self.halo.nnz if self.halo is not None else 0)
        inv = self._inv_deg_as(x.dtype)
        kw = dict(g_mean=gb.get("mean"), g_std=gb.get("std"), mean=saved["mean"],
                  sdev=saved["sdev"], g_max=gb.get("max"), amax=saved["amax"],
                  g_min=gb.get("min"), amin=saved["amin"])
        if self.halo is None:
            return K.segment_pna_bwd(it.rowptr, it.col, irel, x, inv, out, **kw)
        ht, hrel = self.halo.transpose_rel()
        xh = saved["halo"]
        if halo_out is not None:
            K.segment_pna_bwd(ht.rowptr, ht.col, hrel, xh, inv, halo_out, halo=True, **kw)
            return K.segment_pna_bwd(it.rowptr, it.col, irel, x, inv, out, **kw)
        pend = []
        for c0, c1 in self._col_chunks(self.a2a_rev, F, g.element_size()):
            whole = (c0, c1) == (0, F)
            kc = kw if whole else {k: None if v is None else v[:, c0:c1] for k, v in kw.items()}
            hg = K.segment_pna_bwd(ht.rowptr, ht.col, hrel, xh if whole else xh[:, c0:c1], inv,
                                   halo=True, **kc)
            sg, work = self.a2a_rev(hg, async_op=True)
            if not self.overlap:
                work.wait()
            pend.append((c0, c1, sg, work))
        out = K.segment_pna_bwd(it.rowptr, it.col, irel, x, inv, out, **kw)
        st = self.send_map.transpose_csr().compact_rows()
        for c0, c1, sg, work in pend:
            work.wait()
            oc = out if (c0, c1) == (0, F) else out[:, c0:c1]
            K.spmm(st.rowptr, st.col, sg, oc, beta=1.0, split=_hs(st), row_map=st.row_map)
        return out

    def aggregate_softmax(self, x: torch.Tensor, t: torch.Tensor,
                          halo_rows: Optional[torch.Tensor] = None):
        """Softmax aggregation over in-neighbours, local and halo (``out[r, f] = sum_j
        softmax_j(t_f x[j, f]) x[j, f]``, :func:`~dgraph_amd.ops.kernels.segment_softmax`),
        on the schedule of :meth:`aggregate_multi`: the interior pass runs while the halo
        rows are on the links, then the halo block is run over all ``L`` rows starting from
        the interior's ``(out, lse)``. ``t``: the ``[F]`` temperature. Returns ``(out,
        saved)``; ``saved`` is what :meth:`aggregate_softmax_T` needs (``out``, ``lse`` and
        ``halo``, the halo rows this pass read). ``halo_rows`` as in :meth:`aggregate`."""
        self.edges_aggregated += self.nnz
        L, F = self.L, x.shape[1]
        it = self.interior
        out = torch.empty(L, F, dtype=x.dtype, device=x.device)
        lse = torch.empty(L, F, dtype=x.dtype, device=x.device)
        saved = dict(out=out, lse=lse, halo=None)
        if self.halo is None or halo_rows is not None:
            K.segment_softmax(it.rowptr, it.col, x, t, out, lse)
            if self.halo is not None:
                K.segment_softmax(self.halo.rowptr, self.halo.col, halo_rows, t, out, lse,
                                  second=True)
            saved["halo"] = halo_rows
            return out, saved
        # the exchanges depend on the plan alone (a rank with sends and no halo entry posts
        # them too); column chunks as in aggregate()
        pend = []
        for c0, c1 in self._col_chunks(self.a2a, F, x.element_size()):
            xc = x if (c0, c1) == (0, F) else x[:, c0:c1]
            recv, work = self.a2a(K.gather_rows(xc, self.send_map.idx), async_op=True)
            if not self.overlap:
                work.wait()
            pend.append((c0, c1, recv, work))
        K.segment_softmax(it.rowptr, it.col, x, t, out, lse)
        for c0, c1, recv, work in pend:
            work.wait()
            whole = (c0, c1) == (0, F)
            K.segment_softmax(self.halo.rowptr, self.halo.col, recv, t if whole else t[c0:c1],
                              out if whole else out[:, c0:c1],
                              lse if whole else lse[:, c0:c1], second=True)
        saved["halo"] = pend[0][2] if len(pend) == 1 else torch.cat([p[2] for p in pend], 1)
        return out, saved

    def aggregate_softmax_T(self, g: torch.Tensor, x: torch.Tensor, t: torch.Tensor,
                            saved: dict, out: Optional[torch.Tensor] = None,
                            halo_out: Optional[torch.Tensor] = None, want_dt: bool = True):
        """Backward of :meth:`aggregate_softmax` (``g``: ``[L, F]``; ``x``, ``t`` and
        ``saved``: the forward's inputs and second result). Every weight is recomputed from
        the final ``(out, lse)``: the interior entries over the interior's transposed
        pattern with ``x``, the halo block's over its transposed pattern with the kept halo
        rows into ``[H, F]`` rows, which then take the reverse path of
        :meth:`aggregate_multi_T` (reverse exchange under the interior pass, owner-side
        segment sum). ``halo_out``: ``[H, F]`` buffer that keeps the halo gradient here.
        Returns ``(dx, dt)``; ``dt`` (``[F]``, or ``None`` without ``want_dt``) is this
        rank's part: the sum over its interior and halo entries, to be all-reduced with the
        other replicated parameters' gradients."""
        g = vec_rows(g)
        F = x.shape[1]
        it = self.interior if self.interior.symmetric else self.interior.transpose()
        self.edges_aggregated += it.nnz + (self.halo.nnz if self.halo is not None else 0)
        of, lse = saved["out"], saved["lse"]
        dt = None

        def add_dt(part, c0=0, c1=F):
            nonlocal dt
            if part is None:
                return
            if dt is None:
                dt = torch.zeros(F, dtype=part.dtype, device=part.device)
            dt[c0:c1] += part.sum(0)

        if self.halo is None:
            dx, part = K.segment_softmax_bwd(it.rowptr, it.col, x, t, g, of, lse, out, want_dt)
            add_dt(part)
            return dx, dt
        ht = self.halo.transpose()
        xh = saved["halo"]
        if halo_out is not None:
            _, part = K.segment_softmax_bwd(ht.rowptr, ht.col, xh, t, g, of, lse, halo_out,
                                            want_dt)
            add_dt(part)
            dx, part = K.segment_softmax_bwd(it.rowptr, it.col, x, t, g, of, lse, out, want_dt)
            add_dt(part)
            return dx, dt
        pend = []
        for c0, c1 in self._col_chunks(self.a2a_rev, F, g.element_size()):
            whole = (c0, c1) == (0, F)
            cut = (lambda v: v) if whole else (lambda v: v[:, c0:c1])  # noqa: E731
            hg, part = K.segment_softmax_bwd(ht.rowptr, ht.col, cut(xh), t if whole else t[c0:c1],
                                             cut(g), cut(of), cut(lse), None, want_dt)
            add_dt(part, c0, c1)
            sg, work = self.a2a_rev(hg, async_op=True)
            if not self.overlap:
                work.wait()
            pend.append((c0, c1, sg, work))
        dx, part = K.segment_softmax_bwd(it.rowptr, it.col, x, t, g, of, lse, out, want_dt)
        add_dt(part)
        st = self.send_map.transpose_csr().compact_rows()
        for c0, c1, sg, work in pend:
            work.wait()
            oc = dx if (c0, c1) == (0, F) else dx[:, c0:c1]
            K.spmm(st.rowptr, st.col, sg, oc, beta=1.0, split=_hs(st), row_map=st.row_map)
        return dx, dt

    def aggregate_gated(self, k: torch.Tensor, qv: torch.Tensor,
                        halo_rows: Optional[torch.Tensor] = None):
        """Gated aggregation over in-neighbours, local and halo (``out[r, f] = sum_j
        sigmoid(k[r, f] + q[j, f]) v[j, f]``, :func:`~dgraph_amd.ops.kernels.segment_gated`),
        on the schedule of :meth:`aggregate_softmax`. ``k``: ``[L, F]``; ``qv``: the local
        ``[L, 2F]`` source buffer ``[q | v]``, whose ``send_map`` rows go on the links as ONE
        message while the interior pass runs; the halo block is then added over all ``L``
        rows. Returns ``(out, saved)``; ``saved`` is what :meth:`aggregate_gated_T` needs
        (``ds``, the destination-side state ``sum_j s (1 - s) v_j``, and ``halo``, the ``[H,
        2F]`` halo rows this pass read). ``halo_rows`` as in :meth:`aggregate`."""
        self.edges_aggregated += self.nnz
        L, F = self.L, k.shape[1]
        if qv.dim() != 2 or qv.shape[1] != 2 * F:
            raise ValueError(f"aggregate_gated: qv must be [L, {2 * F}] ([q | v]), got "
                             f"{tuple(qv.shape)}")
        it = self.interior
        out = torch.empty(L, F, dtype=k.dtype, device=k.device)
        ds = torch.empty(L, F, dtype=k.dtype, device=k.device)
        saved = dict(ds=ds, halo=None)
        if self.halo is None or halo_rows is not None:
            K.segment_gated(it.rowptr, it.col, k, qv[:, :F], qv[:, F:], out, ds)
            if self.halo is not None:
                K.segment_gated(self.halo.rowptr, self.halo.col, k, halo_rows[:, :F],
                                halo_rows[:, F:], out, ds, accumulate=True)
            saved["halo"] = halo_rows
            return out, saved
        # the exchanges depend on the plan alone (a rank with sends and no halo entry posts
        # them too); a column chunk carries the same channel range of q and of v
        idx = self.send_map.idx
        pend = []
        for c0, c1 in self._col_chunks(self.a2a, F, 2 * k.element_size()):
            if (c0, c1) == (0, F):
                send = K.gather_rows(qv, idx)
            else:
                w = c1 - c0
                send = torch.empty(idx.numel(), 2 * w, dtype=qv.dtype, device=qv.device)
                K.copy_rows(qv[:, c0:c1], src_idx=idx, out=send[:, :w])
                K.copy_rows(qv[:, F + c0:F + c1], src_idx=idx, out=send[:, w:])
            recv, work = self.a2a(send, async_op=True)
            if not self.overlap:
                work.wait()
            pend.append((c0, c1, recv, work))
        K.segment_gated(it.rowptr, it.col, k, qv[:, :F], qv[:, F:], out, ds)
        for c0, c1, recv, work in pend:
            work.wait()
            whole, w = (c0, c1) == (0, F), c1 - c0
            K.segment_gated(self.halo.rowptr, self.halo.col, k if whole else k[:, c0:c1],
                            recv[:, :w], recv[:, w:], out if whole else out[:, c0:c1],
                            ds if whole else ds[:, c0:c1], accumulate=True)
        if len(pend) == 1:
            saved["halo"] = pend[0][2]
        else:  # back to [q | v]
            saved["halo"] = torch.cat([p[2][:, :p[1] - p[0]] for p in pend] +
                                      [p[2][:, p[1] - p[0]:] for p in pend], 1)
        return out, saved

    def aggregate_gated_T(self, g: torch.Tensor, k: torch.Tensor, qv: torch.Tensor,
                          saved: dict):
        """Backward of :meth:`aggregate_gated` (``g``: ``[L, F]``; ``k``, ``qv`` and
        ``saved``: the forward's inputs and second result). The destination side is ``dk = g
        * ds``, no kernel. The source side recomputes every gate: the interior entries over
        the interior's transposed pattern with the local ``[q | v]`` into ``d[q | v]``, the
        halo block's over its transposed pattern with the kept halo rows into ``[H, 2F]``
        rows, which then take the reverse path of :meth:`aggregate_softmax_T` as one message
        (reverse exchange under the interior pass, owner-side segment sum). Returns ``(dk,
        dqv)``."""
        g = vec_rows(g)
        L, F = self.L, k.shape[1]
        it = self.interior if self.interior.symmetric else self.interior.transpose()
        self.edges_aggregated += it.nnz + (self.halo.nnz if self.halo is not None else 0)
        dk = g * saved["ds"]
        dqv = torch.empty(L, 2 * F, dtype=k.dtype, device=k.device)
        q, v, dq, dv = qv[:, :F], qv[:, F:], dqv[:, :F], dqv[:, F:]
        if self.halo is None:
            K.segment_gated_bwd_src(it.rowptr, it.col, k, q, v, g, dq, dv)
            return dk, dqv
        ht = self.halo.transpose()
        qvh = saved["halo"]
        pend = []
        for c0, c1 in self._col_chunks(self.a2a_rev, F, 2 * g.element_size()):
            whole, w = (c0, c1) == (0, F), c1 - c0
            cut = (lambda t: t) if whole else (lambda t: t[:, c0:c1])  # noqa: E731
            hg = torch.empty(ht.num_rows, 2 * w, dtype=k.dtype, device=k.device)
            K.segment_gated_bwd_src(ht.rowptr, ht.col, cut(k), qvh[:, c0:c1],
                                    qvh[:, F + c0:F + c1], cut(g), hg[:, :w], hg[:, w:])
            sg, work = self.a2a_rev(hg, async_op=True)
            if not self.overlap:
                work.wait()
            pend.append((c0, c1, sg, work))
        K.segment_gated_bwd_src(it.rowptr, it.col, k, q, v, g, dq, dv)
        st = self.send_map.transpose_csr().compact_rows()
        for c0, c1, sg, work in pend:
            work.wait()
            if (c0, c1) == (0, F):  # the message has the layout of dqv
                K.spmm(st.rowptr, st.col, sg, dqv, beta=1.0, split=_hs(st), row_map=st.row_map)
                continue
            w = c1 - c0
            for src, dst in ((sg[:, :w], dq[:, c0:c1]), (sg[:, w:], dv[:, c0:c1])):
                K.spmm(st.rowptr, st.col, src, dst, beta=1.0, split=_hs(st),
                       row_map=st.row_map)
        return dk, dqv

    def _edge_blocks(self, e_int, e_halo, x: torch.Tensor, name: str):
        """The per-slot edge rows of the two blocks, checked: ``e_int`` ``[interior.nnz, F]``
        and ``e_halo`` ``[halo.nnz, F]`` (``None`` where the block has no entry)."""
        F = x.shape[1]
        blocks = []
        for blk, e, nm in ((self.interior, e_int, "e_int"), (self.halo, e_halo, "e_halo")):
            n = blk.nnz if blk is not None else 0
            if e is None:
                e = x.new_empty(0, F)
            if e.dim() != 2 or tuple(e.shape) != (n, F):
                raise ValueError(f"{name}: {nm} must be [{n}, {F}] (one row per slot of the "
                                 f"block), got {tuple(e.shape)}")
            blocks.append(vec_rows(e))
        return blocks

    def aggregate_softmax_edge(self, x: torch.Tensor, e_int: torch.Tensor,
                               e_halo: Optional[torch.Tensor], t: torch.Tensor,
                               relu: bool = True, eps: float = 1e-7,
                               halo_rows: Optional[torch.Tensor] = None):
        """Softmax aggregation of per-edge messages ``relu(x[j] + e_ij) + eps`` over the
        in-neighbours, local and halo (:func:`~dgraph_amd.ops.kernels.segment_softmax_edge`),
        on the schedule of :meth:`aggregate_softmax`: the exchange of the ``x`` send rows is
        posted first, the interior block runs under it, then the halo block runs over all
        ``L`` rows starting from the interior's ``(out, lse)``. The edge rows never travel:
        ``e_int`` / ``e_halo`` are this rank's per-slot rows of ``self.interior`` /
        ``self.halo`` (one block per CSR block, as :meth:`edge_dot` returns its scores;
        :meth:`~dgraph_amd.ops.csr.CSR.split_edge_values` cuts per-slot values of the unsplit
        pattern into them). ``t``: the ``[F]`` temperature. Returns ``(out, saved)`` with
        ``saved`` as :meth:`aggregate_softmax`'s."""
        self.edges_aggregated += self.nnz
        L, F = self.L, x.shape[1]
        it = self.interior
        e_int, e_halo = self._edge_blocks(e_int, e_halo, x, "aggregate_softmax_edge")
        out = torch.empty(L, F, dtype=x.dtype, device=x.device)
        lse = torch.empty(L, F, dtype=x.dtype, device=x.device)
        saved = dict(out=out, lse=lse, halo=None)
        kw = dict(relu=relu, eps=eps)
        if self.halo is None or halo_rows is not None:
            K.segment_softmax_edge(it.rowptr, it.col, x, e_int, t, out, lse, **kw)
            if self.halo is not None:
                K.segment_softmax_edge(self.halo.rowptr, self.halo.col, halo_rows, e_halo, t,
                                       out, lse, second=True, **kw)
            saved["halo"] = halo_rows
            return out, saved
        # the exchanges depend on the plan alone (a rank with sends and no halo entry posts
        # them too); column chunks as in aggregate()
        pend = []
        for c0, c1 in self._col_chunks(self.a2a, F, x.element_size()):
            xc = x if (c0, c1) == (0, F) else x[:, c0:c1]
            recv, work = self.a2a(K.gather_rows(xc, self.send_map.idx), async_op=True)
            if not self.overlap:
                work.wait()
            pend.append((c0, c1, recv, work))
        K.segment_softmax_edge(it.rowptr, it.col, x, e_int, t, out, lse, **kw)
        for c0, c1, recv, work in pend:
            work.wait()
            whole = (c0, c1) == (0, F)
            K.segment_softmax_edge(self.halo.rowptr, self.halo.col, recv,
                                   e_halo if whole else e_halo[:, c0:c1],
                                   t if whole else t[c0:c1],
                                   out if whole else out[:, c0:c1],
                                   lse if whole else lse[:, c0:c1], second=True, **kw)
        saved["halo"] = pend[0][2] if len(pend) == 1 else torch.cat([p[2] for p in pend], 1)
        return out, saved

    def aggregate_softmax_edge_T(self, g: torch.Tensor, x: torch.Tensor, e_int: torch.Tensor,
                                 e_halo: Optional[torch.Tensor], t: torch.Tensor, saved: dict,
                                 relu: bool = True, eps: float = 1e-7,
                                 out: Optional[torch.Tensor] = None,
                                 halo_out: Optional[torch.Tensor] = None,
                                 want_dt: bool = True):
        """Backward of :meth:`aggregate_softmax_edge` (``g``: ``[L, F]``; the other arguments
        are the forward's inputs and second result). Each block runs the destination-side
        kernel over its own pattern with the final ``(out, lse)``, which writes the block's
        edge gradient; the source gradient is the row sum of those rows over the block's
        slot-transposed pattern. The halo block goes first: its sums are the ``[H, F]`` rows
        that take the reverse path of :meth:`aggregate_softmax_T` (reverse exchange under the
        interior block, owner-side segment sum). ``halo_out``: ``[H, F]`` buffer that keeps
        the halo gradient here. Returns ``(dx, de_int, de_halo, dt)``; ``de_halo`` is ``[0,
        F]`` without halo entries, and ``dt`` (``[F]``, or ``None`` without ``want_dt``) is
        this rank's part, as :meth:`aggregate_softmax_T`'s."""
        from ..ops.aggregate import sum_edge_rows

        g = vec_rows(g)
        F = x.shape[1]
        it = self.interior
        e_int, e_halo = self._edge_blocks(e_int, e_halo, x, "aggregate_softmax_edge_T")
        self.edges_aggregated += self.nnz
        of, lse = saved["out"], saved["lse"]
        kw = dict(relu=relu, eps=eps, want_dt=want_dt)
        dt = None

        def add_dt(part, c0=0, c1=F):
            nonlocal dt
            if part is None:
                return
            if dt is None:
                dt = torch.zeros(F, dtype=part.dtype, device=part.device)
            dt[c0:c1] += part.sum(0)

        def interior():
            de, part = K.segment_softmax_edge_bwd(it.rowptr, it.col, x, e_int, t, g, of, lse,
                                                  **kw)
            add_dt(part)
            return sum_edge_rows(it, de, out, SPMM_HUB_CAP), de

        def halo_sum(de, into=None):
            # [H, w]: a halo block without entries (a rank that only sends) sums to nothing
            if self.halo.nnz == 0:
                return de.new_zeros(self.H, de.shape[1]) if into is None else into.zero_()
            return sum_edge_rows(self.halo, de, into, SPMM_HUB_CAP)

        if self.halo is None:
            dx, de_int = interior()
            return dx, de_int, x.new_empty(0, F), dt
        ht = self.halo
        xh = saved["halo"]
        de_halo = torch.empty(ht.nnz, F, dtype=x.dtype, device=x.device)
        if halo_out is not None:
            _, part = K.segment_softmax_edge_bwd(ht.rowptr, ht.col, xh, e_halo, t, g, of, lse,
                                                 de_halo, **kw)
            add_dt(part)
            halo_sum(de_halo, halo_out)
            dx, de_int = interior()
            return dx, de_int, de_halo, dt
        pend = []
        for c0, c1 in self._col_chunks(self.a2a_rev, F, g.element_size()):
            whole = (c0, c1) == (0, F)
            cut = (lambda v: v) if whole else (lambda v: v[:, c0:c1])  # noqa: E731
            dec, part = K.segment_softmax_edge_bwd(ht.rowptr, ht.col, cut(xh), cut(e_halo),
                                                   t if whole else t[c0:c1], cut(g), cut(of),
                                                   cut(lse), cut(de_halo), **kw)
            add_dt(part, c0, c1)
            sg, work = self.a2a_rev(halo_sum(dec), async_op=True)
            if not self.overlap:
                work.wait()
            pend.append((c0, c1, sg, work))
        dx, de_int = interior()
        st = self.send_map.transpose_csr().compact_rows()
        for c0, c1, sg, work in pend:
            work.wait()
            oc = dx if (c0, c1) == (0, F) else dx[:, c0:c1]
            K.spmm(st.rowptr, st.col, sg, oc, beta=1.0, split=_hs(st), row_map=st.row_map)
        return dx, de_int, de_halo, dt

    def edge_dot(self, a: torch.Tensor, b: torch.Tensor, heads: int = 1, scale: float = 1.0,
                 halo_rows: Optional[torch.Tensor] = None):
        """One score per edge at this rank's vertices, local and halo sources
        (:func:`~dgraph_amd.ops.kernels.edge_dot`): ``scale * <a[i], b[j]>`` per head for
        every entry ``(i, j)``, with ``b``'s halo rows fetched from their owners. The halo
        exchange of ``b``'s send rows is posted first, the interior block is scored while
        they are on the links, then the halo block on the received rows. Returns
        ``(s_interior, s_halo, saved)``: each block's scores in its own slot order
        (``self.interior`` / ``self.halo``; ``s_halo`` is ``[0, heads]`` without a halo
        block), and what :meth:`edge_dot_T` needs. Whole rows are exchanged: a dot product
        cannot be cut by columns without carrying a partial score from chunk to chunk, so
        there is no column-chunked exchange here. ``halo_rows`` as in :meth:`aggregate`."""
        self.edges_aggregated += self.nnz
        it = self.interior
        saved = dict(halo=None, heads=int(heads), scale=float(scale))
        if self.halo is None or halo_rows is not None:
            s_int = K.edge_dot(it.rowptr, it.col, a, b, heads=heads, scale=scale)
            if self.halo is None:
                return s_int, s_int.new_zeros(0, heads), saved
            saved["halo"] = halo_rows
            return s_int, K.edge_dot(self.halo.rowptr, self.halo.col, a, halo_rows,
                                     heads=heads, scale=scale), saved
        # the exchange depends on the plan alone (a rank with sends and no halo entry posts
        # it too)
        recv, work = self.a2a(K.gather_rows(b, self.send_map.idx), async_op=True)
        if not self.overlap:
            work.wait()
        s_int = K.edge_dot(it.rowptr, it.col, a, b, heads=heads, scale=scale)
        work.wait()
        saved["halo"] = recv
        return s_int, K.edge_dot(self.halo.rowptr, self.halo.col, a, recv, heads=heads,
                                 scale=scale), saved

    def edge_dot_T(self, g_int: torch.Tensor, g_halo: torch.Tensor, a: torch.Tensor,
                   b: torch.Tensor, saved: dict, halo_out: Optional[torch.Tensor] = None):
        """Backward of :meth:`edge_dot` (``g_int`` / ``g_halo``: the gradients of the two
        score blocks; ``a``, ``b`` and ``saved``: the forward's inputs and third result), as
        edge-weighted SpMMs. ``da``: the interior block over ``b`` and the halo block over the
        kept halo rows (``beta=1``). ``db``: the halo block's transposed SpMM into ``[H, F]``
        rows first, which go home by the reverse exchange while the interior's transposed
        SpMM runs, then the owner-side segment sum of the received rows. ``halo_out``:
        ``[H, F]`` buffer that keeps the halo gradient here instead (no exchange; the
        ``halo_rows`` mode of the forward). Returns ``(da, db)``."""
        from ..ops.aggregate import _slot_transpose, edge_dot_grads

        heads, scale = saved["heads"], saved["scale"]
        it = self.interior
        self.edges_aggregated += it.nnz + (self.halo.nnz if self.halo is not None else 0)

        def weights(g, csr):
            w = g.reshape(csr.nnz, heads)
            return (w * scale if scale != 1.0 else w).contiguous()

        w_int = weights(g_int, it)
        if self.halo is None:
            return edge_dot_grads(it, a, b, w_int, heads)
        w_halo = weights(g_halo, self.halo)
        xh = saved["halo"]
        F = a.shape[1]
        if self.halo.nnz > 0:
            ht = _slot_transpose(self.halo)
            hg = K.spmm(ht.rowptr, ht.col, a, halo_out, edge_weight=w_halo[ht.perm].contiguous(),
                        heads=heads)
        else:
            hg = a.new_zeros(self.H, F) if halo_out is None else halo_out.zero_()
        work = None
        if halo_out is None:  # posted whatever this rank's halo block holds
            sg, work = self.a2a_rev(hg, async_op=True)
            if not self.overlap:
                work.wait()
        da, db = edge_dot_grads(it, a, b, w_int, heads)
        if self.halo.nnz > 0:
            hc = self.halo.compact_rows()
            K.spmm(hc.rowptr, hc.col, xh, da, edge_weight=w_halo, heads=heads, beta=1.0,
                   row_map=hc.row_map)
        if work is not None:
            st = self.send_map.transpose_csr().compact_rows()
            work.wait()
            K.spmm(st.rowptr, st.col, sg, db, beta=1.0, split=_hs(st), row_map=st.row_map)
        return da, db

    def _peers(self) -> bool:
        """True when the plan's peers exist (a process group of the plan's size)."""
        import torch.distributed as dist

        return dist.is_initialized() and dist.get_world_size(self.a2a.group) > 1

    def _restricted(self, rows: torch.Tensor):
        """Cached pieces of :meth:`aggregate_T_rows` for one loss-row set: the transposed
        interior block A[rows, :L]^T, and for the halo block only the halo rows that
        neighbour a loss row (A[rows, halo]^T restricted to its nonzero rows) with a
        matching sub-plan of the reverse exchange, so the owners receive just those rows
        instead of all H (built once, collectively: two small all-to-alls)."""
        hit = _cache_lookup(self._restrict_cache, rows)
        if hit is not None:
            return hit
        it = self.interior.select_rows(rows).transpose()
        cs = self.inv_deg[rows.long()].contiguous()
        sub = None
        if self.halo is not None:
            from ..plan.pattern import _alltoall_counts, _alltoallv_ids

            ht = self.halo.select_rows(rows).transpose()  # [H, |rows|]
            nz = torch.nonzero(ht.degree() > 0).reshape(-1)
            ht_nz = ht.select_rows(nz)
            dev = nz.device
            recv_off = torch.zeros(len(self.a2a.recv_splits) + 1, dtype=torch.long, device=dev)
            recv_off[1:] = torch.cumsum(torch.tensor(self.a2a.recv_splits, device=dev), 0)
            owner = torch.searchsorted(recv_off[1:], nz, right=True)
            W = recv_off.numel() - 1
            cnt = torch.bincount(owner, minlength=W)
            slot = nz - recv_off[owner]
            if self._peers():
                peer_cnt = _alltoall_counts(cnt, self.a2a.group)
            else:  # single-process rehearsal of a W-way rank: mirrored loopback plan
                peer_cnt = cnt.clone()
            cnt_l, peer_l = [int(v) for v in cnt.tolist()], [int(v) for v in peer_cnt.tolist()]
            send_sp = torch.tensor(self.a2a.send_splits, device=dev)
            if self._peers():
                peer_slot = _alltoallv_ids(slot, cnt_l, peer_l, self.a2a.group)
            else:
                # mirrored loopback: peer p's request for slot s lands in my send segment for
                # p (whose length may differ from what I receive from p)
                peer_slot = slot % send_sp[owner].clamp_min(1)
            send_off = torch.zeros(W + 1, dtype=torch.long, device=dev)
            send_off[1:] = torch.cumsum(send_sp, 0)
            base = torch.repeat_interleave(send_off[:-1], peer_cnt.to(dev))
            recv_local = self.send_map.idx.long()[base + peer_slot.to(dev)]
            sub = (ht_nz, AllToAllV(cnt_l, peer_l, self.a2a.group),
                   IndexMap(recv_local, self.L).transpose_csr(), nz, recv_local)
        hit = (it, cs, sub)
        _cache_store(self._restrict_cache, rows, hit)  # one loss-row set at a time
        return hit

    def aggregate_T_rows(self, g_rows: torch.Tensor, rows: torch.Tensor, mean: bool = True,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``aggregate_T(g)`` for a ``g`` that is zero outside ``rows`` (given as the
        ``[len(rows), F]`` nonzero block): the transposed SpMM over A[rows, :] only. For an
        output layer trained on 1 % of the vertices this reads ~1 % of the edges and sends
        back only the halo rows that carry a contribution, with exactly the result of the
        dense call. The first call for a row set is collective (sub-plan exchange)."""
        it, cs_rows, sub = self._restricted(rows)
        g_rows = g_rows.contiguous()
        if mean:
            # the column scale applies to the |rows| gradient rows: scale them once (a
            # 1 %-of-V pass) instead of gathering a per-edge scale inside the SpMM
            g_rows = (g_rows.float() * cs_rows.unsqueeze(1)).to(g_rows.dtype) \
                if g_rows.dtype != torch.float64 else g_rows * cs_rows.unsqueeze(1)
        self.edges_aggregated += it.nnz + (sub[0].nnz if sub is not None else 0)
        # A[rows, :]^T touches only the ~30 % of vertices adjacent to a loss row: run the
        # SpMM over those rows (row-compacted, output row map) and zero-fill the rest,
        # instead of walking all V rows of a 1 %-dense transposed block
        itc = it.compact_rows()
        if out is None:
            out = torch.empty(it.num_rows, g_rows.shape[1], dtype=g_rows.dtype,
                              device=g_rows.device)
        out.zero_()
        if sub is None:
            K.spmm(itc.rowptr, itc.col, g_rows, out, split=_hs(itc), row_map=itc.row_map)
            return out
        ht_nz, a2a_sub, st = sub[:3]
        hg = K.spmm(ht_nz.rowptr, ht_nz.col, g_rows, split=_hs(ht_nz))
        sg, work = a2a_sub(hg, async_op=True)
        if not self.overlap:
            work.wait()
        K.spmm(itc.rowptr, itc.col, g_rows, out, split=_hs(itc), row_map=itc.row_map)
        work.wait()
        K.spmm(st.rowptr, st.col, sg, out, beta=1.0, split=_hs(st))
        return out

    # gradient-support restriction of the transposed aggregation (see grad_support); off
    # with DGRAPH_GRAD_SUPPORT=0. Built only with this much device memory left over.
    GRAD_SUPPORT = os.environ.get("DGRAPH_GRAD_SUPPORT", "1") != "0"
    SUPPORT_HEADROOM = 12 << 30

    def grad_support(self, rows: torch.Tensor):
        """The :meth:`prepare_grad_support` result for ``rows`` (``None`` when it was not
        prepared for this row tensor: then the full transposed block is used)."""
        return _cache_lookup(self._support_cache, rows)

    def prepare_grad_support(self, rows: torch.Tensor):
        """For a loss on ``rows`` with a project-first output layer: the local rows where
        the gradient entering the layer below the output layer can be nonzero — the loss
        rows and their in-neighbours (the rows :meth:`aggregate_T_rows` writes, plus the
        rows the halo sub-plan adds to), and the interior transposed block restricted to
        those columns, ``A^T[:, S]`` (cached per ``rows``, like the restricted plans).

        The transposed aggregation of that gradient then walks only the edges whose
        source lies in S (~30 % of them on the bench graph): exact, the other terms are
        products with rows that are zero by construction. Returns ``None`` when disabled
        or when the restricted block does not fit in device memory. Build it at setup,
        before the training workspace exists (bench.py does so on partitioned graphs; on
        one GPU at the papers100M shape the extra ~5 GB pushed the caching allocator into
        per-step release/re-map stalls: 791 -> 853 ms although the kernels got 80 ms
        faster). Collective on a partitioned graph (the restricted plan)."""
        if not self.GRAD_SUPPORT:
            return None
        hit = _cache_lookup(self._support_cache, rows)
        if hit is not None:
            return hit
        it, _, sub = self._restricted(rows)
        parts = [rows.long(), it.compact_rows().row_map.long()]
        if sub is not None:
            parts.append(sub[4].long())  # local rows the halo sub-plan adds to
        S = torch.unique(torch.cat(parts))
        full = self.interior if self.interior.symmetric else self.interior.transpose()
        res = None
        dev = full.device
        keep_frac = S.numel() / max(self.L, 1)
        # the kept columns (~|S|/L of the entries) + row pointers + chunk temporaries
        need = int(full.col.numel() * keep_frac * 1.1) * full.col.element_size() + \
            2 * full.rowptr.numel() * 8 + (1 << 30)
        free = torch.cuda.mem_get_info(dev)[0] if dev.type == "cuda" else need + (64 << 30)
        if free - need >= self.SUPPORT_HEADROOM:
            res = (S, _select_columns(full, S, self.L))
        _cache_store(self._support_cache, rows, res)
        return res

    def _restricted_fwd(self, rows: torch.Tensor):
        """Forward counterpart of :meth:`_restricted`: A[rows, :L] and A[rows, halo] with
        the halo columns renumbered onto the contributing halo rows only, plus the
        forward sub-plan (owners send just those rows: the reverse of the backward
        sub-plan)."""
        hit = _cache_lookup(self._restrict_fwd_cache, rows)
        if hit is not None:
            return hit
        ir = self.interior.select_rows(rows)
        rs = self.inv_deg[rows.long()].contiguous()
        hsub = None
        if self.halo is not None:
            _, _, sub = self._restricted(rows)
            _, a2a_sub, _, nz, recv_local = sub
            hr = self.halo.select_rows(rows)
            pos = torch.full((self.H,), -1, dtype=torch.long, device=nz.device)
            pos[nz] = torch.arange(nz.numel(), device=nz.device)
            hr = CSR(hr.rowptr, pos[hr.col.long()].to(torch.int32).contiguous(),
                     max(int(nz.numel()), 1))
            hsub = (hr, a2a_sub.reversed(), recv_local.to(self.send_map.idx.dtype))
        hit = (ir, rs, hsub)
        _cache_store(self._restrict_fwd_cache, rows, hit)
        return hit

    def aggregate_rows(self, x: torch.Tensor, rows: torch.Tensor, mean: bool = True,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``aggregate(x)[rows]`` without aggregating the other rows: A[rows, :] x over the
        interior block, and over only the halo rows that neighbour ``rows`` (the owners
        send just those, overlapped with the interior SpMM). The first call for a row set
        is collective (sub-plan exchange, shared with :meth:`aggregate_T_rows`)."""
        ir, rs, hsub = self._restricted_fwd(rows)
        rsc = rs if mean else None
        self.edges_aggregated += ir.nnz + (hsub[0].nnz if hsub is not None else 0)
        if hsub is None:
            return K.spmm(ir.rowptr, ir.col, x, out, row_scale=rsc, split=_hs(ir))
        hr, a2a_f, recv_local = hsub
        recv, work = a2a_f(K.gather_rows(x, recv_local), async_op=True)
        if not self.overlap:
            work.wait()
        out = K.spmm(ir.rowptr, ir.col, x, out, row_scale=rsc, split=_hs(ir))
        work.wait()
        K.spmm(hr.rowptr, hr.col, recv, out, row_scale=rsc, beta=1.0, split=_hs(hr))
        return out

    def prepare_backward(self):
        """Build the cached transposes and hub-row splits eagerly (outside any timed
        region)."""
        csrs = [self.interior]
        if not self.interior.symmetric:
            csrs.append(self.interior.transpose())
        if self.halo is not None:
            csrs += [self.halo.compact_rows(), self.halo.transpose(),
                     self.send_map.transpose_csr().compact_rows()]
        for c in csrs:
            _hs(c)
        return self

    def memory_bytes(self) -> int:
        n = self.interior.memory_bytes()
        if self.halo is not None:
            n += self.halo.memory_bytes()
        return n


class _DistAggregateFn(Function):
    @staticmethod
    def forward(ctx, x, graph: DistGraph, mean: bool):
        ctx.graph, ctx.mean = graph, mean
        return graph.aggregate(x.contiguous(), mean)

    @staticmethod
    def backward(ctx, g):
        return ctx.graph.aggregate_T(g, ctx.mean), None, None


class _DistAggregateDropFn(Function):
    @staticmethod
    def forward(ctx, x, graph: DistGraph, mean: bool, drop: EdgeDrop):
        out, kept = graph.aggregate_drop(x, drop, mean)
        ctx.graph, ctx.mean, ctx.drop = graph, mean, drop
        ctx.save_for_backward(kept)
        return out

    @staticmethod
    def backward(ctx, g):
        (kept,) = ctx.saved_tensors
        return ctx.graph.aggregate_drop_T(g, ctx.drop, ctx.mean, kept), None, None, None


class _DistAggregateExtremeFn(Function):
    @staticmethod
    def forward(ctx, x, graph: DistGraph, minimum: bool):
        out, arg = graph.aggregate_extreme(x.contiguous(), minimum)
        ctx.graph = graph
        ctx.save_for_backward(arg)
        return out

    @staticmethod
    def backward(ctx, g):
        (arg,) = ctx.saved_tensors
        return ctx.graph.aggregate_extreme_T(g, arg), None, None


class _DistAggregateMultiFn(Function):
    @staticmethod
    def forward(ctx, x, graph: DistGraph, aggregators: tuple, eps: float):
        x = vec_rows(x)
        out, saved = graph.aggregate_multi(x, aggregators, eps)
        ctx.graph, ctx.aggregators = graph, aggregators
        # the moments that are blocks of ``out`` are saved with it, the others on their own
        ctx.save_for_backward(x, out, None if "mean" in aggregators else saved["mean"],
                              None if "std" in aggregators else saved["sdev"], saved["amax"],
                              saved["amin"], saved["halo"])
        return out

    @staticmethod
    def backward(ctx, g):
        x, out, mean, sdev, amax, amin, halo = ctx.saved_tensors
        blk = multi_blocks(out.detach(), ctx.aggregators, x.shape[1])
        saved = dict(mean=blk.get("mean", mean), sdev=blk.get("std", sdev), amax=amax,
                     amin=amin, halo=halo)
        return ctx.graph.aggregate_multi_T(g, x, saved, ctx.aggregators), None, None, None


def dist_aggregate_multi(x: torch.Tensor, graph: DistGraph,
                         aggregators=("mean", "max", "min", "std"),
                         eps: float = 1e-5) -> torch.Tensor:
    """Autograd-aware distributed :func:`~dgraph_amd.ops.aggregate.aggregate_multi`: the
    aggregations named in ``aggregators`` of every local vertex's in-neighbours, local and
    halo, as the column blocks of one ``[L, A*F]`` tensor (one exchange forward, one
    backward; :meth:`DistGraph.aggregate_multi`)."""
    return _DistAggregateMultiFn.apply(x, graph, check_aggregators(aggregators), float(eps))


class _DistSoftmaxAggregateFn(Function):
    @staticmethod
    def forward(ctx, x, t, graph: DistGraph):
        x = vec_rows(x)
        tv = K.temperature_rows(t, x, "dist_softmax_aggregate")
        out, saved = graph.aggregate_softmax(x, tv)
        ctx.graph = graph
        ctx.save_for_backward(x, t, out, saved["lse"], saved["halo"])
        return out

    @staticmethod
    def backward(ctx, g):
        x, t, out, lse, halo = ctx.saved_tensors
        tv = K.temperature_rows(t, x, "dist_softmax_aggregate")
        want_dt = ctx.needs_input_grad[1]
        dx, dt = ctx.graph.aggregate_softmax_T(g, x, tv, dict(out=out, lse=lse, halo=halo),
                                               want_dt=want_dt)
        if want_dt:
            dt = (dt.sum() if t.numel() == 1 else dt).reshape(t.shape).to(t.dtype)
        return dx, dt, None


def dist_softmax_aggregate(x: torch.Tensor, graph: DistGraph, t=1.0) -> torch.Tensor:
    """Autograd-aware distributed :func:`~dgraph_amd.ops.aggregate.softmax_aggregate` over
    every local vertex's in-neighbours, local and halo (one exchange forward, one backward;
    :meth:`DistGraph.aggregate_softmax`). ``t`` as there; its gradient is this rank's part
    (``t`` is a replicated parameter: all-reduce it with the other weight gradients)."""
    return _DistSoftmaxAggregateFn.apply(x, as_temperature(t, x), graph)


class _DistGatedAggregateFn(Function):
    @staticmethod
    def forward(ctx, k, qv, graph: DistGraph):
        k, qv = vec_rows(k), vec_rows(qv)
        out, saved = graph.aggregate_gated(k, qv)
        ctx.graph = graph
        ctx.save_for_backward(k, qv, saved["ds"], saved["halo"])
        return out

    @staticmethod
    def backward(ctx, g):
        k, qv, ds, halo = ctx.saved_tensors
        dk, dqv = ctx.graph.aggregate_gated_T(g, k, qv, dict(ds=ds, halo=halo))
        return dk, dqv, None


def dist_gated_aggregate(k: torch.Tensor, qv: torch.Tensor, graph: DistGraph) -> torch.Tensor:
    """Autograd-aware distributed :func:`~dgraph_amd.ops.aggregate.gated_aggregate` over
    every local vertex's in-neighbours, local and halo: ``out[i] = sum_j sigmoid(k[i] + q[j])
    v[j]`` per channel, with ``k`` ``[L, F]`` and ``qv`` the local ``[L, 2F]`` buffer ``[q |
    v]`` (one exchange of ``[q | v]`` rows forward, one of ``d[q | v]`` rows backward;
    :meth:`DistGraph.aggregate_gated`). Both may be column views of one projection."""
    if k.dim() != 2 or qv.dim() != 2 or qv.shape[1] != 2 * k.shape[1] or \
            k.shape[0] != qv.shape[0]:
        raise ValueError(f"dist_gated_aggregate: k [L, F] and qv [L, 2F] expected, got "
                         f"{tuple(k.shape)} and {tuple(qv.shape)}")
    return _DistGatedAggregateFn.apply(k, qv, graph)


class _DistSoftmaxAggregateEdgeFn(Function):
    @staticmethod
    def forward(ctx, x, e_int, e_halo, t, graph: DistGraph, relu: bool, eps: float):
        x = vec_rows(x)
        tv = K.temperature_rows(t, x, "dist_softmax_aggregate_edge")
        out, saved = graph.aggregate_softmax_edge(x, e_int, e_halo, tv, relu, eps)
        ctx.graph, ctx.relu, ctx.eps = graph, relu, eps
        ctx.save_for_backward(x, e_int, e_halo, t, out, saved["lse"], saved["halo"])
        return out

    @staticmethod
    def backward(ctx, g):
        x, e_int, e_halo, t, out, lse, halo = ctx.saved_tensors
        tv = K.temperature_rows(t, x, "dist_softmax_aggregate_edge")
        want_dt = ctx.needs_input_grad[3]
        dx, de_int, de_halo, dt = ctx.graph.aggregate_softmax_edge_T(
            g, x, e_int, e_halo, tv, dict(out=out, lse=lse, halo=halo), ctx.relu, ctx.eps,
            want_dt=want_dt)
        if want_dt:
            dt = (dt.sum() if t.numel() == 1 else dt).reshape(t.shape).to(t.dtype)
        return (dx, de_int, None if e_halo is None else de_halo.reshape(e_halo.shape), dt,
                None, None, None)


def dist_softmax_aggregate_edge(x: torch.Tensor, e_int: torch.Tensor,
                                e_halo: Optional[torch.Tensor], graph: DistGraph, t=1.0,
                                relu: bool = True, eps: float = 1e-7) -> torch.Tensor:
    """Autograd-aware distributed :func:`~dgraph_amd.ops.aggregate.softmax_aggregate_edge`:
    the softmax aggregation of the messages ``relu(x[j] + e_ij) + eps`` over every local
    vertex's in-neighbours, local and halo (one exchange of ``x`` rows forward, one backward;
    :meth:`DistGraph.aggregate_softmax_edge`). ``e_int`` / ``e_halo``: the edge rows of
    ``graph.interior`` / ``graph.halo`` in their slot order (``e_halo`` may be ``None`` when
    the halo block has no entry). Gradients reach ``x``, both edge blocks and ``t``, whose
    gradient is this rank's part, as :func:`dist_softmax_aggregate`'s."""
    return _DistSoftmaxAggregateEdgeFn.apply(x, e_int, e_halo, as_temperature(t, x), graph,
                                             bool(relu), float(eps))


class _DistEdgeDotFn(Function):
    @staticmethod
    def forward(ctx, a, b, graph: DistGraph, heads: int, scale: float):
        s_int, s_halo, saved = graph.edge_dot(a, b, heads, scale)
        ctx.graph, ctx.heads, ctx.scale, ctx.n_int = graph, heads, scale, s_int.shape[0]
        ctx.save_for_backward(a, b, saved["halo"])
        return torch.cat([s_int, s_halo]) if s_halo.shape[0] else s_int

    @staticmethod
    def backward(ctx, g):
        a, b, halo = ctx.saved_tensors
        n = ctx.n_int
        da, db = ctx.graph.edge_dot_T(g[:n], g[n:], a, b,
                                      dict(halo=halo, heads=ctx.heads, scale=ctx.scale))
        return da, db, None, None, None


def dist_edge_dot(a: torch.Tensor, b: torch.Tensor, graph: DistGraph, heads: int = 1,
                  scale: float = 1.0) -> torch.Tensor:
    """Autograd-aware distributed :func:`~dgraph_amd.ops.aggregate.edge_dot`: one score per
    head for every edge at this rank's vertices, ``scale * <a[i], b[j]>`` with ``b[j]`` local
    or a halo row (one exchange of whole rows forward, one backward;
    :meth:`DistGraph.edge_dot`). ``a``, ``b``: ``[L, F]``; ``a is b`` receives the sum of both
    gradients. Returns ``[graph.nnz, heads]``: the interior block's scores in
    ``graph.interior``'s slot order, then the halo block's in ``graph.halo``'s."""
    from ..ops.aggregate import check_edge_dot

    heads = int(heads)
    check_edge_dot(a, b, graph.L, graph.L, heads)
    if a is b:
        a = b = vec_rows(a)
    else:
        a, b = vec_rows(a), vec_rows(b)
    return _DistEdgeDotFn.apply(a, b, graph, heads, float(scale))


def dist_aggregate(x: torch.Tensor, graph: DistGraph, mean: bool = True,
                   reduce: Optional[str] = None,
                   drop: Optional[EdgeDrop] = None) -> torch.Tensor:
    """Autograd-aware distributed neighbourhood aggregation: sum or mean (``mean``), or
    with ``reduce="max"`` / ``"min"`` the elementwise extremum over the in-neighbours (its
    gradient goes to the one winning entry, :meth:`DistGraph.aggregate_extreme`), or with
    ``reduce="softmax"`` :func:`dist_softmax_aggregate` at temperature 1. ``drop``: the sum
    / mean runs over the random subgraph an :class:`~dgraph_amd.ops.aggregate.EdgeDrop`
    keeps (:meth:`DistGraph.aggregate_drop`; mean over the kept in-neighbours); ``None`` or
    ``p == 0`` is the plain call."""
    if drop is not None and drop.p > 0.0:
        if reduce is not None:
            raise ValueError(f"drop supports sum / mean only, got reduce={reduce!r}")
        return _DistAggregateDropFn.apply(x, graph, mean, drop)
    if reduce is None:
        return _DistAggregateFn.apply(x, graph, mean)
    if reduce == "softmax":
        return dist_softmax_aggregate(x, graph, 1.0)
    if reduce not in ("max", "min"):
        raise ValueError(f"unsupported reduce {reduce!r}")
    return _DistAggregateExtremeFn.apply(x, graph, reduce == "min")
