#!/usr/bin/env python3
"""Micro-benchmark of the softmax aggregation kernels with edge features
(csrc/kernels/spmm_softmax_edge.hip) next to the plain softmax kernels and to the composed
path, at the same shape in the same process.

Passes per F (fp32), timed in interleaved rounds with device events (one warm-up round, then
``--rounds`` timed ones; median, min and max are reported):

    edge_fwd   K.segment_softmax_edge: message, out and lse in ONE pass (x gathered, e streamed)
    smx_fwd    K.segment_softmax on the same pattern (the gather-only yardstick)
    edge_bwd   K.segment_softmax_edge_bwd: every de row and the dt partial rows
    edge_dx    K.spmm over the slot-transposed pattern with de as the source matrix (dx)
    smx_bwd    K.segment_softmax_bwd over the transposed pattern (dx and dt, nothing per edge)

on the ogbn-products-shaped graph of benchmarks/bench_spmm.py at every ``--feats`` width and
on an ogbn-proteins-shaped graph (132,534 vertices, 79.1 M entries: the dataset whose only
features are edge features) at ``--proteins-feats``. ``e`` and ``de`` are ``4 nnz F``
bytes each; a width at which the two exceed ``--edge-gb`` runs on the graph scaled down to
fit (the record says so in ``scale``).

Then, per shape and width on the graph scaled so that one ``[E, F]`` tensor is at most
``--composed-gb`` (the composed path holds several, more under autograd), the fused op against
``gather`` + add + relu + ``edge_softmax(heads = F)`` (in 64-column blocks above F = 64) +
product + ``scatter_sum`` through autograd, forward and forward + backward:

    fused_fwd / fused_fwd_bwd        softmax_aggregate_edge
    composed_fwd / composed_fwd_bwd  the composition

One JSON line per case: median / min / max ms per pass, the bytes each pass must move and the
effective TB/s, ``edge_over_plain_fwd`` / ``_bwd`` (edge_bwd + edge_dx over smx_bwd) and
``composed_over_fused``.
Example: python benchmarks/bench_softmax_aggr_edge.py --rounds 5
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pass_bytes(nnz, rows, cols, F, isize, parts, tparts):
    """Bytes each pass must move (fp32): gathered / streamed rows + ids + outputs."""
    return {
        # per slot: the x row, the e row and the id; out and lse written once
        "edge_fwd": nnz * (8 * F + isize) + rows * F * 8 + F * 4,
        "smx_fwd": nnz * (4 * F + isize) + rows * F * 8 + F * 4,
        # per slot: x, e read and de written, the id; g, out, lse read once per row
        "edge_bwd": nnz * (12 * F + isize) + rows * F * 12 + parts * F * 4,
        # per slot: one de row and its int64 slot id; dx written once
        "edge_dx": nnz * (4 * F + 8) + cols * F * 4,
        "smx_bwd": nnz * (12 * F + isize) + cols * F * 8 + tparts * F * 4,
    }


def timed(passes, rounds):
    times = {k: [] for k in passes}
    for r in range(rounds + 1):  # round 0 warms every pass up
        for k, fn in passes.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            if r > 0:
                times[k].append(s.elapsed_time(e))
    return times


def stats(ts):
    return {"ms": round(statistics.median(ts), 3), "ms_min": round(min(ts), 3),
            "ms_max": round(max(ts), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--feats", default="64,128,256", help="widths on the products shape")
    ap.add_argument("--proteins-feats", default="64", help="widths on the proteins shape")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--global-frac", type=float, default=0.05)
    ap.add_argument("--window", type=int, default=1 << 14)
    ap.add_argument("--edge-gb", type=float, default=256.0,
                    help="largest e + de (GB) the kernel passes may allocate")
    ap.add_argument("--composed-gb", type=float, default=2.0,
                    help="largest [E, F] tensor (GB) of the composed comparison (0: skip it)")
    a = ap.parse_args()
    from dgraph_amd import _native
    from dgraph_amd.data.synthetic import SHAPES, build_partition
    from dgraph_amd.ops import kernels as K
    from dgraph_amd.ops.aggregate import (EDGE_SUM_HUB_CAP, _slot_transpose, edge_softmax,
                                          gather, scatter_sum, softmax_aggregate_edge)
    from dgraph_amd.ops.csr import IndexMap

    if not torch.cuda.is_available():
        raise SystemExit("bench_softmax_aggr_edge.py needs a GPU")
    ops = _native.ops()
    dev = torch.device("cuda", 0)
    proteins = dataclasses.replace(SHAPES["ogbn-products"], name="ogbn-proteins-shaped",
                                   num_nodes=132_534, num_directed_edges=39_561_252)
    plans = [(SHAPES["ogbn-products"], [int(f) for f in a.feats.split(",") if f]),
             (proteins, [int(f) for f in a.proteins_feats.split(",") if f])]

    def build(shape, scale):
        s = shape if scale >= 1.0 else shape.scaled(scale)
        if scale < 1.0:
            s = dataclasses.replace(s, name=f"{shape.name} x {scale:.3g}")
        return s, build_partition(s, 0, 1, dev, global_frac=a.global_frac,
                                  window=a.window)["csr"]

    def kernels(shape, scale, Fs):
        s, csr = build(shape, scale)
        t = csr.transpose()
        tt = _slot_transpose(csr)
        split = tt.hub_split(EDGE_SUM_HUB_CAP)
        rows, cols, nnz = csr.num_rows, t.num_rows, csr.nnz
        parts = ops.segment_softmax_edge_dt_parts(rows)
        tparts = ops.segment_softmax_dt_parts(cols)
        print(f"[softmax edge] {s.name}: rows={rows} nnz={nnz} max in-degree="
              f"{int(csr.degree().max())} max out-degree={int(tt.degree().max())}", flush=True)
        for F in Fs:
            x = torch.randn(cols, F, device=dev)
            e = torch.randn(nnz, F, device=dev)
            de = torch.empty(nnz, F, device=dev)
            tv = torch.linspace(0.5, 1.5, F, device=dev)
            g = torch.randn(rows, F, device=dev)
            out, lse, o2, l2 = (torch.empty(rows, F, device=dev) for _ in range(4))
            dx = torch.empty(cols, F, device=dev)
            dtp = torch.empty(parts, F, device=dev)
            dtp2 = torch.empty(tparts, F, device=dev)
            passes = {
                "edge_fwd": lambda: K.segment_softmax_edge(csr.rowptr, csr.col, x, e, tv, out,
                                                           lse),
                "smx_fwd": lambda: K.segment_softmax(csr.rowptr, csr.col, x, tv, o2, l2),
                # (out, lse) / (o2, l2) are the ones the forwards left: the real ones
                "edge_bwd": lambda: K.segment_softmax_edge_bwd(csr.rowptr, csr.col, x, e, tv, g,
                                                               out, lse, de, dt_partials=dtp),
                "edge_dx": lambda: K.spmm(tt.rowptr, tt.perm, de, dx, split=split),
                "smx_bwd": lambda: K.segment_softmax_bwd(t.rowptr, t.col, x, tv, g, o2, l2, dx,
                                                         dt_partials=dtp2),
            }
            times = timed(passes, a.rounds)
            nb = pass_bytes(nnz, rows, cols, F, csr.col.element_size(), parts, tparts)
            rec = {"bench": "softmax_aggr_edge", "shape": s.name, "scale": scale, "rows": rows,
                   "nnz": nnz, "dtype": "fp32", "F": F, "rounds": a.rounds,
                   "edge_stream_bytes": 4 * nnz * F}
            med = {}
            for k, ts in times.items():
                med[k] = statistics.median(ts)
                rec[k] = dict(stats(ts), bytes=nb[k], TBps=round(nb[k] / med[k] / 1e9, 3))
            rec["edge_over_plain_fwd"] = round(med["edge_fwd"] / med["smx_fwd"], 3)
            rec["edge_over_plain_fwd_from_bytes"] = round(nb["edge_fwd"] / nb["smx_fwd"], 3)
            rec["edge_over_plain_bwd"] = round((med["edge_bwd"] + med["edge_dx"]) /
                                               med["smx_bwd"], 3)
            rec["edge_over_plain_bwd_from_bytes"] = round((nb["edge_bwd"] + nb["edge_dx"]) /
                                                          nb["smx_bwd"], 3)
            print(json.dumps(rec), flush=True)
            del x, e, de, g, out, lse, o2, l2, dx, dtp, dtp2, passes
            torch.cuda.empty_cache()

    def composed_case(shape, scale, F):
        s, csr = build(shape, scale)
        src = IndexMap(csr.col, csr.num_cols)
        dst = IndexMap(csr.row_ids(), csr.num_rows)
        x = torch.randn(csr.num_cols, F, device=dev, requires_grad=True)
        e = torch.randn(csr.nnz, F, device=dev, requires_grad=True)
        tv = torch.linspace(0.5, 1.5, F, device=dev, requires_grad=True)
        g = torch.randn(csr.num_rows, F, device=dev)

        def composed():
            m = torch.relu(gather(x, src) + e) + 1e-7  # [E, F]
            sc = m * tv
            # edge_softmax takes at most 64 heads: wider F goes in 64-column blocks
            alpha = torch.cat([edge_softmax(sc[:, c:c + 64].contiguous(), csr)
                               for c in range(0, F, 64)], 1) if F > 64 else \
                edge_softmax(sc, csr)                   # [E, F], heads = F
            return scatter_sum(alpha * m, dst)

        def fused():
            return softmax_aggregate_edge(x, e, csr, tv)

        def both(fn):
            x.grad = e.grad = tv.grad = None
            fn().backward(g)

        passes = {"fused_fwd": fused, "composed_fwd": composed,
                  "fused_fwd_bwd": lambda: both(fused),
                  "composed_fwd_bwd": lambda: both(composed)}
        with torch.no_grad():
            diff = float((composed() - fused()).abs().max())
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        peak = {}
        for k in ("fused_fwd_bwd", "composed_fwd_bwd"):
            torch.cuda.reset_peak_memory_stats()
            passes[k]()
            torch.cuda.synchronize()
            peak[k] = torch.cuda.max_memory_allocated() - base
        times = timed(passes, a.rounds)
        rec = {"bench": "softmax_aggr_edge_composed", "shape": s.name, "scale": scale,
               "rows": csr.num_rows, "nnz": csr.nnz, "dtype": "fp32", "F": F,
               "rounds": a.rounds, "max_abs_diff": diff, "edge_tensor_bytes": csr.nnz * F * 4,
               "peak_extra_bytes": peak}
        med = {k: statistics.median(ts) for k, ts in times.items()}
        for k, ts in times.items():
            rec[k] = stats(ts)
        rec["composed_over_fused_fwd"] = round(med["composed_fwd"] / med["fused_fwd"], 2)
        rec["composed_over_fused_fwd_bwd"] = round(med["composed_fwd_bwd"] /
                                                   med["fused_fwd_bwd"], 2)
        print(json.dumps(rec), flush=True)

    for shape, Fs in plans:
        # the widths whose e + de fit run on the full graph, built once; the others scaled
        by_scale = {}
        for F in Fs:
            need = 2 * 4 * 2 * shape.num_directed_edges * F / 1e9  # symmetrised: 2 E slots
            scale = 1.0 if need <= a.edge_gb else round(a.edge_gb / need, 3)
            by_scale.setdefault(scale, []).append(F)
        for scale, group in sorted(by_scale.items(), reverse=True):
            kernels(shape, scale, group)
            torch.cuda.empty_cache()
    if a.composed_gb <= 0:
        return
    for shape, Fs in plans:
        for F in Fs:
            one = 4 * 2 * shape.num_directed_edges * F / 1e9
            composed_case(shape, min(1.0, round(a.composed_gb / one, 4)), F)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
