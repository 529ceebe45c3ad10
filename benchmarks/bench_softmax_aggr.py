#!/usr/bin/env python3
"""Micro-benchmark of the fused softmax aggregation kernels (csrc/kernels/spmm_softmax.hip)
next to the other neighbourhood reductions and to the composed path, at the same shape in
the same process.

Passes per F (fp32) on the default graph of benchmarks/bench_spmm.py, timed in interleaved
rounds with device events (one warm-up round, then ``--rounds`` timed ones):

    smx_fwd    K.segment_softmax: out and lse in ONE gather (one v_exp_f32 per element)
    sum_fwd    K.spmm (the fp32 sum SpMM: the gather-bound yardstick)
    max_fwd    K.segment_extreme
    pna_fwd    K.segment_pna: mean, sdev, max, min
    smx_bwd    K.segment_softmax_bwd: dx and the dt partial rows over the transposed pattern
    sum_T      K.spmm over the transposed pattern

and, on the graph scaled by ``--composed-scale`` (the composed path holds four ``[E, F]``
tensors), the fused op against ``gather`` + ``edge_softmax(heads = F)`` (in 64-column blocks
above F = 64, the kernel's head limit) + product + ``scatter_sum`` through autograd, forward
and forward + backward:

    fused_fwd / fused_fwd_bwd        softmax_aggregate
    composed_fwd / composed_fwd_bwd  the four-op composition

One JSON line per case: median / min / max ms per pass, the bytes each pass must move and
the effective TB/s, ``fwd_vs_sum`` = smx_fwd over sum_fwd (1.0: still gather-bound),
``bwd_vs_sum_T`` likewise, and ``composed_over_fused``.
Example: python benchmarks/bench_softmax_aggr.py --rounds 7
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pass_bytes(nnz, rows, cols, F, isize, parts):
    """Bytes each pass must move (fp32): gathered rows + ids + outputs."""
    gat = nnz * (4 * F + isize)
    return {
        "smx_fwd": gat + rows * F * 8 + F * 4,
        "sum_fwd": gat + rows * F * 4,
        "max_fwd": gat + rows * F * 8,
        "pna_fwd": gat + rows * F * 4 * 6,
        # per transposed entry: g, lse and out rows and the id; x read, dx written once
        "smx_bwd": nnz * (3 * 4 * F + isize) + cols * F * 8 + parts * F * 4,
        "sum_T": gat + cols * F * 4,
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ogbn-products")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--feats", default="64,128,256")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--global-frac", type=float, default=0.05)
    ap.add_argument("--window", type=int, default=1 << 14)
    ap.add_argument("--composed-scale", type=float, default=0.05,
                    help="graph scale of the composed-path comparison (0: skip it)")
    a = ap.parse_args()
    from dgraph_amd import _native
    from dgraph_amd.data.synthetic import SHAPES, build_partition
    from dgraph_amd.ops import kernels as K
    from dgraph_amd.ops.aggregate import edge_softmax, gather, scatter_sum, softmax_aggregate
    from dgraph_amd.ops.csr import IndexMap

    if not torch.cuda.is_available():
        raise SystemExit("bench_softmax_aggr.py needs a GPU")
    ops = _native.ops()
    dev = torch.device("cuda", 0)
    feats = [int(f) for f in a.feats.split(",")]
    shape = SHAPES[a.shape] if a.scale == 1.0 else SHAPES[a.shape].scaled(a.scale)
    p = build_partition(shape, 0, 1, dev, global_frac=a.global_frac, window=a.window)
    csr = p["csr"]
    t = csr.transpose()
    rows, cols, nnz = csr.num_rows, t.num_rows, csr.nnz
    parts = ops.segment_softmax_dt_parts(cols)
    print(f"[softmax] rows={rows} nnz={nnz} max degree={int(csr.degree().max())}", flush=True)
    for F in feats:
        x = torch.randn(cols, F, device=dev)
        tv = torch.linspace(0.5, 1.5, F, device=dev)
        g = torch.randn(rows, F, device=dev)
        out = torch.empty(rows, F, device=dev)
        lse = torch.empty(rows, F, device=dev)
        o2 = torch.empty(rows, F, device=dev)
        arg = torch.empty(rows, F, dtype=torch.int32, device=dev)
        agg = torch.empty(rows, 4 * F, device=dev)
        mean, vmax, vmin, sdev = (agg[:, i * F:(i + 1) * F] for i in range(4))
        amax = torch.empty(rows, F, dtype=torch.int32, device=dev)
        amin = torch.empty(rows, F, dtype=torch.int32, device=dev)
        dx = torch.empty(cols, F, device=dev)
        dtp = torch.empty(parts, F, device=dev)
        passes = {
            "smx_fwd": lambda: K.segment_softmax(csr.rowptr, csr.col, x, tv, out, lse),
            "sum_fwd": lambda: K.spmm(csr.rowptr, csr.col, x, o2),
            "max_fwd": lambda: K.segment_extreme(csr.rowptr, csr.col, x, o2, arg),
            "pna_fwd": lambda: K.segment_pna(csr.rowptr, csr.col, x, mean=mean, sdev=sdev,
                                             vmax=vmax, amax=amax, vmin=vmin, amin=amin),
            # out / lse are the ones smx_fwd left: the real ones of this x
            "smx_bwd": lambda: K.segment_softmax_bwd(t.rowptr, t.col, x, tv, g, out, lse, dx,
                                                     dt_partials=dtp),
            "sum_T": lambda: K.spmm(t.rowptr, t.col, g, dx),
        }
        times = timed(passes, a.rounds)
        nb = pass_bytes(nnz, rows, cols, F, csr.col.element_size(), parts)
        rec = {"bench": "softmax_aggr", "shape": shape.name, "rows": rows, "nnz": nnz,
               "dtype": "fp32", "F": F, "rounds": a.rounds, "dt_parts": parts}
        med = {}
        for k, ts in times.items():
            med[k] = statistics.median(ts)
            rec[k] = {"ms": round(med[k], 3), "ms_min": round(min(ts), 3),
                      "ms_max": round(max(ts), 3), "bytes": nb[k],
                      "TBps": round(nb[k] / med[k] / 1e9, 3)}
        rec["fwd_vs_sum"] = round(med["smx_fwd"] / med["sum_fwd"], 3)
        rec["fwd_vs_pna"] = round(med["smx_fwd"] / med["pna_fwd"], 3)
        rec["bwd_vs_sum_T"] = round(med["smx_bwd"] / med["sum_T"], 3)
        rec["bwd_vs_sum_T_from_bytes"] = round(nb["smx_bwd"] / nb["sum_T"], 3)
        print(json.dumps(rec), flush=True)
        del x, g, out, lse, o2, arg, agg, amax, amin, dx, dtp
    if a.composed_scale <= 0:
        return
    del csr, t, p
    torch.cuda.empty_cache()
    small = SHAPES[a.shape].scaled(a.composed_scale)
    p = build_partition(small, 0, 1, dev, global_frac=a.global_frac, window=a.window)
    csr = p["csr"]
    src = IndexMap(csr.col, csr.num_cols)
    dst = IndexMap(csr.row_ids(), csr.num_rows)
    for F in feats:
        x = torch.randn(csr.num_cols, F, device=dev, requires_grad=True)
        tv = torch.linspace(0.5, 1.5, F, device=dev, requires_grad=True)
        g = torch.randn(csr.num_rows, F, device=dev)

        def composed():
            xe = gather(x, src)                    # [E, F]
            sc = xe * tv
            # edge_softmax takes at most 64 heads: wider F goes in 64-column blocks
            alpha = torch.cat([edge_softmax(sc[:, c:c + 64].contiguous(), csr)
                               for c in range(0, F, 64)], 1) if F > 64 else \
                edge_softmax(sc, csr)              # [E, F], heads = F
            return scatter_sum(alpha * xe, dst)

        def both(fn):
            x.grad = tv.grad = None
            fn().backward(g)

        passes = {
            "fused_fwd": lambda: softmax_aggregate(x, csr, tv),
            "composed_fwd": composed,
            "fused_fwd_bwd": lambda: both(lambda: softmax_aggregate(x, csr, tv)),
            "composed_fwd_bwd": lambda: both(composed),
        }
        with torch.no_grad():
            diff = float((composed() - softmax_aggregate(x, csr, tv)).abs().max())
        times = timed(passes, a.rounds)
        rec = {"bench": "softmax_aggr_composed", "shape": small.name, "rows": csr.num_rows,
               "nnz": csr.nnz, "dtype": "fp32", "F": F, "rounds": a.rounds,
               "max_abs_diff": diff, "edge_tensor_bytes": csr.nnz * F * 4}
        med = {k: statistics.median(ts) for k, ts in times.items()}
        for k, ts in times.items():
            rec[k] = {"ms": round(med[k], 3), "ms_min": round(min(ts), 3),
                      "ms_max": round(max(ts), 3)}
        rec["composed_over_fused_fwd"] = round(med["composed_fwd"] / med["fused_fwd"], 2)
        rec["composed_over_fused_fwd_bwd"] = round(med["composed_fwd_bwd"] /
                                                   med["fused_fwd_bwd"], 2)
        print(json.dumps(rec), flush=True)
        del x, tv, g


if __name__ == "__main__":
    main()
