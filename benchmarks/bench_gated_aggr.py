#!/usr/bin/env python3
"""Micro-benchmark of the fused gated aggregation kernels (csrc/kernels/spmm_gated.hip) next
to the fp32 sum SpMM, the softmax aggregation and the composed torch path, at the same shape
in the same process.

Passes per F (fp32) on the default graph of benchmarks/bench_spmm.py, timed in interleaved
rounds with device events (one warm-up round, then ``--rounds`` timed ones); ``q`` and ``v``
are the halves of one ``[N, 2F]`` buffer, ``dq`` and ``dv`` of another, as the layer has them:

    gated_fwd     K.segment_gated: out in ONE gather of the q and v rows
    gated_fwd_ds  the same pass writing ds as well (what a training step runs)
    sum_fwd       K.spmm (the fp32 sum SpMM: the gather-bound yardstick, ONE row per entry)
    smx_fwd       K.segment_softmax: out and lse (one row per entry, one exp per element)
    gated_bwd     K.segment_gated_bwd_src: dq and dv over the transposed pattern
    sum_T         K.spmm over the transposed pattern

and, on the graph scaled by ``--composed-scale`` (the composed path holds three ``[E, F]``
tensors), the fused op against gather, add, sigmoid, multiply and ``scatter_sum`` through
autograd, forward and forward + backward:

    fused_fwd / fused_fwd_bwd        gated_aggregate
    composed_fwd / composed_fwd_bwd  the composition

One JSON line per case: median / min / max ms per pass, the bytes each pass must move and the
effective TB/s, ``fwd_vs_sum`` = gated_fwd over sum_fwd (2.0 from the bytes: two gathered
rows per entry), ``ds_over_fwd``, ``bwd_vs_sum_T`` and ``composed_over_fused``. Nothing is
asserted on any ratio.
Example: python benchmarks/bench_gated_aggr.py --rounds 7
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pass_bytes(nnz, rows, cols, F, isize):
    """Bytes each pass must move (fp32): gathered rows + ids + resident rows + outputs."""
    one = nnz * (4 * F + isize)
    two = nnz * (2 * 4 * F + isize)
    return {
        "gated_fwd": two + rows * F * 8,          # k read, out written
        "gated_fwd_ds": two + rows * F * 12,      # ... and ds written
        "sum_fwd": one + rows * F * 4,
        "smx_fwd": one + rows * F * 8 + F * 4,
        # per transposed entry: k and g rows and the id; q, v read, dq, dv written once
        "gated_bwd": two + cols * F * 16,
        "sum_T": one + cols * F * 4,
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
    from dgraph_amd.data.synthetic import SHAPES, build_partition
    from dgraph_amd.ops import kernels as K
    from dgraph_amd.ops.aggregate import gated_aggregate, gather, scatter_sum
    from dgraph_amd.ops.csr import IndexMap

    if not torch.cuda.is_available():
        raise SystemExit("bench_gated_aggr.py needs a GPU")
    dev = torch.device("cuda", 0)
    feats = [int(f) for f in a.feats.split(",")]
    shape = SHAPES[a.shape] if a.scale == 1.0 else SHAPES[a.shape].scaled(a.scale)
    p = build_partition(shape, 0, 1, dev, global_frac=a.global_frac, window=a.window)
    csr = p["csr"]
    t = csr.transpose()
    rows, cols, nnz = csr.num_rows, t.num_rows, csr.nnz
    print(f"[gated] rows={rows} nnz={nnz} max degree={int(csr.degree().max())}", flush=True)
    for F in feats:
        k = torch.randn(rows, F, device=dev)
        qv = torch.randn(cols, 2 * F, device=dev)
        q, v = qv[:, :F], qv[:, F:]
        x = torch.randn(cols, F, device=dev)
        tv = torch.linspace(0.5, 1.5, F, device=dev)
        g = torch.randn(rows, F, device=dev)
        out = torch.empty(rows, F, device=dev)
        ds = torch.empty(rows, F, device=dev)
        o2 = torch.empty(rows, F, device=dev)
        lse = torch.empty(rows, F, device=dev)
        dqv = torch.empty(cols, 2 * F, device=dev)
        dx = torch.empty(cols, F, device=dev)
        passes = {
            "gated_fwd": lambda: K.segment_gated(csr.rowptr, csr.col, k, q, v, out),
            "gated_fwd_ds": lambda: K.segment_gated(csr.rowptr, csr.col, k, q, v, out, ds),
            "sum_fwd": lambda: K.spmm(csr.rowptr, csr.col, x, o2),
            "smx_fwd": lambda: K.segment_softmax(csr.rowptr, csr.col, x, tv, o2, lse),
            "gated_bwd": lambda: K.segment_gated_bwd_src(t.rowptr, t.col, k, q, v, g,
                                                         dqv[:, :F], dqv[:, F:]),
            "sum_T": lambda: K.spmm(t.rowptr, t.col, g, dx),
        }
        times = timed(passes, a.rounds)
        nb = pass_bytes(nnz, rows, cols, F, csr.col.element_size())
        rec = {"bench": "gated_aggr", "shape": shape.name, "rows": rows, "nnz": nnz,
               "dtype": "fp32", "F": F, "rounds": a.rounds}
        med = {}
        for name, ts in times.items():
            med[name] = statistics.median(ts)
            rec[name] = {"ms": round(med[name], 3), "ms_min": round(min(ts), 3),
                         "ms_max": round(max(ts), 3), "bytes": nb[name],
                         "TBps": round(nb[name] / med[name] / 1e9, 3)}
        rec["fwd_vs_sum"] = round(med["gated_fwd"] / med["sum_fwd"], 3)
        rec["fwd_vs_sum_from_bytes"] = round(nb["gated_fwd"] / nb["sum_fwd"], 3)
        rec["fwd_vs_smx"] = round(med["gated_fwd"] / med["smx_fwd"], 3)
        rec["ds_over_fwd"] = round(med["gated_fwd_ds"] / med["gated_fwd"], 3)
        rec["bwd_vs_sum_T"] = round(med["gated_bwd"] / med["sum_T"], 3)
        rec["bwd_vs_sum_T_from_bytes"] = round(nb["gated_bwd"] / nb["sum_T"], 3)
        print(json.dumps(rec), flush=True)
        del k, qv, q, v, x, g, out, ds, o2, lse, dqv, dx
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
        k = torch.randn(csr.num_rows, F, device=dev, requires_grad=True)
        qv = torch.randn(csr.num_cols, 2 * F, device=dev, requires_grad=True)
        g = torch.randn(csr.num_rows, F, device=dev)

        def fused():
            return gated_aggregate(k, qv[:, :F], qv[:, F:], csr)

        def composed():
            qe = gather(qv[:, :F].contiguous(), src)    # [E, F]
            ve = gather(qv[:, F:].contiguous(), src)    # [E, F]
            ke = gather(k, dst)                         # [E, F]
            return scatter_sum(torch.sigmoid(ke + qe) * ve, dst)

        def both(fn):
            k.grad = qv.grad = None
            fn().backward(g)

        passes = {
            "fused_fwd": fused,
            "composed_fwd": composed,
            "fused_fwd_bwd": lambda: both(fused),
            "composed_fwd_bwd": lambda: both(composed),
        }
        with torch.no_grad():
            diff = float((composed() - fused()).abs().max())
        times = timed(passes, a.rounds)
        rec = {"bench": "gated_aggr_composed", "shape": small.name, "rows": csr.num_rows,
               "nnz": csr.nnz, "dtype": "fp32", "F": F, "rounds": a.rounds,
               "max_abs_diff": diff, "edge_tensor_bytes": csr.nnz * F * 4}
        med = {name: statistics.median(ts) for name, ts in times.items()}
        for name, ts in times.items():
            rec[name] = {"ms": round(med[name], 3), "ms_min": round(min(ts), 3),
                         "ms_max": round(max(ts), 3)}
        rec["composed_over_fused_fwd"] = round(med["composed_fwd"] / med["fused_fwd"], 2)
        rec["composed_over_fused_fwd_bwd"] = round(med["composed_fwd_bwd"] /
                                                   med["fused_fwd_bwd"], 2)
        print(json.dumps(rec), flush=True)
        del k, qv, g


if __name__ == "__main__":
    main()
