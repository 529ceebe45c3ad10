#!/usr/bin/env python3
"""Micro-benchmark of the max aggregation kernels (csrc/kernels/spmm_max.hip) next to the
sum SpMM at the same shape in the same run.

Four passes per (dtype, F) case on the default graph of benchmarks/bench_spmm.py, timed in
interleaved rounds with device events (one warm-up round, then ``--rounds`` timed ones):

    sum_fwd   K.spmm over the CSR                      (the yardstick, forward)
    max_fwd   K.segment_extreme over the CSR           (+ one int32 arg row per output row)
    sum_T     K.spmm over the transposed CSR           (the yardstick, backward)
    max_bwd   K.segment_extreme_bwd over the transpose (gathers g AND arg rows)

One JSON line per case: median / min / max ms, the bytes each pass has to move (computed
from the shapes below) over the median time, and the max : sum time ratios next to what
the byte counts alone predict.
Example: python benchmarks/bench_segment_max.py --rounds 7
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pass_bytes(nnz, rows, cols, F, esize, isize):
    """Bytes each pass must move: gathered rows + ids + output (+ arg / rel)."""
    return {
        "sum_fwd": nnz * (F * esize + isize) + rows * F * esize,
        "max_fwd": nnz * (F * esize + isize) + rows * F * (esize + 4),
        "sum_T": nnz * (F * esize + isize) + cols * F * esize,
        "max_bwd": nnz * (F * (esize + 4) + isize + 4) + cols * F * esize,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ogbn-products")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--feats", default="128,256")
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--global-frac", type=float, default=0.05)
    ap.add_argument("--window", type=int, default=1 << 14)
    a = ap.parse_args()
    from dgraph_amd import _native
    from dgraph_amd.data.synthetic import SHAPES, build_partition
    from dgraph_amd.ops import kernels as K

    if not torch.cuda.is_available():
        raise SystemExit("bench_segment_max.py needs a GPU")
    _native.ops()
    dev = torch.device("cuda", 0)
    shape = SHAPES[a.shape] if a.scale == 1.0 else SHAPES[a.shape].scaled(a.scale)
    p = build_partition(shape, 0, 1, dev, global_frac=a.global_frac, window=a.window)
    csr = p["csr"]
    t, rel = csr.transpose_rel()
    rows, cols, nnz = csr.num_rows, t.num_rows, csr.nnz
    print(f"[segment_max] rows={rows} nnz={nnz} max degree={int(csr.degree().max())}",
          flush=True)
    dts = {"fp32": torch.float32, "bf16": torch.bfloat16}
    for dname in a.dtypes.split(","):
        dt = dts[dname]
        for F in [int(f) for f in a.feats.split(",")]:
            x = torch.randn(cols, F, device=dev).to(dt)
            g = torch.randn(rows, F, device=dev).to(dt)
            out = torch.empty(rows, F, dtype=dt, device=dev)
            arg = torch.empty(rows, F, dtype=torch.int32, device=dev)
            gx = torch.empty(cols, F, dtype=dt, device=dev)
            passes = {
                "sum_fwd": lambda: K.spmm(csr.rowptr, csr.col, x, out),
                "max_fwd": lambda: K.segment_extreme(csr.rowptr, csr.col, x, out, arg),
                "sum_T": lambda: K.spmm(t.rowptr, t.col, g, gx),
                # arg is the one max_fwd left: the real winners of this x
                "max_bwd": lambda: K.segment_extreme_bwd(t.rowptr, t.col, rel, g, arg, gx),
            }
            times = {k: [] for k in passes}
            for r in range(a.rounds + 1):  # round 0 warms every pass up
                for k, fn in passes.items():
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    s.record()
                    fn()
                    e.record()
                    torch.cuda.synchronize()
                    if r > 0:
                        times[k].append(s.elapsed_time(e))
            nb = pass_bytes(nnz, rows, cols, F, x.element_size(), csr.col.element_size())
            rec = {"bench": "segment_max", "shape": shape.name, "rows": rows, "nnz": nnz,
                   "dtype": dname, "F": F, "rounds": a.rounds}
            med = {}
            for k, ts in times.items():
                med[k] = statistics.median(ts)
                rec[k] = {"ms": round(med[k], 3), "ms_min": round(min(ts), 3),
                          "ms_max": round(max(ts), 3), "bytes": nb[k],
                          "TBps": round(nb[k] / med[k] / 1e9, 3)}
            rec["fwd_ratio"] = round(med["max_fwd"] / med["sum_fwd"], 3)
            rec["fwd_ratio_from_bytes"] = round(nb["max_fwd"] / nb["sum_fwd"], 3)
            rec["bwd_ratio"] = round(med["max_bwd"] / med["sum_T"], 3)
            rec["bwd_ratio_from_bytes"] = round(nb["max_bwd"] / nb["sum_T"], 3)
            print(json.dumps(rec), flush=True)
            del x, g, out, arg, gx


if __name__ == "__main__":
    main()
