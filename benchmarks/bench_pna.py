#!/usr/bin/env python3
"""Micro-benchmark of the fused PNA statistics kernels (csrc/kernels/spmm_pna.hip) next to
the separate passes they replace, at the same shape in the same process.

Passes per F (fp32) on the default graph of benchmarks/bench_spmm.py, timed in interleaved
rounds with device events (one warm-up round, then ``--rounds`` timed ones):

    pna_fwd    K.segment_pna: mean, sdev, max, min (+ two int32 arg rows) in ONE gather
    mean_fwd   K.spmm with the 1/deg row scale                     \\
    max_fwd    K.segment_extreme                                    | the separate forward:
    min_fwd    K.segment_extreme(minimum=True)                      | four gathers of x[col]
    sq_fwd     K.spmm over x*x (the E[x^2] of the naive variance)  /
    pna_bwd    K.segment_pna_bwd with all four gradients over the transposed pattern
    mean_T     K.spmm over the transposed pattern                  \\  the separate backward
    max_bwd    K.segment_extreme_bwd                                | (no std term: the
    min_bwd    K.segment_extreme_bwd                               /   library had none)

One JSON line per case: median / min / max ms per pass, ``fwd_ratio`` = pna_fwd over the sum
of the four separate forward passes, ``fwd_vs_mean_plus_max`` = pna_fwd over mean_fwd +
max_fwd (two of the four passes it replaces: above 1 is a defect), ``bwd_ratio`` likewise,
and the ratio the byte counts alone predict.
Example: python benchmarks/bench_pna.py --rounds 7
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pass_bytes(nnz, rows, cols, F, isize):
    """Bytes each pass must move (fp32): gathered rows + ids + outputs (+ arg / rel)."""
    gat = nnz * (4 * F + isize)
    return {
        "pna_fwd": gat + rows * F * 4 * 6,
        "mean_fwd": gat + rows * F * 4,
        "max_fwd": gat + rows * F * 8,
        "min_fwd": gat + rows * F * 8,
        "sq_fwd": gat + rows * F * 4,
        # per transposed entry: four gradient rows, mean, sdev, two arg rows, id, rel, 1/deg
        "pna_bwd": nnz * (8 * 4 * F + isize + 8) + cols * F * 8,
        "mean_T": gat + cols * F * 4,
        "max_bwd": nnz * (8 * F + isize + 4) + cols * F * 4,
        "min_bwd": nnz * (8 * F + isize + 4) + cols * F * 4,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ogbn-products")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--feats", default="128,256")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--global-frac", type=float, default=0.05)
    ap.add_argument("--window", type=int, default=1 << 14)
    a = ap.parse_args()
    from dgraph_amd import _native
    from dgraph_amd.data.synthetic import SHAPES, build_partition
    from dgraph_amd.ops import kernels as K

    if not torch.cuda.is_available():
        raise SystemExit("bench_pna.py needs a GPU")
    _native.ops()
    dev = torch.device("cuda", 0)
    shape = SHAPES[a.shape] if a.scale == 1.0 else SHAPES[a.shape].scaled(a.scale)
    p = build_partition(shape, 0, 1, dev, global_frac=a.global_frac, window=a.window)
    csr = p["csr"]
    t, rel = csr.transpose_rel()
    rows, cols, nnz = csr.num_rows, t.num_rows, csr.nnz
    inv = csr.inv_degree()
    print(f"[pna] rows={rows} nnz={nnz} max degree={int(csr.degree().max())}", flush=True)
    for F in [int(f) for f in a.feats.split(",")]:
        x = torch.randn(cols, F, device=dev)
        xx = x * x
        g = torch.randn(rows, 4 * F, device=dev)
        gm, gx_, gn, gs = (g[:, i * F:(i + 1) * F] for i in range(4))
        gc = gm.contiguous()
        agg = torch.empty(rows, 4 * F, device=dev)  # [mean | max | min | std] blocks
        mean, vmax, vmin, sdev = (agg[:, i * F:(i + 1) * F] for i in range(4))
        amax = torch.empty(rows, F, dtype=torch.int32, device=dev)
        amin = torch.empty(rows, F, dtype=torch.int32, device=dev)
        out = torch.empty(rows, F, device=dev)
        arg = torch.empty(rows, F, dtype=torch.int32, device=dev)
        dx = torch.empty(cols, F, device=dev)
        passes = {
            "pna_fwd": lambda: K.segment_pna(csr.rowptr, csr.col, x, mean=mean, sdev=sdev,
                                             vmax=vmax, amax=amax, vmin=vmin, amin=amin),
            "mean_fwd": lambda: K.spmm(csr.rowptr, csr.col, x, out, row_scale=inv),
            "max_fwd": lambda: K.segment_extreme(csr.rowptr, csr.col, x, out, arg),
            "min_fwd": lambda: K.segment_extreme(csr.rowptr, csr.col, x, out, arg,
                                                 minimum=True),
            "sq_fwd": lambda: K.spmm(csr.rowptr, csr.col, xx, out, row_scale=inv),
            # mean / sdev / amax / amin are the ones pna_fwd left: the real ones of this x
            "pna_bwd": lambda: K.segment_pna_bwd(t.rowptr, t.col, rel, x, inv, dx, g_mean=gm,
                                                 g_std=gs, mean=mean, sdev=sdev, g_max=gx_,
                                                 amax=amax, g_min=gn, amin=amin),
            "mean_T": lambda: K.spmm(t.rowptr, t.col, gc, dx, col_scale=inv),
            "max_bwd": lambda: K.segment_extreme_bwd(t.rowptr, t.col, rel, gc, amax, dx),
            "min_bwd": lambda: K.segment_extreme_bwd(t.rowptr, t.col, rel, gc, amin, dx),
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
        nb = pass_bytes(nnz, rows, cols, F, csr.col.element_size())
        rec = {"bench": "pna", "shape": shape.name, "rows": rows, "nnz": nnz, "dtype": "fp32",
               "F": F, "rounds": a.rounds}
        med = {}
        for k, ts in times.items():
            med[k] = statistics.median(ts)
            rec[k] = {"ms": round(med[k], 3), "ms_min": round(min(ts), 3),
                      "ms_max": round(max(ts), 3), "bytes": nb[k],
                      "TBps": round(nb[k] / med[k] / 1e9, 3)}
        fwd = ("mean_fwd", "max_fwd", "min_fwd", "sq_fwd")
        bwd = ("mean_T", "max_bwd", "min_bwd")
        rec["fwd_ratio"] = round(med["pna_fwd"] / sum(med[k] for k in fwd), 3)
        rec["fwd_ratio_from_bytes"] = round(nb["pna_fwd"] / sum(nb[k] for k in fwd), 3)
        rec["fwd_vs_mean_plus_max"] = round(med["pna_fwd"] / (med["mean_fwd"] + med["max_fwd"]),
                                            3)
        rec["bwd_ratio"] = round(med["pna_bwd"] / sum(med[k] for k in bwd), 3)
        rec["bwd_ratio_from_bytes"] = round(nb["pna_bwd"] / sum(nb[k] for k in bwd), 3)
        print(json.dumps(rec), flush=True)
        del x, xx, g, gc, agg, amax, amin, out, arg, dx


if __name__ == "__main__":
    main()
