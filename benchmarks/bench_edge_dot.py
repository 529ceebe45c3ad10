#!/usr/bin/env python3
"""Micro-benchmark of the per-edge dot product kernel (csrc/kernels/sddmm.hip) next to the
fp32 sum SpMM on the same CSR, to the composed torch expression, and inside ``aggregate``'s
backward with edge weights that require grad.

Graphs: the ogbn-products-shaped synthetic CSR (``--shape`` / ``--scale``) and a power-law one
(``--powerlaw-rows`` rows, Zipf degrees with one hub of ``rows / 8`` entries), so that a
row-parallel kernel and a slot-parallel one can be told apart. Passes per graph, F and heads
(fp32), timed in interleaved rounds with device events (one warm-up round, then ``--rounds``):

    sddmm      K.edge_dot: s[k, h] = <a[r(k)], b[col[k]]> per head
    sum_fwd    K.spmm (the fp32 sum SpMM: both kernels gather the same rows once)

One JSON line per case: median / min / max ms per pass, the bytes each pass must move,
``sddmm_vs_sum`` = the measured ratio, ``from_bytes`` = sddmm bytes / sum bytes, and
``vs_target`` = measured ratio / (1.25 * from_bytes): at most 1 when the kernel is within the
margin of the gather-bound yardstick.

``--composed-scale``: on the graph at that scale (the composed path holds two [nnz, F]
tensors), ``K.edge_dot`` against ``(a[rows] * b[col]).view(nnz, H, D).sum(-1)``.

``--backward``: forward + backward of ``aggregate(x, csr, edge_weight=w, heads=H)`` with ``w``
requiring grad, its time and ``torch.cuda.max_memory_allocated`` across the backward. This
part uses nothing that this kernel added, so the same file run in a checkout of an earlier
commit (``--backward-only``) gives the "before" figures.
Example: python benchmarks/bench_edge_dot.py --rounds 7
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pass_bytes(nnz, rows, F, heads, isize):
    """Bytes each pass must move (fp32): gathered rows + ids, the rows' own side, outputs."""
    gat = nnz * (4 * F + isize) + (rows + 1) * 8
    return {"sddmm": gat + rows * F * 4 + nnz * heads * 4, "sum_fwd": gat + rows * F * 4}


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


def powerlaw_csr(rows, dev, seed=0):
    """Zipf-like degrees (mean about 8) over ``rows`` rows and columns, one hub row of
    ``rows / 8`` entries, uniform columns."""
    from dgraph_amd.ops.csr import CSR

    g = torch.Generator().manual_seed(seed)
    u = torch.rand(rows, generator=g)
    deg = (2.0 / u.clamp(min=1e-4) ** 0.75).long().clamp(max=rows // 16)
    deg[rows // 2] = rows // 8
    rowptr = torch.zeros(rows + 1, dtype=torch.long)
    torch.cumsum(deg, 0, out=rowptr[1:])
    col = torch.randint(0, rows, (int(rowptr[-1]),), generator=g, dtype=torch.int32)
    return CSR(rowptr.to(dev), col.to(dev), rows)


def kernel_cases(name, csr, feats, heads_list, rounds, dev):
    from dgraph_amd.ops import kernels as K

    rows, nnz = csr.num_rows, csr.nnz
    deg = csr.degree()
    print(f"[edge_dot] {name}: rows={rows} nnz={nnz} max degree={int(deg.max())} "
          f"median degree={int(deg.median())}", flush=True)
    for F in feats:
        a = torch.randn(rows, F, device=dev)
        b = torch.randn(csr.num_cols, F, device=dev)
        o = torch.empty(rows, F, device=dev)
        for H in heads_list:
            s = torch.empty(nnz, H, device=dev)
            passes = {
                "sddmm": lambda: K.edge_dot(csr.rowptr, csr.col, a, b, s, heads=H),
                "sum_fwd": lambda: K.spmm(csr.rowptr, csr.col, b, o),
            }
            times = timed(passes, rounds)
            nb = pass_bytes(nnz, rows, F, H, csr.col.element_size())
            rec = {"bench": "edge_dot", "graph": name, "rows": rows, "nnz": nnz,
                   "dtype": "fp32", "F": F, "heads": H, "rounds": rounds}
            med = {}
            for k, ts in times.items():
                rec[k] = stats(ts)
                med[k] = rec[k]["ms"]
                rec[k]["bytes"] = nb[k]
                rec[k]["TBps"] = round(nb[k] / med[k] / 1e9, 3)
            rec["sddmm_vs_sum"] = round(med["sddmm"] / med["sum_fwd"], 3)
            rec["from_bytes"] = round(nb["sddmm"] / nb["sum_fwd"], 3)
            rec["vs_target"] = round(rec["sddmm_vs_sum"] / (1.25 * rec["from_bytes"]), 3)
            print(json.dumps(rec), flush=True)
            del s
        del a, b, o


def composed_cases(name, csr, feats, heads_list, rounds, dev):
    from dgraph_amd.ops import kernels as K

    rows_of = csr.row_ids()
    col = csr.col.long()
    for F in feats:
        a = torch.randn(csr.num_rows, F, device=dev)
        b = torch.randn(csr.num_cols, F, device=dev)
        for H in heads_list:
            def composed():
                return (a[rows_of] * b[col]).view(csr.nnz, H, F // H).sum(-1)

            diff = float((composed() - K.edge_dot(csr.rowptr, csr.col, a, b, heads=H)).abs().max())
            times = timed({"sddmm": lambda: K.edge_dot(csr.rowptr, csr.col, a, b, heads=H),
                           "composed": composed}, rounds)
            rec = {"bench": "edge_dot_composed", "graph": name, "rows": csr.num_rows,
                   "nnz": csr.nnz, "dtype": "fp32", "F": F, "heads": H, "rounds": rounds,
                   "max_abs_diff": diff, "edge_tensor_bytes": csr.nnz * F * 4}
            for k, ts in times.items():
                rec[k] = stats(ts)
            rec["composed_over_sddmm"] = round(rec["composed"]["ms"] / rec["sddmm"]["ms"], 2)
            print(json.dumps(rec), flush=True)


def backward_cases(name, csr, feats, heads, rounds, dev):
    """``aggregate`` forward + backward with edge weights requiring grad: the time of the
    backward and the peak of allocated memory across it."""
    from dgraph_amd.ops.aggregate import aggregate

    csr.transpose()
    for F in feats:
        x = torch.randn(csr.num_cols, F, device=dev, requires_grad=True)
        w = torch.rand(csr.nnz, heads, device=dev, requires_grad=True)
        g = torch.randn(csr.num_rows, F, device=dev)
        ts, peaks = [], []
        for r in range(rounds + 1):
            x.grad = w.grad = None
            out = aggregate(x, csr, edge_weight=w, heads=heads)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            s.record()
            out.backward(g)
            e.record()
            torch.cuda.synchronize()
            if r > 0:
                ts.append(s.elapsed_time(e))
                peaks.append(torch.cuda.max_memory_allocated() - base)
            del out
        rec = {"bench": "aggregate_backward_edge_weight", "graph": name, "rows": csr.num_rows,
               "nnz": csr.nnz, "dtype": "fp32", "F": F, "heads": heads, "rounds": rounds,
               "backward": stats(ts), "peak_rise_bytes": max(peaks),
               "max_memory_allocated": torch.cuda.max_memory_allocated(),
               "edge_tensor_bytes": csr.nnz * F * 4}
        print(json.dumps(rec), flush=True)
        del x, w, g
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ogbn-products")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--feats", default="64,128,256")
    ap.add_argument("--heads", default="1,4")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--global-frac", type=float, default=0.05)
    ap.add_argument("--window", type=int, default=1 << 14)
    ap.add_argument("--powerlaw-rows", type=int, default=1 << 21,
                    help="rows of the power-law graph (0: skip it)")
    ap.add_argument("--composed-scale", type=float, default=0.05,
                    help="graph scale of the composed-expression comparison (0: skip it)")
    ap.add_argument("--backward-scale", type=float, default=0.05,
                    help="graph scale of the aggregate-backward comparison (0: skip it)")
    ap.add_argument("--backward-only", action="store_true",
                    help="only the aggregate-backward part (runs on earlier commits too)")
    a = ap.parse_args()
    from dgraph_amd.data.synthetic import SHAPES, build_partition

    if not torch.cuda.is_available():
        raise SystemExit("bench_edge_dot.py needs a GPU")
    dev = torch.device("cuda", 0)
    feats = [int(f) for f in a.feats.split(",")]
    heads = [int(h) for h in a.heads.split(",")]

    def graph(scale):
        shape = SHAPES[a.shape] if scale == 1.0 else SHAPES[a.shape].scaled(scale)
        p = build_partition(shape, 0, 1, dev, global_frac=a.global_frac, window=a.window)
        return shape.name, p["csr"]

    if not a.backward_only:
        name, csr = graph(a.scale)
        kernel_cases(name, csr, feats, heads, a.rounds, dev)
        del csr
        torch.cuda.empty_cache()
        if a.powerlaw_rows > 0:
            csr = powerlaw_csr(a.powerlaw_rows, dev)
            kernel_cases(f"powerlaw-{a.powerlaw_rows}", csr, feats, heads, a.rounds, dev)
            del csr
            torch.cuda.empty_cache()
        if a.composed_scale > 0:
            name, csr = graph(a.composed_scale)
            composed_cases(name, csr, feats, heads, a.rounds, dev)
            del csr
            torch.cuda.empty_cache()
    if a.backward_scale > 0:
        name, csr = graph(a.backward_scale)
        backward_cases(name, csr, feats, max(heads), a.rounds, dev)


if __name__ == "__main__":
    main()
