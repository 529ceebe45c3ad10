#!/usr/bin/env python3
"""Micro-benchmark of DropEdge fused into the CSR aggregation (csrc/kernels/spmm_drop.hip) next
to the plain fp32 SpMM on the same pattern and inputs in the same run, and next to the rebuild
it replaces.

Per (F, p) on the graph generator of benchmarks/bench_spmm.py (products-shaped by default),
timed in interleaved rounds with device events (one warm-up round, then ``--rounds`` timed
ones):

    spmm          K.spmm as it runs by default: the fp32 row-group kernel (spmm_f32.hip), every
                  entry gathered
    spmm_generic  K.spmm with the row-group kernel switched off: the generic one-wave-per-row
                  kernel (spmm_csr_v2_kernel), whose data flow the drop kernel shares
    drop_fwd     K.spmm_drop over the pattern: one Philox4x32-10 per entry, a ballot, the
                  kept entries compacted, only their rows gathered
    drop_T        K.spmm_drop over the transposed pattern with transposed=True (the backward)
    kept_degree   K.kept_degree: the mask counted, no feature traffic
    rebuild       what the fused kernels replace, for context: mask the edge list, then
                  CSR.from_coo and transpose() of the surviving edges (``--rebuild-rounds``
                  timed ones; host clock around a device synchronise, since it syncs inside)

One JSON line per (F, p): median / min / max ms, the bytes a pass must move once (the kept
share of the gathered rows for the drop passes) over the median time, and each drop pass over
the plain SpMM.
Example: python benchmarks/bench_drop_edge.py --rounds 7
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pass_bytes(nnz, kept, rows, F, isize):
    """Bytes a pass over ``rows`` output rows must move, every item once (fp32 rows): all
    column ids, the gathered rows of the ``kept`` entries, the output rows."""
    return nnz * isize + kept * 4 * F + rows * (4 * F + 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ogbn-products")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--widths", default="64,128,256")
    ap.add_argument("--p", default="0,0.1,0.5", help="comma list of drop probabilities")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rebuild-rounds", type=int, default=2)
    ap.add_argument("--global-frac", type=float, default=0.05)
    ap.add_argument("--window", type=int, default=1 << 14)
    a = ap.parse_args()
    from dgraph_amd import _native
    from dgraph_amd.data.synthetic import SHAPES, build_partition
    from dgraph_amd.ops import kernels as K
    from dgraph_amd.ops.csr import CSR
    from dgraph_amd.ops.philox import edge_keep_mask

    if not torch.cuda.is_available():
        raise SystemExit("bench_drop_edge.py needs a GPU")
    assert _native.load(), "native library missing"
    ops = _native.ops()
    dev = torch.device("cuda", 0)
    shape = SHAPES[a.shape] if a.scale == 1.0 else SHAPES[a.shape].scaled(a.scale)
    part = build_partition(shape, 0, 1, dev, global_frac=a.global_frac, window=a.window)
    csr = part["csr"]
    t = csr.transpose()
    rows, cols, nnz = csr.num_rows, csr.num_cols, csr.nnz
    isize = csr.col.element_size()
    seed = torch.tensor([20240607], dtype=torch.int64, device=dev)
    print(f"[drop_edge] rows={rows} cols={cols} nnz={nnz} "
          f"max degree={int(csr.degree().max())}", flush=True)
    erow = csr.row_ids()
    ecol = csr.col.long()

    def rebuild(p):
        keep = edge_keep_mask(seed, erow, ecol, p)
        sub = CSR.from_coo(erow[keep], ecol[keep], rows, cols)
        sub.transpose()
        return sub

    for p in [float(s) for s in a.p.split(",")]:
        kept_total = int(K.kept_degree(csr.rowptr, csr.col, seed=seed, p=p,
                                       num_cols=cols).sum())
        rb = []
        for r in range(a.rebuild_rounds + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sub = rebuild(p)
            torch.cuda.synchronize()
            if r > 0:
                rb.append((time.perf_counter() - t0) * 1e3)
            assert sub.nnz == kept_total
            del sub
        for F in [int(s) for s in a.widths.split(",")]:
            x = torch.randn(cols, F, device=dev)
            g = torch.randn(rows, F, device=dev)
            out = torch.empty(rows, F, device=dev)
            gx = torch.empty(cols, F, device=dev)
            kept = torch.empty(rows, dtype=torch.int32, device=dev)
            def spmm_generic():
                ops.set_spmm_f32_config(0)
                try:
                    K.spmm(csr.rowptr, csr.col, x, out)
                finally:
                    ops.set_spmm_f32_config(1)

            passes = {
                "spmm": lambda: K.spmm(csr.rowptr, csr.col, x, out),
                "spmm_generic": spmm_generic,
                "drop_fwd": lambda: K.spmm_drop(csr.rowptr, csr.col, x, out, seed=seed, p=p),
                "drop_T": lambda: K.spmm_drop(t.rowptr, t.col, g, gx, seed=seed, p=p,
                                              transposed=True),
                "kept_degree": lambda: K.kept_degree(csr.rowptr, csr.col, kept, seed=seed, p=p,
                                                     num_cols=cols),
            }
            times = {n: [] for n in passes}
            for r in range(a.rounds + 1):  # round 0 warms every pass up
                for n, fn in passes.items():
                    s, e = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                    torch.cuda.synchronize()
                    s.record()
                    fn()
                    e.record()
                    torch.cuda.synchronize()
                    if r > 0:
                        times[n].append(s.elapsed_time(e))
            nb = {"spmm": pass_bytes(nnz, nnz, rows, F, isize),
                  "spmm_generic": pass_bytes(nnz, nnz, rows, F, isize),
                  "drop_fwd": pass_bytes(nnz, kept_total, rows, F, isize),
                  "drop_T": pass_bytes(nnz, kept_total, cols, F, t.col.element_size()),
                  "kept_degree": nnz * isize + rows * 12}
            rec = {"bench": "drop_edge", "shape": shape.name, "rows": rows, "nnz": nnz, "F": F,
                   "p": p, "kept": kept_total, "rounds": a.rounds}
            med = {}
            for n, ts in times.items():
                med[n] = statistics.median(ts)
                rec[n] = {"ms": round(med[n], 3), "ms_min": round(min(ts), 3),
                          "ms_max": round(max(ts), 3), "bytes": nb[n],
                          "TBps": round(nb[n] / med[n] / 1e9, 3)}
            rec["rebuild"] = {"ms": round(statistics.median(rb), 1), "ms_min": round(min(rb), 1),
                              "ms_max": round(max(rb), 1), "rounds": len(rb)}
            rec["drop_fwd_over_spmm"] = round(med["drop_fwd"] / med["spmm"], 3)
            rec["drop_T_over_spmm"] = round(med["drop_T"] / med["spmm"], 3)
            rec["drop_fwd_over_generic"] = round(med["drop_fwd"] / med["spmm_generic"], 3)
            rec["drop_T_over_generic"] = round(med["drop_T"] / med["spmm_generic"], 3)
            print(json.dumps(rec), flush=True)
            del x, g, out, gx, kept
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
