#!/usr/bin/env python3
"""Micro-benchmark of the gated aggregation kernels with bf16 storage
(csrc/kernels/spmm_gated_bf16.hip) next to the fp32 ones (spmm_gated.hip) on the default graph
of benchmarks/bench_gated_aggr.py, in the same run.

Per F, timed in interleaved rounds with device events (one warm-up round, then ``--rounds``
timed ones; ``--inner`` launches per timed window); ``q | v`` are the halves of one ``[N, 2F]``
buffer and ``dq | dv`` of another, in both dtypes:

    f32_fwd / f32_fwd_ds / f32_bwd     K.segment_gated (without / with ds), bwd_src on fp32 rows
    bf16_fwd / bf16_fwd_ds / bf16_bwd  the same on bf16 rows, bf16 outputs (the direct store)
    acc_fwd_ds / acc_bwd               bf16 rows into fp32 outputs plus the cast to bf16: what a
                                       partition with a halo block runs before / after its
                                       second pass (the accumulate-and-cast path)

One JSON line per F: median / min / max ms per launch, the bytes each pass must move once
(gathered rows + ids + what it reads and writes per row; from the shapes) over the median, the
bf16 / fp32 ratio of every pass and ``acc_over_direct``. Nothing is asserted on any ratio.
Example: python benchmarks/bench_gated_aggr_bf16.py --rounds 7
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KINDS = ("fwd", "fwd_ds", "bwd")


def pass_bytes(nnz, rows, cols, F, isize):
    """Bytes each pass must move: two gathered rows and an id per entry; k in and out (and ds)
    out per row; q, v in and dq, dv out per source row. ``acc``: fp32 out, then its cast."""
    nb = {}
    for tag, es in (("f32", 4), ("bf16", 2)):
        two = nnz * (2 * es * F + isize)
        nb[f"{tag}_fwd"] = two + rows * F * 2 * es
        nb[f"{tag}_fwd_ds"] = two + rows * F * 3 * es
        nb[f"{tag}_bwd"] = two + cols * F * 4 * es
    two = nnz * (4 * F + isize)
    nb["acc_fwd_ds"] = two + rows * F * (2 + 2 * 4) + 2 * rows * F * (4 + 2)
    nb["acc_bwd"] = two + cols * F * (2 * 2 + 2 * 4) + 2 * cols * F * (4 + 2)
    return nb


def make_passes(K, csr, t, tag, k, qv, g, F, odt):
    """The three launches of one dtype over its own operands and outputs."""
    rows, cols = csr.num_rows, t.num_rows
    q, v = qv[:, :F], qv[:, F:]
    out, ds = (torch.empty(rows, F, dtype=odt, device=k.device) for _ in range(2))
    dqv = torch.empty(cols, 2 * F, dtype=odt, device=k.device)
    fwd = lambda: K.segment_gated(csr.rowptr, csr.col, k, q, v, out)  # noqa: E731
    fwd_ds = lambda: K.segment_gated(csr.rowptr, csr.col, k, q, v, out, ds)  # noqa: E731
    bwd = lambda: K.segment_gated_bwd_src(t.rowptr, t.col, k, q, v, g, dqv[:, :F],  # noqa: E731
                                          dqv[:, F:])
    if tag != "acc":
        return {f"{tag}_fwd": fwd, f"{tag}_fwd_ds": fwd_ds, f"{tag}_bwd": bwd}
    return {"acc_fwd_ds": lambda: (fwd_ds(), out.to(k.dtype), ds.to(k.dtype)),
            "acc_bwd": lambda: (bwd(), dqv.to(k.dtype))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ogbn-products")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--feats", default="64,128,256")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3, help="launches per timed window")
    ap.add_argument("--global-frac", type=float, default=0.05)
    ap.add_argument("--window", type=int, default=1 << 14)
    a = ap.parse_args()
    from dgraph_amd.data.synthetic import SHAPES, build_partition
    from dgraph_amd.ops import kernels as K

    if not torch.cuda.is_available():
        raise SystemExit("bench_gated_aggr_bf16.py needs a GPU")
    dev = torch.device("cuda", 0)
    shape = SHAPES[a.shape] if a.scale == 1.0 else SHAPES[a.shape].scaled(a.scale)
    p = build_partition(shape, 0, 1, dev, global_frac=a.global_frac, window=a.window)
    csr = p["csr"]
    t = csr.transpose()
    rows, cols, nnz = csr.num_rows, t.num_rows, csr.nnz
    print(f"[gated_bf16] rows={rows} nnz={nnz} max degree={int(csr.degree().max())}",
          flush=True)
    for F in [int(f) for f in a.feats.split(",")]:
        k, qv, g = (torch.randn(n, w, device=dev) for n, w in ((rows, F), (cols, 2 * F),
                                                                (rows, F)))
        kb, qvb, gb = k.bfloat16(), qv.bfloat16(), g.bfloat16()
        passes = make_passes(K, csr, t, "f32", k, qv, g, F, torch.float32)
        passes.update(make_passes(K, csr, t, "bf16", kb, qvb, gb, F, torch.bfloat16))
        passes.update(make_passes(K, csr, t, "acc", kb, qvb, gb, F, torch.float32))
        times = {n: [] for n in passes}
        for r in range(a.rounds + 1):  # round 0 warms every pass up
            for n, fn in passes.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                s.record()
                for _ in range(a.inner):
                    fn()
                e.record()
                torch.cuda.synchronize()
                if r > 0:
                    times[n].append(s.elapsed_time(e) / a.inner)
        nb = pass_bytes(nnz, rows, cols, F, csr.col.element_size())
        rec = {"bench": "gated_aggr_bf16", "shape": shape.name, "rows": rows, "nnz": nnz,
               "F": F, "rounds": a.rounds, "inner": a.inner}
        med = {}
        for n, ts in times.items():
            med[n] = statistics.median(ts)
            rec[n] = {"ms": round(med[n], 3), "ms_min": round(min(ts), 3),
                      "ms_max": round(max(ts), 3), "bytes": nb[n],
                      "TBps": round(nb[n] / med[n] / 1e9, 3)}
        for kind in KINDS:
            rec[f"bf16_{kind}_over_f32_{kind}"] = round(med[f"bf16_{kind}"] / med[f"f32_{kind}"], 3)
        for kind in ("fwd_ds", "bwd"):
            rec[f"acc_over_direct_{kind}"] = round(med[f"acc_{kind}"] / med[f"bf16_{kind}"], 3)
        print(json.dumps(rec), flush=True)
        del k, qv, g, kb, qvb, gb, passes


if __name__ == "__main__":
    main()
