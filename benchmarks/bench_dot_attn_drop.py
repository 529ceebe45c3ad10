#!/usr/bin/env python3
"""Micro-benchmark of the fused dot-product attention kernels with attention dropout
(csrc/kernels/dot_attn_drop_f32.hip) next to the plain kernels (dot_attn_f32.hip), on the same
pattern and inputs in the same run.

Per (C, heads) case on the graph generator of benchmarks/bench_spmm.py, timed in interleaved
rounds with device events (one warm-up round, then ``--rounds`` timed ones), at each ``--p``:

    dot_fwd / dot_bwd_dst / dot_bwd_src      the plain kernels (no dropout)
    drop_fwd       dot_attn_drop_fwd_f32: the same gathers; one Philox4x32-10 call per entry
                   (two at 8 heads) on the lane that loads the entry's column id
    drop_bwd_dst   dot_attn_drop_bwd_dst_f32: the same, the mask regenerated
    drop_bwd_src   dot_attn_drop_bwd_src_f32 over the transpose: also loads t_slot per entry
    op             ops.dot_attention(..., dropout_p=) forward + backward (skipped with
                   --kernels-only)

The dropout kernels move the plain kernels' bytes (the source side 4 or 8 more per entry for
``t_slot``): the mask is never stored. One JSON line per case and p: median / min / max ms,
the bytes each pass must move once over the median time, and each dropout kernel's time over
its plain counterpart.
Example: python benchmarks/bench_dot_attn_drop.py --rounds 7
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pass_bytes(nnz, rows, cols, C, H, isize):
    """Bytes each pass must move, every item once (fp32)."""
    row, st = 4 * C, 4 * H
    fwd = nnz * (2 * row + isize) + rows * (2 * row + 2 * st)
    dst = nnz * (2 * row + isize) + rows * (3 * row + 3 * st)
    src = nnz * (2 * row + 3 * st + isize) + cols * 4 * row
    return {"dot_fwd": fwd, "dot_bwd_dst": dst, "dot_bwd_src": src, "drop_fwd": fwd,
            "drop_bwd_dst": dst, "drop_bwd_src": src + nnz * isize}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ogbn-products")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--cases", default="256:4,128:1", help="comma list of C:heads")
    ap.add_argument("--p", default="0.1,0.5", help="comma list of dropout probabilities")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--global-frac", type=float, default=0.05)
    ap.add_argument("--window", type=int, default=1 << 14)
    ap.add_argument("--kernels-only", action="store_true", help="time the six kernels only")
    a = ap.parse_args()
    from dgraph_amd import _native
    from dgraph_amd.data.synthetic import SHAPES, build_partition
    from dgraph_amd.ops.dot_attn import dot_attention
    from dgraph_amd.ops.gat import GatPattern

    if not torch.cuda.is_available():
        raise SystemExit("bench_dot_attn_drop.py needs a GPU")
    ops = _native.ops()
    dev = torch.device("cuda", 0)
    shape = SHAPES[a.shape] if a.scale == 1.0 else SHAPES[a.shape].scaled(a.scale)
    part = build_partition(shape, 0, 1, dev, global_frac=a.global_frac, window=a.window)
    csr = part["csr"]
    rows, cols, nnz = csr.num_rows, csr.num_cols, csr.nnz
    pat = GatPattern(csr.rowptr, csr.col, cols, 0)
    t_slot = pat.t_slot
    seed = torch.tensor([20240607], dtype=torch.int64, device=dev)
    print(f"[dot_attn_drop] rows={rows} cols={cols} nnz={nnz} "
          f"max degree={int(csr.degree().max())}", flush=True)
    f = lambda *s: torch.randn(*s, device=dev)  # noqa: E731
    for C, H in [tuple(int(t) for t in c.split(":")) for c in a.cases.split(",")]:
        scale = 1.0 / math.sqrt(C // H)
        q, g = f(rows, C), f(rows, C)
        kv = f(cols, 2 * C)
        k, v = kv[:, :C], kv[:, C:]
        out, dq = torch.empty(rows, C, device=dev), torch.empty(rows, C, device=dev)
        dk, dv = torch.empty(cols, C, device=dev), torch.empty(cols, C, device=dev)
        m, l = torch.empty(rows, H, device=dev), torch.empty(rows, H, device=dev)
        c = torch.empty(rows, H, device=dev)
        kvg = qg = None
        if not a.kernels_only:
            kvg = kv.clone().requires_grad_()
            qg = q.clone().requires_grad_()
        for p in [float(t) for t in a.p.split(",")]:

            def dot_fwd():
                ops.dot_attn_fwd_f32(pat.rowptr, pat.col, q, k, v, None, None, cols, out, 0.0,
                                     m, l, H, scale)

            def dot_bwd_dst():
                ops.dot_attn_bwd_dst_f32(pat.rowptr, pat.col, q, k, v, None, None, cols, m, l,
                                         g, c, dq, H, scale)

            def dot_bwd_src():
                ops.dot_attn_bwd_src_f32(pat.t_rowptr, pat.t_col, q, g, k, v, m, l, c, dk, dv,
                                         H, scale)

            def drop_fwd():
                ops.dot_attn_drop_fwd_f32(pat.rowptr, pat.col, q, k, v, None, None, cols, out,
                                          m, l, seed, p, H, scale)

            def drop_bwd_dst():
                ops.dot_attn_drop_bwd_dst_f32(pat.rowptr, pat.col, q, k, v, None, None, cols, m,
                                              l, g, c, dq, seed, p, H, scale)

            def drop_bwd_src():
                ops.dot_attn_drop_bwd_src_f32(pat.t_rowptr, pat.t_col, t_slot, q, g, k, v, m, l,
                                              c, dk, dv, seed, p, H, scale)

            def op():
                qg.grad = kvg.grad = None
                dot_attention(qg, kvg[:, :C], kvg[:, C:], pat, heads=H, dropout_p=p,
                              dropout_seed=seed).backward(g)

            # each backward kernel reads the statistics and c = <g, out> per head of ITS
            # forward: the plain group runs on the plain forward's, the dropout group on its own
            def prepare(fwd):
                fwd()
                c.copy_((g * out).view(rows, H, C // H).sum(-1))

            groups = [("dot", dot_fwd, {"dot_fwd": dot_fwd, "dot_bwd_dst": dot_bwd_dst,
                                        "dot_bwd_src": dot_bwd_src}),
                      ("drop", drop_fwd, {"drop_fwd": drop_fwd, "drop_bwd_dst": drop_bwd_dst,
                                          "drop_bwd_src": drop_bwd_src})]
            extra = {} if a.kernels_only else {"op": op}
            names = [n for _, _, ps in groups for n in ps] + list(extra)
            times = {n: [] for n in names}

            def timed(n, fn, keep):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                s.record()
                fn()
                e.record()
                torch.cuda.synchronize()
                if keep:
                    times[n].append(s.elapsed_time(e))

            for r in range(a.rounds + 1):  # round 0 warms every pass up
                for _, fwd, ps in groups:
                    prepare(fwd)
                    for n, fn in ps.items():
                        timed(n, fn, r > 0)
                for n, fn in extra.items():
                    timed(n, fn, r > 0)
            nb = pass_bytes(nnz, rows, cols, C, H, pat.col.element_size())
            rec = {"bench": "dot_attn_drop", "shape": shape.name, "rows": rows, "nnz": nnz,
                   "C": C, "heads": H, "p": p, "rounds": a.rounds}
            med = {}
            for n, ts in times.items():
                med[n] = statistics.median(ts)
                rec[n] = {"ms": round(med[n], 3), "ms_min": round(min(ts), 3),
                          "ms_max": round(max(ts), 3)}
                if n in nb:
                    rec[n].update(bytes=nb[n], TBps=round(nb[n] / med[n] / 1e9, 3))
            for n in ("fwd", "bwd_dst", "bwd_src"):
                rec[f"drop_{n}_over_dot_{n}"] = round(med[f"drop_{n}"] / med[f"dot_{n}"], 3)
            plain3 = med["dot_fwd"] + med["dot_bwd_dst"] + med["dot_bwd_src"]
            drop3 = med["drop_fwd"] + med["drop_bwd_dst"] + med["drop_bwd_src"]
            rec["drop_three_over_dot_three"] = round(drop3 / plain3, 3)
            if not a.kernels_only:
                rec["op_over_three_kernels"] = round(med["op"] / drop3, 3)
            print(json.dumps(rec), flush=True)
        del q, g, kv, k, v, out, dq, dk, dv, kvg, qg
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
