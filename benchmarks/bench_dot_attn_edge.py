#!/usr/bin/env python3
"""Micro-benchmark of the fused dot-product attention kernels with edge features
(csrc/kernels/dot_attn_edge_f32.hip) next to the plain kernels (dot_attn_f32.hip) and next to
the composed per-edge formulation, on the same pattern and inputs in the same run.

Per (C, heads) case on the graph generator of benchmarks/bench_spmm.py, timed in interleaved
rounds with device events (one warm-up round, then ``--rounds`` timed ones):

    dot_fwd / dot_bwd_dst / dot_bwd_src      the plain kernels (no edge term)
    edge_fwd       dot_attn_edge_fwd_f32: gathers k_j, v_j, streams ee_p
    edge_bwd_dst   dot_attn_edge_bwd_dst_f32: the same reads; writes dee_p and w_p per entry
    edge_bwd_src   dot_attn_edge_bwd_src_f32 over the transpose: gathers q_i, g_i, w[t_slot]
    op             ops.dot_attention(..., edge=) forward + backward
    composed       the same function from the existing ops: row gathers of q_i, k_j, v_j into
                   [E, C], the adds, the per-head scores, edge_softmax, the weighted
                   scatter-sum, and autograd's backward of all of it (skipped with
                   --kernels-only)

``ee`` and ``dee`` are 4 C E bytes each and the composed path keeps a dozen or so [E, C]
tensors alive through its backward, so the default ``--scale`` is 0.05 of ogbn-products; the
sizes are printed. One JSON line per case: median / min / max ms, the bytes each pass must
move once (computed from the shapes below) over the median time, each edge kernel's time over
its plain counterpart, and the op over the composed path.
Example: python benchmarks/bench_dot_attn_edge.py --rounds 7
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
    return {
        # k_j and v_j per entry; q in, out + 2 statistics out per row
        "dot_fwd": nnz * (2 * row + isize) + rows * (2 * row + 2 * st),
        # k_j and v_j per entry; q, g, 3 statistics in, dq out per row
        "dot_bwd_dst": nnz * (2 * row + isize) + rows * (3 * row + 3 * st),
        # q_i, g_i and 3 statistics per entry; k, v in, dk, dv out per source row
        "dot_bwd_src": nnz * (2 * row + 3 * st + isize) + cols * 4 * row,
        # + ee_p per entry
        "edge_fwd": nnz * (3 * row + isize) + rows * (2 * row + 2 * st),
        # + ee_p in, dee_p and the two weights out per entry
        "edge_bwd_dst": nnz * (4 * row + 2 * st + isize) + rows * (3 * row + 3 * st),
        # q_i, g_i, the slot and its two weights per entry; dk, dv out per source row
        "edge_bwd_src": nnz * (2 * row + 2 * st + 2 * isize) + cols * 2 * row,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ogbn-products")
    ap.add_argument("--scale", type=float, default=0.05)
    ap.add_argument("--cases", default="256:4,128:1", help="comma list of C:heads")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--global-frac", type=float, default=0.05)
    ap.add_argument("--window", type=int, default=1 << 14)
    ap.add_argument("--kernels-only", action="store_true",
                    help="time the six kernels only (no op, no composed path: larger scales)")
    a = ap.parse_args()
    from dgraph_amd import _native
    from dgraph_amd.data.synthetic import SHAPES, build_partition
    from dgraph_amd.ops.aggregate import edge_softmax, gather, scatter_sum
    from dgraph_amd.ops.csr import IndexMap
    from dgraph_amd.ops.dot_attn import dot_attention
    from dgraph_amd.ops.gat import GatPattern

    if not torch.cuda.is_available():
        raise SystemExit("bench_dot_attn_edge.py needs a GPU")
    ops = _native.ops()
    dev = torch.device("cuda", 0)
    shape = SHAPES[a.shape] if a.scale == 1.0 else SHAPES[a.shape].scaled(a.scale)
    p = build_partition(shape, 0, 1, dev, global_frac=a.global_frac, window=a.window)
    csr = p["csr"]
    rows, cols, nnz = csr.num_rows, csr.num_cols, csr.nnz
    pat = GatPattern(csr.rowptr, csr.col, cols, 0)
    t_slot = pat.t_slot
    row_map = IndexMap(csr.row_ids(), rows)
    col_map = IndexMap(csr.col.long(), cols)
    print(f"[dot_attn_edge] rows={rows} cols={cols} nnz={nnz} "
          f"max degree={int(csr.degree().max())}", flush=True)
    f = lambda *s: torch.randn(*s, device=dev)  # noqa: E731
    for C, H in [tuple(int(t) for t in c.split(":")) for c in a.cases.split(",")]:
        scale = 1.0 / math.sqrt(C // H)
        D = C // H
        gib = lambda n: n / 2 ** 30  # noqa: E731
        print(f"[dot_attn_edge] C={C} heads={H}: ee and dee {gib(4 * C * nnz):.2f} GiB each, "
              f"w {gib(8 * H * nnz):.3f} GiB, a [rows, C] array {gib(4 * C * rows):.3f} GiB",
              flush=True)
        q, g = f(rows, C), f(rows, C)
        kv = f(cols, 2 * C)
        k, v = kv[:, :C], kv[:, C:]
        ee = f(nnz, C).mul_(0.25)
        out, dq = torch.empty(rows, C, device=dev), torch.empty(rows, C, device=dev)
        dk, dv = torch.empty(cols, C, device=dev), torch.empty(cols, C, device=dev)
        m, l = torch.empty(rows, H, device=dev), torch.empty(rows, H, device=dev)
        c = torch.empty(rows, H, device=dev)
        dee = torch.empty(nnz, C, device=dev)
        w = torch.empty(nnz, 2 * H, device=dev)
        kvg = qg = eeg = None
        if not a.kernels_only:
            kvg = kv.clone().requires_grad_()
            qg = q.clone().requires_grad_()
            eeg = ee.clone().requires_grad_()

        def dot_fwd():
            ops.dot_attn_fwd_f32(pat.rowptr, pat.col, q, k, v, None, None, cols, out, 0.0, m, l,
                                 H, scale)

        def dot_bwd_dst():
            ops.dot_attn_bwd_dst_f32(pat.rowptr, pat.col, q, k, v, None, None, cols, m, l, g, c,
                                     dq, H, scale)

        def dot_bwd_src():
            ops.dot_attn_bwd_src_f32(pat.t_rowptr, pat.t_col, q, g, k, v, m, l, c, dk, dv, H,
                                     scale)

        def edge_fwd():
            ops.dot_attn_edge_fwd_f32(pat.rowptr, pat.col, q, k, v, None, None, cols, ee, out,
                                      0.0, m, l, H, scale)

        def edge_bwd_dst():
            ops.dot_attn_edge_bwd_dst_f32(pat.rowptr, pat.col, q, k, v, None, None, cols, ee, m,
                                          l, g, c, dq, dee, w, H, scale)

        def edge_bwd_src():
            ops.dot_attn_edge_bwd_src_f32(pat.t_rowptr, pat.t_col, t_slot, q, g, w, dk, dv, H,
                                          scale)

        def op():
            qg.grad = kvg.grad = eeg.grad = None
            dot_attention(qg, kvg[:, :C], kvg[:, C:], pat, heads=H, edge=eeg).backward(g)

        def composed():
            qg.grad = kvg.grad = eeg.grad = None
            qe = gather(qg, row_map)
            kve = gather(kvg, col_map)
            ke, ve = kve[:, :C] + eeg, kve[:, C:] + eeg
            s = (qe * ke).view(nnz, H, D).sum(-1) * scale
            alpha = edge_softmax(s, csr)
            msg = (ve.view(nnz, H, D) * alpha.unsqueeze(-1)).view(nnz, C)
            scatter_sum(msg, row_map).backward(g)

        # each backward kernel reads the statistics and c = <g, out> per head of ITS forward:
        # the plain group runs on the plain forward's, the edge group on the edge forward's
        def prepare(fwd):
            fwd()
            c.copy_((g * out).view(rows, H, C // H).sum(-1))

        groups = [("dot", dot_fwd, {"dot_fwd": dot_fwd, "dot_bwd_dst": dot_bwd_dst,
                                    "dot_bwd_src": dot_bwd_src}),
                  ("edge", edge_fwd, {"edge_fwd": edge_fwd, "edge_bwd_dst": edge_bwd_dst,
                                      "edge_bwd_src": edge_bwd_src})]
        extra = {} if a.kernels_only else {"op": op, "composed": composed}
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
        if not a.kernels_only:  # the two paths compute the same function
            op()
            ref = [t.grad.clone() for t in (qg, kvg, eeg)]
            composed()
            for name, x, y in zip(("dq", "dkv", "dee"), ref, (qg.grad, kvg.grad, eeg.grad)):
                err = float((x - y).abs().max()) / max(1.0, float(y.abs().max()))
                print(f"[dot_attn_edge] op against composed, {name}: {err:.2e}", flush=True)
        nb = pass_bytes(nnz, rows, cols, C, H, pat.col.element_size())
        rec = {"bench": "dot_attn_edge", "shape": shape.name, "rows": rows, "nnz": nnz, "C": C,
               "heads": H, "rounds": a.rounds, "ee_bytes": 4 * C * nnz}
        med = {}
        for n, ts in times.items():
            med[n] = statistics.median(ts)
            rec[n] = {"ms": round(med[n], 3), "ms_min": round(min(ts), 3),
                      "ms_max": round(max(ts), 3)}
            if n in nb:
                rec[n].update(bytes=nb[n], TBps=round(nb[n] / med[n] / 1e9, 3))
        for n in ("fwd", "bwd_dst", "bwd_src"):
            rec[f"edge_{n}_over_dot_{n}"] = round(med[f"edge_{n}"] / med[f"dot_{n}"], 3)
        if not a.kernels_only:
            rec["op_over_three_kernels"] = round(
                med["op"] / (med["edge_fwd"] + med["edge_bwd_dst"] + med["edge_bwd_src"]), 3)
            rec["op_over_composed"] = round(med["op"] / med["composed"], 3)
        print(json.dumps(rec), flush=True)
        del q, g, kv, k, v, ee, out, dq, dk, dv, dee, w, kvg, qg, eeg
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
