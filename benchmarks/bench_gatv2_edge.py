#!/usr/bin/env python3
"""Micro-benchmark of the fused GATv2 attention kernels with edge features
(csrc/kernels/gatv2_edge_f32.hip) next to the plain kernels (gatv2_f32.hip) and next to the
composed per-edge formulation, on the same pattern and inputs in the same run.

Per (C, heads) case on the graph generator of benchmarks/bench_spmm.py, timed in interleaved
rounds with device events (one warm-up round, then ``--rounds`` timed ones):

    v2_fwd / v2_bwd_dst / v2_bwd_src         the plain kernels (no edge term)
    edge_fwd       gatv2_edge_fwd_f32: gathers r_j, streams ee_p
    edge_bwd_dst   gatv2_edge_bwd_dst_f32: the same reads; writes dee_p and w_p per entry
    edge_bwd_src   gatv2_edge_bwd_src_f32 over the transpose: gathers g_i, dee and w by t_slot
    op             ops.gatv2_attention(..., edge=) forward + backward
    composed       the same function from the existing ops: row gathers of l_i and r_j into
                   [E, C], the adds, LeakyReLU, the per-head scores, edge_softmax, the
                   weighted scatter-sum, and autograd's backward of all of it (skipped with
                   --kernels-only)

``ee`` and ``dee`` are 4 C E bytes each and the composed path keeps a dozen or so [E, C]
tensors alive through its backward, so the default ``--scale`` is 0.05 of ogbn-products; the
sizes are printed. One JSON line per case: median / min / max ms, the bytes each pass must
move once (computed from the shapes below) over the median time, each edge kernel's time over
its plain counterpart, and the op over the composed path.
Example: python benchmarks/bench_gatv2_edge.py --rounds 7
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
        # r_j per entry; l in, out + 2 statistics out per row
        "v2_fwd": nnz * (row + isize) + rows * (2 * row + 2 * st),
        # r_j per entry; l, g, 3 statistics in, dl out per row
        "v2_bwd_dst": nnz * (row + isize) + rows * (3 * row + 3 * st),
        # l_i, g_i and 3 statistics per entry; r in, dr out per source row
        "v2_bwd_src": nnz * (2 * row + 3 * st + isize) + cols * 2 * row,
        # + ee_p per entry
        "edge_fwd": nnz * (2 * row + isize) + rows * (2 * row + 2 * st),
        # + ee_p in, dee_p and the weight out per entry
        "edge_bwd_dst": nnz * (3 * row + st + isize) + rows * (3 * row + 3 * st),
        # g_i, dee[slot], the slot and its weight per entry; dr out per source row
        "edge_bwd_src": nnz * (2 * row + st + 2 * isize) + cols * row,
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
    from dgraph_amd.ops.gat import GatPattern
    from dgraph_amd.ops.gatv2 import gatv2_attention

    if not torch.cuda.is_available():
        raise SystemExit("bench_gatv2_edge.py needs a GPU")
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
    print(f"[gatv2_edge] rows={rows} cols={cols} nnz={nnz} "
          f"max degree={int(csr.degree().max())}", flush=True)
    f = lambda *s: torch.randn(*s, device=dev)  # noqa: E731
    slope = 0.2
    for C, H in [tuple(int(t) for t in c.split(":")) for c in a.cases.split(",")]:
        D = C // H
        gib = lambda n: n / 2 ** 30  # noqa: E731
        print(f"[gatv2_edge] C={C} heads={H}: ee and dee {gib(4 * C * nnz):.2f} GiB each, "
              f"w {gib(4 * H * nnz):.3f} GiB, a [rows, C] array {gib(4 * C * rows):.3f} GiB",
              flush=True)
        l, g, r = f(rows, C), f(rows, C), f(cols, C)
        att = f(C).mul_(0.5 / math.sqrt(D))
        ee = f(nnz, C).mul_(0.25)
        out, dl = torch.empty(rows, C, device=dev), torch.empty(rows, C, device=dev)
        dr = torch.empty(cols, C, device=dev)
        m, ls = torch.empty(rows, H, device=dev), torch.empty(rows, H, device=dev)
        c = torch.empty(rows, H, device=dev)
        dee = torch.empty(nnz, C, device=dev)
        w = torch.empty(nnz, H, device=dev)
        da_part = torch.empty(ops.gatv2_da_parts(rows, C), C, device=dev)
        grad_ins = []
        if not a.kernels_only:
            grad_ins = [t.clone().requires_grad_() for t in (l, r, att, ee)]

        def v2_fwd():
            ops.gatv2_fwd_f32(pat.rowptr, pat.col, l, r, None, cols, att, out, 0.0, m, ls, H,
                              slope)

        def v2_bwd_dst():
            ops.gatv2_bwd_dst_f32(pat.rowptr, pat.col, l, r, None, cols, att, m, ls, g, c, dl,
                                  da_part, H, slope)

        def v2_bwd_src():
            ops.gatv2_bwd_src_f32(pat.t_rowptr, pat.t_col, l, g, r, att, m, ls, c, dr, H, slope)

        def edge_fwd():
            ops.gatv2_edge_fwd_f32(pat.rowptr, pat.col, l, r, None, cols, ee, att, out, 0.0, m,
                                   ls, H, slope)

        def edge_bwd_dst():
            ops.gatv2_edge_bwd_dst_f32(pat.rowptr, pat.col, l, r, None, cols, ee, att, m, ls, g,
                                       c, dl, dee, w, da_part, H, slope)

        def edge_bwd_src():
            ops.gatv2_edge_bwd_src_f32(pat.t_rowptr, pat.t_col, t_slot, g, w, dee, dr, H)

        def clear():
            for t in grad_ins:
                t.grad = None

        def op():
            clear()
            lg, rg, ag, eg = grad_ins
            gatv2_attention(lg, rg, ag, pat, heads=H, negative_slope=slope,
                            edge=eg).backward(g)

        def composed():
            clear()
            lg, rg, ag, eg = grad_ins
            re = gather(rg, col_map)
            act = torch.nn.functional.leaky_relu(gather(lg, row_map) + re + eg, slope)
            s = (act * ag).view(nnz, H, D).sum(-1)
            alpha = edge_softmax(s, csr)
            msg = (re.view(nnz, H, D) * alpha.unsqueeze(-1)).view(nnz, C)
            scatter_sum(msg, row_map).backward(g)

        # each backward kernel reads the statistics and c = <g, out> per head of ITS forward:
        # the plain group runs on the plain forward's, the edge group on the edge forward's
        def prepare(fwd):
            fwd()
            c.copy_((g * out).view(rows, H, D).sum(-1))

        groups = [(v2_fwd, {"v2_fwd": v2_fwd, "v2_bwd_dst": v2_bwd_dst,
                            "v2_bwd_src": v2_bwd_src}),
                  (edge_fwd, {"edge_fwd": edge_fwd, "edge_bwd_dst": edge_bwd_dst,
                              "edge_bwd_src": edge_bwd_src})]
        extra = {} if a.kernels_only else {"op": op, "composed": composed}
        times = {n: [] for _, ps in groups for n in ps}
        times.update({n: [] for n in extra})

        def timed(n, fn, keep):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            if keep:
                times[n].append(s.elapsed_time(e))

        for rnd in range(a.rounds + 1):  # round 0 warms every pass up
            for fwd, ps in groups:
                prepare(fwd)
                for n, fn in ps.items():
                    timed(n, fn, rnd > 0)
            for n, fn in extra.items():
                timed(n, fn, rnd > 0)
        if not a.kernels_only:  # the two paths compute the same function
            op()
            ref = [t.grad.clone() for t in grad_ins]
            composed()
            for name, x, t in zip(("dl", "dr", "datt", "dee"), ref, grad_ins):
                err = float((x - t.grad).abs().max()) / max(1.0, float(t.grad.abs().max()))
                print(f"[gatv2_edge] op against composed, {name}: {err:.2e}", flush=True)
        nb = pass_bytes(nnz, rows, cols, C, H, pat.col.element_size())
        rec = {"bench": "gatv2_edge", "shape": shape.name, "rows": rows, "nnz": nnz, "C": C,
               "heads": H, "rounds": a.rounds, "ee_bytes": 4 * C * nnz}
        med = {}
        for n, ts in times.items():
            med[n] = statistics.median(ts)
            rec[n] = {"ms": round(med[n], 3), "ms_min": round(min(ts), 3),
                      "ms_max": round(max(ts), 3)}
            if n in nb:
                rec[n].update(bytes=nb[n], TBps=round(nb[n] / med[n] / 1e9, 3))
        for n in ("fwd", "bwd_dst", "bwd_src"):
            rec[f"edge_{n}_over_v2_{n}"] = round(med[f"edge_{n}"] / med[f"v2_{n}"], 3)
        if not a.kernels_only:
            rec["op_over_three_kernels"] = round(
                med["op"] / (med["edge_fwd"] + med["edge_bwd_dst"] + med["edge_bwd_src"]), 3)
            rec["op_over_composed"] = round(med["op"] / med["composed"], 3)
        print(json.dumps(rec), flush=True)
        del l, g, r, ee, out, dl, dr, dee, w, da_part, grad_ins
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
