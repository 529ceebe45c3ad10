#!/usr/bin/env python3
"""Micro-benchmark of the fused GATv2 attention kernels (csrc/kernels/gatv2_f32.hip) next to
the fp32 sum SpMM, the additive-attention forward (gat_f32.hip) and the three dot-product
attention kernels (dot_attn_f32.hip) on the same pattern in the same run.

Per (C, heads) case on the default graph of benchmarks/bench_spmm.py, timed in interleaved
rounds with device events (one warm-up round, then ``--rounds`` timed ones):

    spmm      K.spmm over the CSR, fp32, width C                (the yardstick, one gather)
    spmm_T    K.spmm over the transposed CSR                    (the yardstick, backward)
    gat_fwd   gat_fwd_f32: scalar statistics pass + one gather of z
    dot_fwd / dot_bwd_dst / dot_bwd_src   the dot-product kernels (2 gathered rows per entry)
    v2_fwd    gatv2_fwd_f32: one pass, gathers r_j once (score and message)
    v2_bwd_dst   gatv2_bwd_dst_f32: gathers r_j; dl and the partial rows of da
    v2_bwd_src   gatv2_bwd_src_f32 over the transpose: gathers l_i, g_i and 3 statistics
    op        ops.gatv2_attention forward + backward (xd | xs the halves of one [N, 2C]
              buffer; includes c = <g, out> and the column sum of da_part)

One JSON line per case: median / min / max ms, the bytes each pass must move once (gathered
rows + ids + the rows it reads and writes per output row; computed from the shapes below)
over the median time, and each GATv2 kernel's time over its dot-product sibling and over the
SpMM of its direction.
Example: python benchmarks/bench_gatv2.py --rounds 7
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pass_bytes(nnz, rows, cols, C, H, isize, P):
    """Bytes each pass must move, every item once (fp32)."""
    row, st = 4 * C, 4 * H
    return {
        "spmm": nnz * (row + isize) + rows * row,
        "spmm_T": nnz * (row + isize) + cols * row,
        # z_j and ss_j per entry; sd in, out + 2 statistics out per row
        "gat_fwd": nnz * (row + st + isize) + rows * (row + 3 * st),
        # k_j and v_j per entry; q in, out + 2 statistics out per row
        "dot_fwd": nnz * (2 * row + isize) + rows * (2 * row + 2 * st),
        # k_j and v_j per entry; q, g, 3 statistics in, dq out per row
        "dot_bwd_dst": nnz * (2 * row + isize) + rows * (3 * row + 3 * st),
        # q_i, g_i and 3 statistics per entry; k, v in, dk, dv out per source row
        "dot_bwd_src": nnz * (2 * row + 3 * st + isize) + cols * 4 * row,
        # r_j per entry; l in, out + 2 statistics out per row
        "v2_fwd": nnz * (row + isize) + rows * (2 * row + 2 * st),
        # r_j per entry; l, g, 3 statistics in, dl out per row; da_part out
        "v2_bwd_dst": nnz * (row + isize) + rows * (3 * row + 3 * st) + P * row,
        # l_i, g_i and 3 statistics per entry; r in, dr out per source row
        "v2_bwd_src": nnz * (2 * row + 3 * st + isize) + cols * 2 * row,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ogbn-products")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--cases", default="128:4,256:4", help="comma list of C:heads")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--global-frac", type=float, default=0.05)
    ap.add_argument("--window", type=int, default=1 << 14)
    a = ap.parse_args()
    from dgraph_amd import _native
    from dgraph_amd.data.synthetic import SHAPES, build_partition
    from dgraph_amd.ops import kernels as K
    from dgraph_amd.ops.gat import GatPattern
    from dgraph_amd.ops.gatv2 import gatv2_attention

    if not torch.cuda.is_available():
        raise SystemExit("bench_gatv2.py needs a GPU")
    ops = _native.ops()
    dev = torch.device("cuda", 0)
    shape = SHAPES[a.shape] if a.scale == 1.0 else SHAPES[a.shape].scaled(a.scale)
    p = build_partition(shape, 0, 1, dev, global_frac=a.global_frac, window=a.window)
    csr = p["csr"]
    rows, cols, nnz = csr.num_rows, csr.num_cols, csr.nnz
    pat = GatPattern(csr.rowptr, csr.col, cols, 0)
    print(f"[gatv2] rows={rows} cols={cols} nnz={nnz} max degree={int(csr.degree().max())}",
          flush=True)
    f = lambda *s: torch.randn(*s, device=dev)  # noqa: E731
    for C, H in [tuple(int(t) for t in c.split(":")) for c in a.cases.split(",")]:
        scale = 1.0 / math.sqrt(C // H)
        q, g = f(rows, C), f(rows, C)  # q doubles as the GATv2 destination rows l
        kv = f(cols, 2 * C)
        k, v = kv[:, :C], kv[:, C:]    # k doubles as the GATv2 source rows r
        att = f(C) / math.sqrt(C // H)
        ss, sd = f(cols, H), f(rows, H)
        z = f(cols, C)
        out, dq = torch.empty(rows, C, device=dev), torch.empty(rows, C, device=dev)
        dk, dv = torch.empty(cols, C, device=dev), torch.empty(cols, C, device=dev)
        m, l = torch.empty(rows, H, device=dev), torch.empty(rows, H, device=dev)
        m2, l2 = torch.empty_like(m), torch.empty_like(l)
        gm, gl = torch.empty_like(m), torch.empty_like(l)
        c, c2 = torch.empty(rows, H, device=dev), torch.empty(rows, H, device=dev)
        P = ops.gatv2_da_parts(rows, C)
        da_part = torch.empty(P, C, device=dev)
        lrg = torch.cat([q, k], 1).requires_grad_() if rows == cols else None
        attg = att.clone().requires_grad_()

        def dot_fwd():
            ops.dot_attn_fwd_f32(pat.rowptr, pat.col, q, k, v, None, None, cols, out, 0.0, m, l,
                                 H, scale)

        def dot_bwd_dst():
            ops.dot_attn_bwd_dst_f32(pat.rowptr, pat.col, q, k, v, None, None, cols, m, l, g, c,
                                     dq, H, scale)

        def dot_bwd_src():
            ops.dot_attn_bwd_src_f32(pat.t_rowptr, pat.t_col, q, g, k, v, m, l, c, dk, dv, H,
                                     scale)

        def v2_fwd():
            ops.gatv2_fwd_f32(pat.rowptr, pat.col, q, k, None, cols, att, out, 0.0, m2, l2, H,
                              0.2)

        def v2_bwd_dst():
            ops.gatv2_bwd_dst_f32(pat.rowptr, pat.col, q, k, None, cols, att, m2, l2, g, c2, dq,
                                  da_part, H, 0.2)

        def v2_bwd_src():
            ops.gatv2_bwd_src_f32(pat.t_rowptr, pat.t_col, q, g, k, att, m2, l2, c2, dk, H, 0.2)

        def op():
            lrg.grad = attg.grad = None
            gatv2_attention(lrg[:, :C], lrg[:, C:], attg, pat, heads=H).backward(g)

        passes = {
            "spmm": lambda: K.spmm(pat.rowptr, pat.col, z, out),
            "spmm_T": lambda: K.spmm(pat.t_rowptr, pat.t_col, g, dk),
            "gat_fwd": lambda: ops.gat_fwd_f32(pat.rowptr, pat.col, z, None, cols, ss, None, sd,
                                               out, 0.0, gm, gl, H, 0.2),
            "dot_fwd": dot_fwd,
            "v2_fwd": v2_fwd,
        }
        # the backward kernels read their forward's statistics and c = <g, out> per head
        dot_fwd()
        c.copy_((g * out).view(rows, H, C // H).sum(-1))
        v2_fwd()
        c2.copy_((g * out).view(rows, H, C // H).sum(-1))
        passes.update(dot_bwd_dst=dot_bwd_dst, v2_bwd_dst=v2_bwd_dst, dot_bwd_src=dot_bwd_src,
                      v2_bwd_src=v2_bwd_src)
        if lrg is not None:
            passes["op"] = op
        times = {n: [] for n in passes}
        for r in range(a.rounds + 1):  # round 0 warms every pass up
            for n, fn in passes.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                s.record()
                fn()
                e.record()
                torch.cuda.synchronize()
                if r > 0:
                    times[n].append(s.elapsed_time(e))
        nb = pass_bytes(nnz, rows, cols, C, H, pat.col.element_size(), P)
        rec = {"bench": "gatv2", "shape": shape.name, "rows": rows, "nnz": nnz, "C": C,
               "heads": H, "rounds": a.rounds, "da_parts": P}
        med = {}
        for n, ts in times.items():
            med[n] = statistics.median(ts)
            rec[n] = {"ms": round(med[n], 3), "ms_min": round(min(ts), 3),
                      "ms_max": round(max(ts), 3)}
            if n in nb:
                rec[n].update(bytes=nb[n], TBps=round(nb[n] / med[n] / 1e9, 3))
        for kind in ("fwd", "bwd_dst", "bwd_src"):
            rec[f"v2_{kind}_over_dot_{kind}"] = round(med[f"v2_{kind}"] / med[f"dot_{kind}"], 3)
        rec["v2_fwd_over_spmm"] = round(med["v2_fwd"] / med["spmm"], 3)
        rec["v2_fwd_over_gat_fwd"] = round(med["v2_fwd"] / med["gat_fwd"], 3)
        rec["v2_bwd_dst_over_spmm"] = round(med["v2_bwd_dst"] / med["spmm"], 3)
        rec["v2_bwd_src_over_two_spmm_T"] = round(med["v2_bwd_src"] / (2 * med["spmm_T"]), 3)
        if "op" in med:
            rec["op_over_three_kernels"] = round(
                med["op"] / (med["v2_fwd"] + med["v2_bwd_dst"] + med["v2_bwd_src"]), 3)
        print(json.dumps(rec), flush=True)
        del q, g, z, kv, k, v, out, dq, dk, dv, lrg, passes, da_part


if __name__ == "__main__":
    main()
