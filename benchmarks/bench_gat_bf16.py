#!/usr/bin/env python3
"""Micro-benchmark of the relation-attention kernels with bf16 storage
(csrc/kernels/gat_bf16.hip) next to the fp32 ones (gat_f32.hip) and the sum SpMM, on one
MAG240M-shaped relation (paper cites paper of ``--scale`` of the graph) in the same run.

Per (C, heads) case, timed in interleaved rounds with device events (one warm-up round, then
``--rounds`` timed ones):

    spmm / spmm_T          K.spmm over the CSR / its transpose, fp32 rows (the yardstick)
    spmm16 / spmm16_T      the same on bf16 rows
    f32_scores             the source-score GEMM z @ A the fp32 forward needs first
    f32_fwd / f32_bwd_dst / f32_bwd_src   gat_*_f32 (ss an operand)
    f32_da                 the [heads, rows] x [rows, C] GEMM of the fp32 dL/da_src
    bf16_fwd / bf16_bwd_dst / bf16_bwd_src   gat_*_bf16 (ss from the gathered row; the
                           source side also leaves the partial rows of dL/da_src)

One JSON line per case: median / min / max ms and the bytes each pass must move once
(gathered rows + ids + what it reads and writes per row; from the shapes) over the median.
Example: python benchmarks/bench_gat_bf16.py --scale 0.03 --rounds 7
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pass_bytes(nnz, rows, cols, C, H, P):
    """Bytes each pass must move, every item once (int32 ids)."""
    st = 4 * H
    nb = {}
    for tag, row in (("f32", 4 * C), ("bf16", 2 * C)):
        ss = st if tag == "f32" else 0  # the fp32 kernels gather ss_j next to z_j
        # z_j per entry; sd in, out in + out, 2 statistics out per row
        nb[f"{tag}_fwd"] = nnz * (row + ss + 4) + rows * (2 * row + 3 * st)
        # z_j per entry; g, sd, 2 statistics in, c and gsd out per row
        nb[f"{tag}_bwd_dst"] = nnz * (row + ss + 4) + rows * (row + 5 * st)
        # g_i and sd, m, 1/l, c per entry; z in, dz and gss out per source row
        nb[f"{tag}_bwd_src"] = nnz * (row + 4 * st + 4) + cols * (2 * row + st + ss)
    nb["bf16_bwd_src"] += P * 4 * C
    nb["spmm"] = nnz * (4 * C + 4) + rows * 4 * C
    nb["spmm_T"] = nnz * (4 * C + 4) + cols * 4 * C
    nb["spmm16"] = nnz * (2 * C + 4) + rows * 2 * C
    nb["spmm16_T"] = nnz * (2 * C + 4) + cols * 2 * C
    return nb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=0.03, help="fraction of MAG240M")
    ap.add_argument("--cases", default="256:4", help="comma list of C:heads")
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    from dgraph_amd import _native
    from dgraph_amd.data.mag import HETERO_SHAPES, build_relation_csrs
    from dgraph_amd.ops import kernels as K
    from dgraph_amd.ops.gat import GatPattern, _score_matrix

    if not torch.cuda.is_available():
        raise SystemExit("bench_gat_bf16.py needs a GPU")
    ops = _native.ops()
    dev = torch.device("cuda", 0)
    shape = HETERO_SHAPES["mag240m"].scaled(a.scale)
    csr = build_relation_csrs(shape, 0, 1, dev, relations=[0])[0][0]
    rows, cols, nnz = csr.num_rows, csr.num_cols, csr.nnz
    pat = GatPattern(csr.rowptr, csr.col, cols, 0)
    print(f"[gat_bf16] {shape.name} cites: rows={rows} cols={cols} nnz={nnz} "
          f"max degree={int(csr.degree().max())}", flush=True)
    f = lambda *s: torch.randn(*s, device=dev)  # noqa: E731
    for C, H in [tuple(int(t) for t in c.split(":")) for c in a.cases.split(",")]:
        z, g = f(cols, C), f(rows, C)
        z16, g16 = z.bfloat16(), g.bfloat16()
        att = f(H, C // H) / (C // H) ** 0.5
        A, a_flat = _score_matrix(att), att.reshape(-1).contiguous()
        sd = f(rows, H)
        ss = z @ A
        out, out16 = torch.zeros(rows, C, device=dev), torch.zeros(rows, C, device=dev,
                                                                  dtype=torch.bfloat16)
        gz, gz16 = torch.empty_like(z), torch.empty_like(z16)
        st = lambda n: torch.empty(n, H, device=dev)  # noqa: E731
        m, l, c, gsd, gss = st(rows), st(rows), st(rows), st(rows), st(cols)
        m16, l16, c16, gsd16, gss16 = st(rows), st(rows), st(rows), st(rows), st(cols)
        P = ops.gat_bf16_da_parts(cols, C)
        dap = torch.empty(P, C, device=dev)
        passes = {
            "spmm": lambda: K.spmm(pat.rowptr, pat.col, z, out),
            "spmm_T": lambda: K.spmm(pat.t_rowptr, pat.t_col, g, gz),
            "spmm16": lambda: K.spmm(pat.rowptr, pat.col, z16, out16),
            "spmm16_T": lambda: K.spmm(pat.t_rowptr, pat.t_col, g16, gz16),
            "f32_scores": lambda: torch.matmul(z, A),
            "f32_fwd": lambda: ops.gat_fwd_f32(pat.rowptr, pat.col, z, None, cols, ss, None, sd,
                                               out, 0.0, m, l, H, 0.2),
            "f32_bwd_dst": lambda: ops.gat_bwd_dst_f32(pat.rowptr, pat.col, z, None, cols, ss,
                                                       None, sd, m, l, g, c, gsd, H, 0.2),
            "f32_bwd_src": lambda: ops.gat_bwd_src_f32(pat.t_rowptr, pat.t_col, g, z, ss, sd, m,
                                                       l, c, a_flat, gz, gss, H, 0.2),
            "f32_da": lambda: torch.matmul(gss.t(), z),
            "bf16_fwd": lambda: ops.gat_fwd_bf16(pat.rowptr, pat.col, z16, None, cols, a_flat,
                                                 sd, out16, 0.0, m16, l16, H, 0.2),
            "bf16_bwd_dst": lambda: ops.gat_bwd_dst_bf16(pat.rowptr, pat.col, z16, None, cols,
                                                         a_flat, sd, m16, l16, g16, c16, gsd16,
                                                         H, 0.2),
            "bf16_bwd_src": lambda: ops.gat_bwd_src_bf16(pat.t_rowptr, pat.t_col, g16, z16,
                                                         a_flat, sd, m16, l16, c16, gz16, gss16,
                                                         dap, H, 0.2),
        }
        times = {n: [] for n in passes}
        for r in range(a.rounds + 1):  # round 0 warms every pass up (and orders fwd -> bwd)
            for n, fn in passes.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                s.record()
                fn()
                e.record()
                torch.cuda.synchronize()
                if r > 0:
                    times[n].append(s.elapsed_time(e))
        nb = pass_bytes(nnz, rows, cols, C, H, P)
        rec = {"bench": "gat_bf16", "shape": shape.name, "rows": rows, "nnz": nnz, "C": C,
               "heads": H, "rounds": a.rounds, "da_parts": P}
        med = {}
        for n, ts in times.items():
            med[n] = statistics.median(ts)
            rec[n] = {"ms": round(med[n], 3), "ms_min": round(min(ts), 3),
                      "ms_max": round(max(ts), 3)}
            if n in nb:
                rec[n].update(bytes=nb[n], TBps=round(nb[n] / med[n] / 1e9, 3))
        for kind in ("fwd", "bwd_dst", "bwd_src"):
            rec[f"bf16_{kind}_over_f32_{kind}"] = round(med[f"bf16_{kind}"] / med[f"f32_{kind}"], 3)
        rec["bf16_three_over_f32_three_and_gemms"] = round(
            sum(med[f"bf16_{k}"] for k in ("fwd", "bwd_dst", "bwd_src")) /
            (sum(med[f"f32_{k}"] for k in ("fwd", "bwd_dst", "bwd_src")) + med["f32_scores"] +
             med["f32_da"]), 3)
        print(json.dumps(rec), flush=True)
        del z, g, z16, g16, out, out16, gz, gz16, passes, dap


if __name__ == "__main__":
    main()
