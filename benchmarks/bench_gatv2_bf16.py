#!/usr/bin/env python3
"""Micro-benchmark of the GATv2 attention kernels with bf16 storage
(csrc/kernels/gatv2_bf16.hip) next to the fp32 ones (gatv2_f32.hip) on the default graph of
benchmarks/bench_gatv2.py, in the same run.

Per (C, heads) case, timed in interleaved rounds with device events (one warm-up round, then
``--rounds`` timed ones; ``--inner`` launches per timed window):

    f32_fwd / f32_bwd_dst / f32_bwd_src     gatv2_*_f32 (c an operand of the backward)
    bf16_fwd / bf16_bwd_dst / bf16_bwd_src  gatv2_*_bf16 (bwd_dst gathers r_j ONCE and writes c)

l | r are the column halves of one [N, 2C] buffer in both dtypes. One JSON line per case:
median / min / max ms per launch and the bytes each pass must move once (gathered rows + ids +
what it reads and writes per row; from the shapes) over the median, and the bf16 / fp32 ratio
of every kernel.
Example: python benchmarks/bench_gatv2_bf16.py --cases 256:4,64:1 --rounds 7
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SLOPE = 0.2


def pass_bytes(nnz, rows, cols, C, H, parts):
    """Bytes each pass must move, every item once (int32 ids, fp32 statistics and att)."""
    st = 4 * H
    nb = {}
    for tag, row in (("f32", 4 * C), ("bf16", 2 * C)):
        # r_j per entry; l in, out + 2 statistics out per row
        nb[f"{tag}_fwd"] = nnz * (row + 4) + rows * (2 * row + 2 * st) + 4 * C
        # r_j per entry; l, g, 3 statistics (bf16: 2 in, c out), dl out per row; da_part
        nb[f"{tag}_bwd_dst"] = nnz * (row + 4) + rows * (3 * row + 3 * st) + \
            4 * C * (1 + parts[tag])
        # l_i, g_i and 3 statistics per entry; r in, dr out per source row
        nb[f"{tag}_bwd_src"] = nnz * (2 * row + 3 * st + 4) + cols * 2 * row + 4 * C
    return nb


def make_passes(ops, pat, tag, t, att, rows, cols, C, H):
    """The three launches of one dtype over its own operands and outputs."""
    l, r, g = t["lr"][:rows, :C], t["lr"][:, C:], t["g"]
    out, dl, dr = torch.empty_like(g), torch.empty_like(g), torch.empty_like(t["lr"])[:, C:]
    m, li, c = (torch.empty(rows, H, device=g.device) for _ in range(3))
    rp, cl, trp, tcl = pat.rowptr, pat.col, pat.t_rowptr, pat.t_col
    if tag == "f32":
        P = ops.gatv2_da_parts(rows, C)
        dap = torch.empty(P, C, device=g.device)

        def fwd():
            ops.gatv2_fwd_f32(rp, cl, l, r, None, cols, att, out, 0.0, m, li, H, SLOPE)

        def dst():
            ops.gatv2_bwd_dst_f32(rp, cl, l, r, None, cols, att, m, li, g, c, dl, dap, H, SLOPE)

        def src():
            ops.gatv2_bwd_src_f32(trp, tcl, l, g, r, att, m, li, c, dr, H, SLOPE)

        fwd()  # the fp32 backward reads c = <g, out> per head
        c.copy_((g * out).view(rows, H, C // H).sum(-1))
    else:
        P = ops.gatv2_bf16_da_parts(rows, C)
        dap = torch.empty(P, C, device=g.device)

        def fwd():
            ops.gatv2_fwd_bf16(rp, cl, l, r, None, cols, att, out, m, li, H, SLOPE)

        def dst():
            ops.gatv2_bwd_dst_bf16(rp, cl, l, r, None, cols, att, m, li, g, c, dl, dap, H, SLOPE)

        def src():
            ops.gatv2_bwd_src_bf16(trp, tcl, l, g, r, att, m, li, c, dr, H, SLOPE)

    return {f"{tag}_fwd": fwd, f"{tag}_bwd_dst": dst, f"{tag}_bwd_src": src}, P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ogbn-products")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--cases", default="256:4,64:1", help="comma list of C:heads")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5, help="launches per timed window")
    ap.add_argument("--global-frac", type=float, default=0.05)
    ap.add_argument("--window", type=int, default=1 << 14)
    a = ap.parse_args()
    from dgraph_amd import _native
    from dgraph_amd.data.synthetic import SHAPES, build_partition
    from dgraph_amd.ops.gat import GatPattern

    if not torch.cuda.is_available():
        raise SystemExit("bench_gatv2_bf16.py needs a GPU")
    ops = _native.ops()
    dev = torch.device("cuda", 0)
    shape = SHAPES[a.shape] if a.scale == 1.0 else SHAPES[a.shape].scaled(a.scale)
    p = build_partition(shape, 0, 1, dev, global_frac=a.global_frac, window=a.window)
    csr = p["csr"]
    rows, cols, nnz = csr.num_rows, csr.num_cols, csr.nnz
    pat = GatPattern(csr.rowptr, csr.col, cols, 0)
    print(f"[gatv2_bf16] rows={rows} cols={cols} nnz={nnz} "
          f"max degree={int(csr.degree().max())}", flush=True)
    f = lambda *s: torch.randn(*s, device=dev)  # noqa: E731
    for C, H in [tuple(int(t) for t in c.split(":")) for c in a.cases.split(",")]:
        att = f(C) / (C // H) ** 0.5
        t32 = dict(lr=f(max(rows, cols), 2 * C), g=f(rows, C))
        t16 = {n: t.bfloat16() for n, t in t32.items()}
        passes, parts = {}, {}
        for tag, t in (("f32", t32), ("bf16", t16)):
            fns, parts[tag] = make_passes(ops, pat, tag, t, att, rows, cols, C, H)
            passes.update(fns)
        times = {n: [] for n in passes}
        for r in range(a.rounds + 1):  # round 0 warms every pass up (and orders fwd -> bwd)
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
        nb = pass_bytes(nnz, rows, cols, C, H, parts)
        rec = {"bench": "gatv2_bf16", "shape": shape.name, "rows": rows, "nnz": nnz, "C": C,
               "heads": H, "rounds": a.rounds, "inner": a.inner}
        med = {}
        for n, ts in times.items():
            med[n] = statistics.median(ts)
            rec[n] = {"ms": round(med[n], 3), "ms_min": round(min(ts), 3),
                      "ms_max": round(max(ts), 3), "bytes": nb[n],
                      "TBps": round(nb[n] / med[n] / 1e9, 3)}
        kinds = ("fwd", "bwd_dst", "bwd_src")
        for kind in kinds:
            rec[f"bf16_{kind}_over_f32_{kind}"] = round(med[f"bf16_{kind}"] / med[f"f32_{kind}"], 3)
        rec["bf16_three_over_f32_three"] = round(
            sum(med[f"bf16_{k}"] for k in kinds) / sum(med[f"f32_{k}"] for k in kinds), 3)
        print(json.dumps(rec), flush=True)
        del t32, t16, passes


if __name__ == "__main__":
    main()
