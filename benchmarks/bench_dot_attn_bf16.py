#!/usr/bin/env python3
"""Micro-benchmark of the dot-product attention kernels with bf16 storage
(csrc/kernels/dot_attn_bf16.hip) next to the fp32 ones (dot_attn_f32.h) on the default graph
of benchmarks/bench_dot_attn.py, in the same run.

Per (C, heads) case, timed in interleaved rounds with device events (one warm-up round, then
``--rounds`` timed ones; ``--inner`` launches per timed window):

    f32_fwd / f32_bwd_dst / f32_bwd_src     dot_attn_*_f32 (c an operand of the backward)
    bf16_fwd / bf16_bwd_dst / bf16_bwd_src  dot_attn_*_bf16 (bwd_dst gathers k_j and v_j twice
                                            and writes c)

k | v are the column halves of one [N, 2C] buffer in both dtypes. One JSON line per case:
median / min / max ms per launch and the bytes each pass must move once (gathered rows + ids +
what it reads and writes per row; from the shapes) over the median. ``bf16_bwd_dst`` counts its
gathered rows ONCE (``bytes``) and states ``bytes_two_pass`` next to it: a rate above what the
memory system delivers on ``bytes`` says the second pass was not served from cache.
Example: python benchmarks/bench_dot_attn_bf16.py --cases 256:4,64:1 --rounds 7
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pass_bytes(nnz, rows, cols, C, H):
    """Bytes each pass must move, every item once (int32 ids, fp32 statistics)."""
    st = 4 * H
    nb = {}
    for tag, row in (("f32", 4 * C), ("bf16", 2 * C)):
        # k_j and v_j per entry; q in, out + 2 statistics out per row
        nb[f"{tag}_fwd"] = nnz * (2 * row + 4) + rows * (2 * row + 2 * st)
        # k_j and v_j per entry; q, g, 3 statistics (bf16: 2 in, c out), dq out per row
        nb[f"{tag}_bwd_dst"] = nnz * (2 * row + 4) + rows * (3 * row + 3 * st)
        # q_i, g_i and 3 statistics per entry; k, v in, dk, dv out per source row
        nb[f"{tag}_bwd_src"] = nnz * (2 * row + 3 * st + 4) + cols * 4 * row
    nb["bf16_bwd_dst_two_pass"] = nb["bf16_bwd_dst"] + nnz * (4 * C + 4)
    return nb


def make_passes(ops, pat, tag, t, rows, cols, C, H, scale):
    """The three launches of one dtype over its own operands and outputs."""
    q, g, k, v = t["q"], t["g"], t["kv"][:, :C], t["kv"][:, C:]
    out, dq, dkv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(t["kv"])
    dk, dv = dkv[:, :C], dkv[:, C:]
    m, l, c = (torch.empty(rows, H, device=q.device) for _ in range(3))
    rp, cl, trp, tcl = pat.rowptr, pat.col, pat.t_rowptr, pat.t_col
    if tag == "f32":
        def fwd():
            ops.dot_attn_fwd_f32(rp, cl, q, k, v, None, None, cols, out, 0.0, m, l, H, scale)

        def dst():
            ops.dot_attn_bwd_dst_f32(rp, cl, q, k, v, None, None, cols, m, l, g, c, dq, H, scale)

        def src():
            ops.dot_attn_bwd_src_f32(trp, tcl, q, g, k, v, m, l, c, dk, dv, H, scale)

        fwd()  # the fp32 backward reads c = <g, out> per head
        c.copy_((g * out).view(rows, H, C // H).sum(-1))
    else:
        def fwd():
            ops.dot_attn_fwd_bf16(rp, cl, q, k, v, None, None, cols, out, m, l, H, scale)

        def dst():
            ops.dot_attn_bwd_dst_bf16(rp, cl, q, k, v, None, None, cols, m, l, g, c, dq, H, scale)

        def src():
            ops.dot_attn_bwd_src_bf16(trp, tcl, q, g, k, v, m, l, c, dk, dv, H, scale)

    return {f"{tag}_fwd": fwd, f"{tag}_bwd_dst": dst, f"{tag}_bwd_src": src}


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
        raise SystemExit("bench_dot_attn_bf16.py needs a GPU")
    ops = _native.ops()
    dev = torch.device("cuda", 0)
    shape = SHAPES[a.shape] if a.scale == 1.0 else SHAPES[a.shape].scaled(a.scale)
    p = build_partition(shape, 0, 1, dev, global_frac=a.global_frac, window=a.window)
    csr = p["csr"]
    rows, cols, nnz = csr.num_rows, csr.num_cols, csr.nnz
    pat = GatPattern(csr.rowptr, csr.col, cols, 0)
    print(f"[dot_attn_bf16] rows={rows} cols={cols} nnz={nnz} "
          f"max degree={int(csr.degree().max())}", flush=True)
    f = lambda *s: torch.randn(*s, device=dev)  # noqa: E731
    for C, H in [tuple(int(t) for t in c.split(":")) for c in a.cases.split(",")]:
        scale = 1.0 / math.sqrt(C // H)
        t32 = dict(q=f(rows, C), g=f(rows, C), kv=f(cols, 2 * C))
        t16 = {n: t.bfloat16() for n, t in t32.items()}
        passes = {}
        for tag, t in (("f32", t32), ("bf16", t16)):
            passes.update(make_passes(ops, pat, tag, t, rows, cols, C, H, scale))
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
        nb = pass_bytes(nnz, rows, cols, C, H)
        rec = {"bench": "dot_attn_bf16", "shape": shape.name, "rows": rows, "nnz": nnz, "C": C,
               "heads": H, "rounds": a.rounds, "inner": a.inner}
        med = {}
        for n, ts in times.items():
            med[n] = statistics.median(ts)
            rec[n] = {"ms": round(med[n], 3), "ms_min": round(min(ts), 3),
                      "ms_max": round(max(ts), 3), "bytes": nb[n],
                      "TBps": round(nb[n] / med[n] / 1e9, 3)}
        two = nb["bf16_bwd_dst_two_pass"]
        rec["bf16_bwd_dst"].update(bytes_two_pass=two,
                                   TBps_two_pass=round(two / med["bf16_bwd_dst"] / 1e9, 3))
        kinds = ("fwd", "bwd_dst", "bwd_src")
        for kind in kinds:
            rec[f"bf16_{kind}_over_f32_{kind}"] = round(med[f"bf16_{kind}"] / med[f"f32_{kind}"], 3)
        rec["bf16_three_over_f32_three"] = round(
            sum(med[f"bf16_{k}"] for k in kinds) / sum(med[f"f32_{k}"] for k in kinds), 3)
        print(json.dumps(rec), flush=True)
        del t32, t16, passes


if __name__ == "__main__":
    main()
