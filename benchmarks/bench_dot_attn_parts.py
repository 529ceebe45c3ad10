#!/usr/bin/env python3
"""Micro-benchmark of the carry-in forward of the dot-product attention kernels
(``dot_attn_fwd_carry_f32``, csrc/kernels/dot_attn_f32.hip) and of the overlapped halo op
(``ops.dot_attn.dot_attention_halo``) on one rank's real partition: rank ``--rank`` of a
``--world``-way partition of the graph, built alone (data/synthetic.py ``rehearse``), so the
interior / halo split of the pattern and the send plan have their real shapes.

Per (C, heads) case, timed in interleaved rounds with device events (one warm-up round, then
``--rounds`` timed ones), medians reported:

(a) what the split itself costs, kernels only:
    fwd_two_source   dot_attn_fwd_f32 over the merged pattern, local and halo rows as two sources
    fwd_interior     dot_attn_fwd_f32 over the interior pattern
    fwd_halo_carry   dot_attn_fwd_carry_f32 over the halo pattern, on the interior pass's state
    with the bytes each must move once, computed from the shapes (the split reads q twice for
    the rows that have halo entries and rewrites their out and statistics).

(b) the op, forward + backward, the exchange included, on the LOOPBACK transport
    (comm/alltoallv.py: one process, the rank receives a copy of its own send rows):
    op_sync      the synchronous exchange (pack, all-to-all-v, wait), then ops.dot_attention
                 with two sources; its adjoint exchange in backward
    op_overlap   ops.dot_attention_halo: interior forward under the exchange, halo carry after;
                 reverse exchange under dq and the local dk / dv
    once with the link model off (the loopback copy completes at once: nothing to hide, the
    difference is what the split costs) and once with every exchange held for latency +
    largest per-peer message / ``--link-gbps`` on a side stream. The second is a MODEL of a
    link run on one GPU, not a multi-GPU measurement.

One JSON line per case. Example: python benchmarks/bench_dot_attn_parts.py --rounds 7
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pass_bytes(nnz_i, nnz_h, rows, rows_h, C, H, isize):
    """Bytes each forward must move, every item once (fp32): k_j and v_j per entry and its
    id; q in, out + 2 statistics out per row; the carry pass reads q, out and both statistics
    and writes out and both statistics for the ``rows_h`` rows that have halo entries, and
    the row pointer for all."""
    row, st = 4 * C, 4 * H
    return {
        "fwd_two_source": (nnz_i + nnz_h) * (2 * row + isize) + rows * (2 * row + 2 * st),
        "fwd_interior": nnz_i * (2 * row + isize) + rows * (2 * row + 2 * st),
        "fwd_halo_carry": nnz_h * (2 * row + isize) + rows_h * (3 * row + 4 * st) + rows * 8,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ogbn-products")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rank", type=int, default=1)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--cases", default="256:4,128:1", help="comma list of C:heads")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--link-gbps", type=float, default=153.0,
                    help="rate of the modelled point-to-point link (GB/s per direction)")
    ap.add_argument("--global-frac", type=float, default=0.05)
    ap.add_argument("--window", type=int, default=1 << 14)
    a = ap.parse_args()
    from dgraph_amd import _native
    from dgraph_amd.comm import alltoallv as A
    from dgraph_amd.data.synthetic import SHAPES, build_partition
    from dgraph_amd.ops.dot_attn import HaloPlan, dot_attention, dot_attention_halo
    from dgraph_amd.ops.gat import GatPattern

    if not torch.cuda.is_available():
        raise SystemExit("bench_dot_attn_parts.py needs a GPU")
    ops = _native.ops()
    dev = torch.device("cuda", 0)
    shape = SHAPES[a.shape] if a.scale == 1.0 else SHAPES[a.shape].scaled(a.scale)
    p = build_partition(shape, a.rank, a.world, dev, global_frac=a.global_frac,
                        window=a.window, rehearse=True)
    csr, Ls, Hn = p["csr"], p["L"], p["H"]
    rows = csr.num_rows
    pat = GatPattern(csr.rowptr, csr.col, Ls, Hn)
    inner, outer = pat.split()
    nnz_i, nnz_h = inner.col.numel(), outer.col.numel()
    rows_h = int(((outer.rowptr[1:] - outer.rowptr[:-1]) > 0).sum())
    a2a = A.AllToAllV(p["send_splits"], p["recv_splits"])
    plan = HaloPlan(a2a, p["send_local_idx"], Ls)
    print(f"[dot_attn_parts] rank {a.rank} of {a.world}: rows={rows} local sources={Ls} "
          f"halo rows={Hn} send rows={a2a.total_send} interior nnz={nnz_i} halo nnz={nnz_h} "
          f"rows with halo entries={rows_h}", flush=True)
    f = lambda *s: torch.randn(*s, device=dev)  # noqa: E731
    for C, H in [tuple(int(t) for t in c.split(":")) for c in a.cases.split(",")]:
        scale = 1.0 / math.sqrt(C // H)
        q, g = f(rows, C), f(rows, C)
        kv, kvh = f(Ls, 2 * C), f(Hn, 2 * C)
        k, v, kh, vh = kv[:, :C], kv[:, C:], kvh[:, :C], kvh[:, C:]
        out = torch.empty(rows, C, device=dev)
        m, l = torch.empty(rows, H, device=dev), torch.empty(rows, H, device=dev)
        out2, m2, l2 = torch.empty_like(out), torch.empty_like(m), torch.empty_like(l)
        qg, kvg = q.clone().requires_grad_(), kv.clone().requires_grad_()

        def fwd_two_source():
            ops.dot_attn_fwd_f32(pat.rowptr, pat.col, q, k, v, kh, vh, Ls, out, 0.0, m, l, H,
                                 scale)

        def fwd_interior():
            ops.dot_attn_fwd_f32(inner.rowptr, inner.col, q, k, v, None, None, Ls, out2, 0.0,
                                 m2, l2, H, scale)

        def fwd_halo_carry():  # (on the interior pass's state; run after it in every round)
            ops.dot_attn_fwd_carry_f32(outer.rowptr, outer.col, q, kh, vh, None, None, Hn, out2,
                                       m2, l2, H, scale)

        def op_sync():
            qg.grad = kvg.grad = None
            halo = plan.exchange(kvg)
            dot_attention(qg, kvg[:, :C], kvg[:, C:], pat, halo[:, :C], halo[:, C:],
                          heads=H).backward(g)

        def op_overlap():
            qg.grad = kvg.grad = None
            dot_attention_halo(qg, kvg, pat, plan, heads=H).backward(g)

        def timed(passes, rounds):
            times = {n: [] for n in passes}
            for r in range(rounds + 1):  # round 0 warms every pass up
                for n, fn in passes.items():
                    s, e = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                    torch.cuda.synchronize()
                    s.record()
                    fn()
                    e.record()
                    torch.cuda.synchronize()
                    if r > 0:
                        times[n].append(s.elapsed_time(e))
            return times

        rec = {"bench": "dot_attn_parts", "shape": shape.name, "rank": a.rank,
               "world": a.world, "rows": rows, "interior_nnz": nnz_i, "halo_nnz": nnz_h,
               "halo_rows": Hn, "send_rows": a2a.total_send, "C": C, "heads": H,
               "rounds": a.rounds}
        # (a) the kernels
        times = timed({"fwd_two_source": fwd_two_source, "fwd_interior": fwd_interior,
                       "fwd_halo_carry": fwd_halo_carry}, a.rounds)
        nb = pass_bytes(nnz_i, nnz_h, rows, rows_h, C, H, pat.col.element_size())
        med = {}
        for n, ts in times.items():
            med[n] = statistics.median(ts)
            rec[n] = {"ms": round(med[n], 3), "ms_min": round(min(ts), 3),
                      "ms_max": round(max(ts), 3), "bytes": nb[n],
                      "TBps": round(nb[n] / med[n] / 1e9, 3)}
        rec["split_over_two_source"] = round(
            (med["fwd_interior"] + med["fwd_halo_carry"]) / med["fwd_two_source"], 3)
        rec["split_max_abs_diff"] = float((out - out2).abs().max())
        # (b) the op on the loopback transport: link model off, then on
        row_bytes = 2 * C * 4
        for label, gbps in (("link_off", 0.0), ("link_model", a.link_gbps)):
            A.LOOPBACK_LINK_GBPS = gbps
            times = timed({"op_sync": op_sync, "op_overlap": op_overlap}, a.rounds)
            ms = {n: statistics.median(ts) for n, ts in times.items()}
            rec[label] = {
                "model_not_multi_gpu": True, "link_gbps": gbps,
                "modelled_exchange_us_fwd": round(a2a.link_us(row_bytes, gbps), 1),
                "modelled_exchange_us_bwd": round(a2a.reversed().link_us(row_bytes, gbps), 1),
                "op_sync_ms": round(ms["op_sync"], 3),
                "op_sync_ms_min_max": [round(min(times["op_sync"]), 3),
                                       round(max(times["op_sync"]), 3)],
                "op_overlap_ms": round(ms["op_overlap"], 3),
                "op_overlap_ms_min_max": [round(min(times["op_overlap"]), 3),
                                          round(max(times["op_overlap"]), 3)],
                "overlap_over_sync": round(ms["op_overlap"] / ms["op_sync"], 3)}
        A.LOOPBACK_LINK_GBPS = 0.0
        print(json.dumps(rec), flush=True)
        del q, g, kv, kvh, k, v, kh, vh, out, m, l, out2, m2, l2, qg, kvg


if __name__ == "__main__":
    main()
