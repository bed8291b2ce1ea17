"""Idle time at the decode loop's host polls, from a rocprofv3 kernel trace of one headline generate.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python bench.py --gpus 1 --steps 2 --warmup 1
    python tools/poll_gap_report.py DIR [--steps 1023] [--kernels-per-step 19]

Per chain (= hardware queue that runs decode steps) and per batch (= from one dec_init_kernel to the next) the kernels are
numbered in start order: kernel i after the init kernel belongs to step i // K at position i % K (K = 19 in the headless greedy
step: per layer self-attention, cross-attention, feed-forward; then lm_head).  The gap after the last kernel of step p - 1 is a POLL
gap when p is a poll point of t5_api.hip's decode_loop (16, 32, 64, 96, 128, then every 64), a GRAPH gap at the other multiples of
the graph length, and a step gap elsewhere.  Reported: the poll gaps' sum per batch and chain, the medians of the three classes,
and the cross-attention kernel's mean duration per (layer, chain).
"""
from __future__ import annotations

import argparse
import csv
import statistics
import sys
from collections import defaultdict
from pathlib import Path


def poll_points(steps: int) -> list[int]:
    pts, p = [], 0
    while p < steps:
        p += 16 if p < 32 else (32 if p < 128 else 64)
        if p < steps:
            pts.append(p)
    return pts


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--steps", type=int, default=1023)
    ap.add_argument("--kernels-per-step", type=int, default=19)
    ap.add_argument("--graph-steps", type=int, default=8)
    args = ap.parse_args()
    files = sorted(Path(args.dir).rglob("*kernel_trace.csv"))
    if not files:
        print(f"no *kernel_trace.csv under {args.dir}", file=sys.stderr)
        return 2
    K, U = args.kernels_per_step, args.graph_steps
    polls = set(poll_points(args.steps))
    by_queue = defaultdict(list)
    with open(files[0], newline="") as f:
        for r in csv.DictReader(f):
            by_queue[r["Queue_Id"]].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    print(f"trace: {files[0]}  poll points per batch: {len(polls)}  ({sorted(polls)[:6]} ...)")
    chain = 0
    for q in sorted(by_queue):
        ks = sorted(by_queue[q])
        starts = [i for i, k in enumerate(ks) if "dec_init_kernel" in k[2]]
        print(f"queue {q}: {len(ks)} kernels, {len(starts)} decode inits")
        if not starts:
            continue
        batches = []
        for bi, i0 in enumerate(starts):
            i1 = starts[bi + 1] if bi + 1 < len(starts) else len(ks)
            body = [k for k in ks[i0 + 1:i1] if "dec_" in k[2]][: args.steps * K]
            if len(body) == args.steps * K:
                batches.append(body)
        if not batches:
            continue
        print(f"chain {chain} (queue {q}): {len(batches)} whole batches of {args.steps} steps x {K} kernels")
        cross = defaultdict(list)
        for bi, body in enumerate(batches):
            gaps = {"poll": [], "graph": [], "step": [], "kernel": []}
            for i in range(1, len(body)):
                gap = (body[i][0] - body[i - 1][1]) / 1e3
                step, pos = divmod(i, K)
                kind = "kernel" if pos else ("poll" if step in polls else ("graph" if step % U == 0 else "step"))
                gaps[kind].append(gap)
            for i, k in enumerate(body):
                pos = i % K
                if pos < K - 1 and pos % 3 == 1:
                    cross[pos // 3].append((k[1] - k[0]) / 1e3)
            med = {k: (statistics.median(v) if v else float("nan")) for k, v in gaps.items()}
            span = (body[-1][1] - body[0][0]) / 1e6
            excess = sum(gaps["poll"]) - len(gaps["poll"]) * med["graph"]      # what the polls add to as many plain graph boundaries
            print(f"  batch {bi}: decode span {span:8.2f} ms | poll gaps n={len(gaps['poll'])} sum {sum(gaps['poll']):8.1f} us "
                  f"median {med['poll']:6.1f} max {max(gaps['poll'], default=0):6.1f} excess {excess:7.1f} | graph-boundary median {med['graph']:5.2f} us "
                  f"(sum {sum(gaps['graph']):7.1f}) | step-boundary median {med['step']:5.2f} us | kernel-to-kernel median {med['kernel']:5.2f} us")
        print("  cross-attention mean us by layer: " + "  ".join(f"L{l} {statistics.mean(v):6.2f}" for l, v in sorted(cross.items())))
        chain += 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
