#!/usr/bin/env python3
"""Time of the frame-level piano-roll scores and of the TP / FN / FP error notes of one decoded batch: the device path
(music2midi_amd.scoring.frame_counts / error_notes, csrc/frame_roll.hip) against its definition on the host on the same ids
(music2midi_amd.frame_metrics) and against scoring.chroma_counts, the sibling kernel that walks the same notes.

    python tools/frame_metrics_bench.py [--runs 30] [--host-reps 3] [--corrupt 0.05] [--limit 300]

The shapes of tools/note_metrics_bench.py: 32 rows x 1 023 ids with 250-note labels over 10 s, 128 rows x 346 ids with 90-note
labels over 3 s, and one recording of 80 segments x 1 023 ids, ONE timeline (sequential mode).  The ids are the labels' own tokens
with ``--corrupt`` of the positions replaced by random ids, the tokens' log-probabilities are -Exp(0.12).  Every shape is measured
in a child process of its own under a time limit of ``--limit`` seconds; the first one that fails ends the run.  After 5 warm calls,
medians over ``--runs`` with the quartiles:
  counts_kernel_ms       K = 1 and K = 16: the time between two events around the counts launch alone (notes, labels, thresholds
                         already on the device)
  counts_call_ms         the host clock around a whole frame_counts call (detokenise, label upload, launch, copy of the counts)
  notes_kernel_ms        the two launches of error_notes (full roll), workspace and outputs allocated before
  notes_call_ms          the host clock around error_notes(...).to_numpy()
  chroma_kernel_ms, chroma_call_ms    scoring.chroma_counts on the same ids in the same run, and the ratios to it
  host_counts_ms, host_notes_ms       the numpy definition on this machine's CPUs, median of ``--host-reps`` passes (K = 1)
The integers and the notes of the two paths must be equal.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import copy
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SHAPES = [  # rows, ids per row, label notes per row, seconds per row
    dict(rows=32, length=1023, notes=250, seconds=10.0),
    dict(rows=128, length=346, notes=90, seconds=3.0),
    dict(rows=80, length=1023, notes=250, seconds=3.0, sequential=True),      # one recording of 240 s
]
SWEEP = [0.06 * k for k in range(16)]


def _stats(times) -> dict:
    q = statistics.quantiles(times, n=4)
    return {"median": statistics.median(times), "q1": q[0], "q3": q[2]}


def measure(shape: dict, args) -> dict:
    import numpy as np
    import torch
    from music2midi_amd import confidence, frame_metrics, native, scoring
    from music2midi_amd.config import DEFAULT_CONFIG, load_config
    from music2midi_amd.tokenizer import EOS, ONSET, PAD, MidiTokenizer

    native.require_gpu()
    tok = MidiTokenizer(load_config(copy.deepcopy(DEFAULT_CONFIG)))
    R, L, n, span = shape["rows"], shape["length"], shape["notes"], shape["seconds"]
    rng = np.random.default_rng(R)
    labels = []
    for _ in range(R):
        dur = rng.uniform(0.05, 1.0, n)
        start = rng.uniform(0.0, span - dur)
        labels.append(np.stack([start, start + dur, rng.integers(40, 80, n), np.full(n, 80.0)], axis=1))
    ids = np.full((R, L), PAD, dtype=np.int64)
    for r, notes in enumerate(labels):
        row = tok._tokenize(notes).numpy()[:L]
        ids[r, :len(row)] = row
    repl = rng.integers(0, 400, ids.shape)
    repl[repl == EOS] = ONSET
    ids = np.where(rng.random(ids.shape) < args.corrupt, repl, ids)
    lp = (-rng.exponential(0.12, ids.shape)).astype(np.float32)
    ids_dev, lp_dev = torch.from_numpy(ids).cuda(), torch.from_numpy(lp).cuda()
    sequential = bool(shape.get("sequential"))
    mode = dict(mode="sequential", duration_per_batch=span) if sequential else {}
    if sequential:                                              # row r is segment r: its labels start at r * span seconds
        labels = np.concatenate([notes + [r * span, r * span, 0, 0] for r, notes in enumerate(labels)])
    timelines = [labels] if sequential else labels

    def wall(call):
        times = []
        for _ in range(args.runs):
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            call()                                              # returns after the result is on the host
            times.append((time.perf_counter() - w0) * 1e3)
        return _stats(times)

    def events(enqueue):
        times = []
        for _ in range(args.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            enqueue()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        return _stats(times)

    packed, offsets, label_frames = scoring._pack_labels(timelines)
    lab, off = torch.from_numpy(packed).cuda(), torch.from_numpy(offsets).cuda()
    dn = scoring.detokenize_scored(tok, ids_dev, lp_dev, **mode)
    frame_cap = scoring._frame_cap(tok, dn, None, label_frames, "frame_metrics_bench")
    res = {"rows": R, "ids_per_row": L, "label_notes": n, "sequential": sequential, "runs": args.runs, "frame_cap": frame_cap,
           "decoded_notes": int(dn.counts.sum()), "counts": []}

    chroma = lambda: scoring.chroma_counts(tok, ids_dev, labels, **mode)
    for _ in range(5):
        chroma()
    res["chroma_kernel_ms"] = events(lambda: scoring._enqueue_counts(dn, lab, off, frame_cap))
    res["chroma_call_ms"] = wall(chroma)

    for thresholds in ([0.0], SWEEP):
        count = lambda th=thresholds: scoring.frame_counts(tok, ids_dev, labels, token_logprobs=lp_dev, thresholds=th, **mode)
        for _ in range(5):
            got = count()
        thr = torch.from_numpy(scoring.threshold_logprobs(thresholds, True)).cuda()
        case = {"thresholds": len(thresholds), "counts_kernel_ms": events(lambda: scoring._enqueue_frame_counts(dn, lab, off, thr, frame_cap)),
                "counts_call_ms": wall(count), "tp": got.tp.sum(axis=0).tolist(), "fn": got.fn.sum(axis=0).tolist(),
                "fp": got.fp.sum(axis=0).tolist(), "f1": got.f1.tolist(), "melody_f1": got.melody_f1.tolist()}
        case["kernel_over_chroma_kernel"] = case["counts_kernel_ms"]["median"] / res["chroma_kernel_ms"]["median"]
        case["call_over_chroma_call"] = case["counts_call_ms"]["median"] / res["chroma_call_ms"]["median"]
        if len(thresholds) == 1 and args.host_reps > 0:
            host = []
            for _ in range(args.host_reps):
                h0 = time.perf_counter()
                kept, _ = confidence.decode_with_confidence(tok, ids, lp, min_confidence=0.0, **mode)
                want = np.asarray([frame_metrics.frame_counts(l, d) for l, d in zip(timelines, [kept] if sequential else kept)])
                host.append((time.perf_counter() - h0) * 1e3)
            case["host_counts_ms"] = statistics.median(host)
            case["host_over_call"] = case["host_counts_ms"] / case["counts_call_ms"]["median"]
            mine = np.stack([got.tp[:, 0], got.fn[:, 0], got.fp[:, 0], got.melody_tp[:, 0], got.melody_fn[:, 0], got.melody_fp[:, 0]], axis=1)
            case["equal_to_host"] = bool(np.array_equal(want, mine))
        res["counts"].append(case)

    # the error notes of the full roll, one threshold
    lib = native.load()
    T, max_labels = len(timelines), int(np.diff(offsets).max())
    cap = lib.m2m_score_error_notes_capacity(R, L, int(sequential), max_labels, 0)
    need = lib.m2m_score_error_notes_workspace_bytes(T, frame_cap, 0)
    ws = torch.empty(need // 8, dtype=torch.int64, device="cuda")
    out_notes = torch.empty((T, 3, cap, 3), dtype=torch.int32, device="cuda")
    out_counts = torch.empty((T, 3), dtype=torch.int32, device="cuda")

    def enqueue_notes():
        native.check(lib.m2m_score_error_notes(dn.notes.data_ptr(), dn.counts.data_ptr(), dn.note_lp.data_ptr(), R, L, int(sequential),
                                               float(dn.time_step), lab.data_ptr(), off.data_ptr(), int(packed.shape[1]), T, frame_cap,
                                               float("-inf"), 0, max_labels, ws.data_ptr(), need, out_notes.data_ptr(), out_counts.data_ptr(),
                                               native.stream_handle(out_notes.device)), "m2m_score_error_notes")
    notes_call = lambda: scoring.error_notes(tok, ids_dev, labels, token_logprobs=lp_dev, **mode).to_numpy()
    for _ in range(5):
        found = notes_call()
    notes = {"workspace_bytes": int(need), "cap": int(cap), "runs_found": [int(sum(len(f[q]) for f in found)) for q in range(3)],
             "notes_kernel_ms": events(enqueue_notes), "notes_call_ms": wall(notes_call)}
    notes["kernel_over_chroma_kernel"] = notes["notes_kernel_ms"]["median"] / res["chroma_kernel_ms"]["median"]
    notes["call_over_chroma_call"] = notes["notes_call_ms"]["median"] / res["chroma_call_ms"]["median"]
    if args.host_reps > 0:
        host, same = [], True
        for _ in range(args.host_reps):
            h0 = time.perf_counter()
            kept, _ = confidence.decode_with_confidence(tok, ids, lp, min_confidence=0.0, **mode)
            want = [[frame_metrics.roll_to_notes(r) for r in frame_metrics.error_rolls(l, d)] for l, d in zip(timelines, [kept] if sequential else kept)]
            host.append((time.perf_counter() - h0) * 1e3)
        for a, b in zip(want, found):
            same &= all(np.array_equal(x, y) for x, y in zip(a, b))
        notes["host_notes_ms"] = statistics.median(host)
        notes["host_over_call"] = notes["host_notes_ms"] / notes["notes_call_ms"]["median"]
        notes["equal_to_host"] = bool(same)
    res["error_notes"] = notes
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=3, help="0 skips the host leg")
    ap.add_argument("--corrupt", type=float, default=0.05)
    ap.add_argument("--limit", type=float, default=300.0, help="seconds one shape may take")
    ap.add_argument("--shape", type=int, default=None, help="measure this shape only, in this process")
    args = ap.parse_args()
    if args.runs < 20:
        ap.error("--runs must be at least 20")
    if args.shape is not None:
        print(json.dumps(measure(SHAPES[args.shape], args)), flush=True)
        return
    results = []
    for i in range(len(SHAPES)):
        cmd = [sys.executable, str(Path(__file__).resolve()), "--shape", str(i), "--runs", str(args.runs), "--host-reps", str(args.host_reps),
               "--corrupt", str(args.corrupt)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"shape {i} did not finish within {args.limit:g} s: nothing more is started") from None
        if done.returncode != 0:
            raise SystemExit(f"shape {i} failed with status {done.returncode}: nothing more is started\n{done.stderr[-2000:]}")
        results.append(json.loads(done.stdout.strip().splitlines()[-1]))
    print(json.dumps({"shapes": results}), flush=True)
    if any(c.get("equal_to_host") is False for r in results for c in r["counts"] + [r["error_notes"]]):
        raise SystemExit("the device results differ from the definition's")


if __name__ == "__main__":
    main()
