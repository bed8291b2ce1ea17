#!/usr/bin/env python3
"""Time of the note-level precision / recall / F1 of one decoded batch: the device path (music2midi_amd.scoring.note_counts: the
matching of csrc/note_match.hip, one launch for all thresholds) against its definition on the host on the same ids
(confidence.decode_with_confidence + note_metrics.match_counts per threshold).

    python tools/note_metrics_bench.py [--runs 30] [--host-reps 3] [--corrupt 0.05] [--limit 300]

The two shapes of tools/chroma_bench.py: 32 rows x 1 023 ids with 250-note labels over 10 s, and 128 rows x 346 ids with 90-note
labels over 3 s; and one recording of 80 segments x 1 023 ids, ONE timeline of 20 000 label notes (sequential mode), where the
host definition builds n_ref x n_est matrices and runs once, for one threshold (every other case of that shape is compared with the
definition applied pitch by pitch).  The ids are the labels' own tokens with ``--corrupt`` of the positions replaced by random
ids, the tokens' log-probabilities are -Exp(0.12) (a confidence around one half per note).  Every shape is measured in a child process of its own
under a time limit of ``--limit`` seconds; the first one that fails ends the run.  After 5 warm calls, for K = 1 (threshold 0) and
K = 16 (thresholds 0 .. 0.9), with ``offset_ratio`` 0.2 and onsets only:
  kernel_ms        median over ``--runs`` of the time between two events around the matching launch alone (notes, labels and
                   thresholds already on the device)
  call_ms          median of the host clock around a whole note_counts call (detokenise, label upload, launch, copy of the counts)
  calls_16x1_ms    K = 16 only: the host clock around 16 calls with one threshold each
  host_ms          the definition on this machine's CPUs, median of ``--host-reps`` passes (K = 16, offset_ratio 0.2: one pass)
and chroma_call_ms, scoring.chroma_counts on the same ids, for scale.  The integers of the two paths must be equal.  Prints one
JSON line.
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
    # one recording: the rows are its segments, ONE timeline of 20 000 label notes (sequential mode)
    dict(rows=80, length=1023, notes=250, seconds=10.0, sequential=True),
]
SWEEP = [0.06 * k for k in range(16)]


def measure(shape: dict, args) -> dict:
    import numpy as np
    import torch
    from music2midi_amd import confidence, native, note_metrics, scoring
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
            call()                                              # returns after the counts are on the host
            times.append((time.perf_counter() - w0) * 1e3)
        return statistics.median(times)

    packed, offsets, _ = scoring._pack_labels(timelines)
    lab, off = torch.from_numpy(packed).cuda(), torch.from_numpy(offsets).cuda()
    dn = scoring.detokenize_scored(tok, ids_dev, lp_dev, **mode)
    res = {"rows": R, "ids_per_row": L, "label_notes": n, "sequential": sequential, "runs": args.runs, "decoded_notes": int(dn.counts.sum()), "cases": []}
    for ratio in (0.2, None):
        for thresholds in ([0.0], SWEEP):
            K = len(thresholds)
            count = lambda th=thresholds: scoring.note_counts(tok, ids_dev, labels, token_logprobs=lp_dev, thresholds=th, offset_ratio=ratio, **mode)
            for _ in range(5):
                got = count()
            thr = torch.from_numpy(scoring.threshold_logprobs(thresholds, True)).cuda()
            kernel = []
            for _ in range(args.runs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                scoring._enqueue_note_counts(dn, lab, off, thr, 0.05, -1.0 if ratio is None else ratio, 0.05)
                e1.record()
                torch.cuda.synchronize()
                kernel.append(e0.elapsed_time(e1))
            case = {"offset_ratio": ratio, "thresholds": K, "kernel_ms": statistics.median(kernel), "kernel_ms_min_max": [min(kernel), max(kernel)],
                    "call_ms": wall(count), "tp": got.tp.sum(axis=0).tolist(), "n_est": got.n_est.sum(axis=0).tolist(),
                    "n_ref": int(got.n_ref[:, 0].sum()), "f1": got.f1.tolist()}
            if K > 1:
                case["calls_16x1_ms"] = wall(lambda: [count([c]) for c in thresholds])
                case["one_call_over_16_calls"] = case["call_ms"] / case["calls_16x1_ms"]
            reps = 0 if args.host_reps <= 0 else 1 if K > 1 else args.host_reps
            if (K > 1 and ratio is None) or (sequential and (K > 1 or ratio is None)):
                reps = 0                                        # (one timeline: the definition builds n_ref x n_est matrices, one pass)
            elif sequential:
                reps = 1
            host = []
            for _ in range(reps):
                h0 = time.perf_counter()
                want = np.zeros((len(timelines), K, 3), dtype=np.int64)
                for k, c in enumerate(thresholds):
                    kept, _ = confidence.decode_with_confidence(tok, ids, lp, min_confidence=c, **mode)
                    for t, (l, d) in enumerate(zip(timelines, [kept] if sequential else kept)):
                        tp, n_ref, n_est = note_metrics.match_counts(l, d, offset_ratio=ratio)
                        want[t, k] = (tp, n_est, n_ref)
                host.append((time.perf_counter() - h0) * 1e3)
            if host:
                case["host_ms"] = statistics.median(host)
                case["host_over_call"] = case["host_ms"] / case["call_ms"]
                case["equal_to_host"] = bool(np.array_equal(want, np.stack([got.tp, got.n_est, got.n_ref], axis=2)))
            if sequential and args.host_reps > 0:
                # a hit needs equal pitches, so the hit graph is a disjoint union over the pitches and the definition applied per
                # pitch sums to the definition: small matrices, every threshold
                same = True
                for k, c in enumerate(thresholds):
                    kept, _ = confidence.decode_with_confidence(tok, ids, lp, min_confidence=c, **mode)
                    sums = np.zeros(3, dtype=np.int64)
                    for pitch in np.unique(np.concatenate([labels[:, 2], kept[:, 2]])):
                        sums += note_metrics.match_counts(labels[labels[:, 2] == pitch], kept[kept[:, 2] == pitch], offset_ratio=ratio)
                    same &= (int(got.tp[0, k]), int(got.n_ref[0, k]), int(got.n_est[0, k])) == tuple(sums.tolist())
                case["equal_to_host_per_pitch"] = bool(same)
            res["cases"].append(case)
    chroma = lambda: scoring.chroma_counts(tok, ids_dev, labels, **mode)
    for _ in range(5):
        chroma()
    res["chroma_call_ms"] = wall(chroma)
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
    if any(c.get(key) is False for r in results for c in r["cases"] for key in ("equal_to_host", "equal_to_host_per_pitch")):
        raise SystemExit("the device counts differ from the definition's")


if __name__ == "__main__":
    main()
