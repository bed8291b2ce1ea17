#!/usr/bin/env python3
"""Time of scoring one decoded batch: the device path (music2midi_amd.evaluation.evaluate_tokens: detokenise, melody and counts as
HIP kernels) against the host path on the same ids (MidiTokenizer.decode + numpy_to_midi + evaluation.evaluate_batch).

    python tools/chroma_bench.py [--runs 30] [--host-reps 3] [--corrupt 0.05]

Two shapes: 32 rows x 1 023 ids with 250-note labels over 10 s (the headline decode: 200.3 ms in bf16, README), and 128 rows x 346
ids with 90-note labels over 3 s (one chunk of `sample_tokens`: 360 ms computed to the end, README).  The ids are the labels'
own tokens with ``--corrupt`` of the positions replaced by random ids (EOS excluded), so the decoder meets unmatched offsets,
pending pitches and unused ids as it does on a model's output.  After 5 warm calls, per shape:
  kernels_ms      median over ``--runs`` of the time between two events around the two launches alone (labels already on the device;
                  detokenise_kernel_ms: the first of the two, to an event between them)
  device_ms       median of the time between two events around a whole evaluate_tokens call (label upload, launches, count copy)
  wall_ms         median of the host clock around the same call, which ends in the copy of the counts to the host
  host_ms         median of ``--host-reps`` passes of the host path, on this machine's CPUs
and the share of the decode each is.  The float of the two paths must be equal.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import copy
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

SHAPES = [  # rows, ids per row, label notes, seconds, the decode it follows (ms)
    dict(rows=32, length=1023, notes=250, seconds=10.0, decode_ms=200.3),
    dict(rows=128, length=346, notes=90, seconds=3.0, decode_ms=360.0),
]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=3, help="0 skips the host leg")
    ap.add_argument("--corrupt", type=float, default=0.05)
    args = ap.parse_args()
    if args.runs < 20:
        ap.error("--runs must be at least 20")

    import numpy as np
    import torch
    from music2midi_amd import evaluation, native, scoring
    from music2midi_amd.config import DEFAULT_CONFIG, load_config
    from music2midi_amd.tokenizer import EOS, ONSET, PAD, MidiTokenizer
    from music2midi_amd.utils import numpy_to_midi

    native.require_gpu()
    tok = MidiTokenizer(load_config(copy.deepcopy(DEFAULT_CONFIG)))
    results = []
    for shape in SHAPES:
        R, L, n, span = shape["rows"], shape["length"], shape["notes"], shape["seconds"]
        rng = np.random.default_rng(R)
        labels = []
        for _ in range(R):
            dur = rng.uniform(0.05, 1.0, n)
            start = rng.uniform(0.0, span - dur)
            labels.append(np.stack([start, start + dur, rng.integers(40, 80, n), np.full(n, 80.0)], axis=1))
        ids = np.full((R, L), PAD, dtype=np.int64)
        widths = []
        for r, notes in enumerate(labels):
            row = tok._tokenize(notes).numpy()[:L]
            ids[r, :len(row)] = row
            widths.append(len(row))
        repl = rng.integers(0, 400, ids.shape)
        repl[repl == EOS] = ONSET
        ids = np.where(rng.random(ids.shape) < args.corrupt, repl, ids)
        ids_host = torch.from_numpy(ids)
        ids_dev = ids_host.cuda()

        for _ in range(5):
            score = evaluation.evaluate_tokens(tok, ids_dev, labels)
        # the two launches alone
        packed, offsets, label_frames = scoring._pack_labels(labels)
        lab, off = torch.from_numpy(packed).cuda(), torch.from_numpy(offsets).cuda()
        cap = max(label_frames, scoring.frame_count((400 - 1 - tok.time_token_offset) * tok.time_step))
        kernels, detok, device, wall = [], [], [], []
        for _ in range(args.runs):
            e0, em, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            dn = scoring.detokenize(tok, ids_dev)
            em.record()
            out = scoring._enqueue_counts(dn, lab, off, cap)
            e1.record()
            torch.cuda.synchronize()
            kernels.append(e0.elapsed_time(e1))
            detok.append(e0.elapsed_time(em))
        for _ in range(args.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            e0.record()
            score = evaluation.evaluate_tokens(tok, ids_dev, labels)      # returns after the counts are on the host
            wall.append((time.perf_counter() - w0) * 1e3)
            e1.record()
            torch.cuda.synchronize()
            device.append(e0.elapsed_time(e1))
        res = {"rows": R, "ids_per_row": L, "label_notes": n, "mean_ids_before_pad": float(np.mean(widths)), "runs": args.runs,
               "kernels_ms": statistics.median(kernels), "kernels_ms_min_max": [min(kernels), max(kernels)],
               "detokenise_kernel_ms": statistics.median(detok),
               "device_ms": statistics.median(device), "wall_ms": statistics.median(wall), "wall_ms_min_max": [min(wall), max(wall)],
               "decode_ms": shape["decode_ms"], "score": score}
        res["kernels_share_of_decode"] = res["kernels_ms"] / shape["decode_ms"]
        res["wall_share_of_decode"] = res["wall_ms"] / shape["decode_ms"]
        counts = out.cpu().numpy()
        res["device_counts_equal"] = bool(counts[:, 1].sum() > 0 and float(counts[:, 0].sum() / counts[:, 1].sum()) == score)
        if args.host_reps > 0:
            parts = {"detokenise_ms": [], "numpy_to_midi_ms": [], "score_ms": []}
            for _ in range(args.host_reps):
                h0 = time.perf_counter()
                decoded = tok.decode(ids_host, mode="batched")
                h1 = time.perf_counter()
                predicted, wanted = [numpy_to_midi(d) for d in decoded], [numpy_to_midi(l) for l in labels]
                h2 = time.perf_counter()
                host_score = evaluation.evaluate_batch(wanted, predicted)
                h3 = time.perf_counter()
                for key, dt in zip(parts, (h1 - h0, h2 - h1, h3 - h2)):
                    parts[key].append(dt * 1e3)
            res.update({"host_" + k: statistics.median(v) for k, v in parts.items()})
            res["host_ms"] = sum(statistics.median(v) for v in parts.values())
            res["host_share_of_decode"] = res["host_ms"] / shape["decode_ms"]
            res["host_over_wall"] = res["host_ms"] / res["wall_ms"]
            res["equal_to_host"] = bool(score == host_score)
        results.append(res)
    print(json.dumps({"shapes": results}), flush=True)
    if any(r.get("equal_to_host") is False for r in results):
        raise SystemExit("the device score differs from the host's")


if __name__ == "__main__":
    main()
