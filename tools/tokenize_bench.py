#!/usr/bin/env python3
"""Tokenising of note labels on the device against the host's (MidiTokenizer.__call__: numpy, one Python loop per clip) on one GPU.

    python tools/tokenize_bench.py [--reps 30] [--warmup 3] [--parts calls,fit] [--fit-steps 50] [--fit-reps 5]

Note arrays are drawn from a seed at the reference geometry (50 ms step, 200 time ids): 16 clips x 45 notes and 16 x 90 notes of 3 s,
128 x 90 notes of 3 s, 32 x 250 notes of 10 s.  Every figure is the median of `--reps` warm runs (`--fit-reps` for the training part),
with the quartiles next to it.

  calls  wall clock of the host's labels - tokenizer(batch), PAD -> -100, the pad to the bucket: what Music2MIDI._labels does, the
         tensor left on the host as the parent commit hands it to the trainer - against tokenize.tokenize(labels=True, bucket=16) end
         to end (eligibility pass, pack, upload, kernel, copy of the lengths, ending in a synchronise), the two tensors compared; and
         event timing of the kernel alone on notes that are on the device already (20 launches per event pair)
  fit    Music2MIDI.fit_batches over `--fit-steps` batches of 16 labelled 3 s clips with 90 notes each, bf16, random-init weights,
         with and without config.trainer.device_labels: one model, the key switched from call to call, interleaved after one warm
         pass over the same batches (every label width's graph is captured there; a second model from the same seed takes that
         pass with the key set, and the losses of the two are compared); steps per second from the wall clock of the call, which
         ends with the losses on the host.  The key-off leg is the parent commit's path.  `--parts fit_host` times that leg only
         and needs nothing of the tokenize module: it is the leg to run on an earlier commit for a same-machine comparison.
Prints one JSON line.
"""
from __future__ import annotations

import argparse
import copy
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from music2midi_amd import synth  # noqa: E402
from music2midi_amd.config import DEFAULT_CONFIG, load_config  # noqa: E402
from music2midi_amd.input import ModelInputs  # noqa: E402
from music2midi_amd.tokenizer import PAD, MidiTokenizer  # noqa: E402

BUCKET = 16
BATCHES = {"16x45_3s": (16, 45, 3.0), "16x90_3s": (16, 90, 3.0), "128x90_3s": (128, 90, 3.0), "32x250_10s": (32, 250, 10.0)}


def clip(rng, n: int, duration: float) -> np.ndarray:
    """n notes over `duration` seconds, sorted by onset as a dataset segment is, whole pitches 21..108."""
    on = np.sort(rng.uniform(0.0, duration, n))
    return np.stack([on, on + rng.uniform(0.03, 0.8, n), rng.integers(21, 109, n).astype(np.float64), np.full(n, 80.0)], axis=1)


def stats(ms: list) -> dict:
    q = np.percentile(np.asarray(ms, dtype=np.float64), [25, 50, 75])
    return {"median_ms": round(float(q[1]), 4), "q25_ms": round(float(q[0]), 4), "q75_ms": round(float(q[2]), 4), "runs": len(ms)}


def wall_ms(fn, reps: int, warmup: int) -> dict:
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return stats(out)


def event_ms(fn, reps: int, warmup: int, inner: int) -> dict:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return stats(out)


def host_labels(tok, batch) -> torch.Tensor:
    labels = tok(batch)
    labels[labels == PAD] = -100
    return torch.nn.functional.pad(labels, (0, -labels.shape[1] % BUCKET), value=-100)


def part_calls(reps: int, warmup: int) -> dict:
    from music2midi_amd import tokenize
    tok = MidiTokenizer(load_config(copy.deepcopy(DEFAULT_CONFIG)))
    rng = np.random.default_rng(0)
    out = {}
    for name, (B, n, duration) in BATCHES.items():
        batch = [clip(rng, n, duration) for _ in range(B)]
        want = host_labels(tok, batch)
        got = tokenize.tokenize(tok, batch, labels=True, bucket=BUCKET).ids
        flat, per_clip = tokenize._flat_notes(batch)
        packed = torch.from_numpy(tokenize._pack(flat, per_clip)).cuda()
        ids = torch.empty((B, tokenize.row_bound(n, 200)), dtype=torch.int64, device="cuda")
        lengths = torch.empty(B, dtype=torch.int32, device="cuda")
        vocabulary = tokenize._vocabulary(tok)
        row = {"labels_shape": list(want.shape), "labels_equal": bool(torch.equal(got.cpu(), want)),
               "host": wall_ms(lambda: host_labels(tok, batch), reps, warmup),
               "device": wall_ms(lambda: tokenize.tokenize(tok, batch, labels=True, bucket=BUCKET), reps, warmup),
               "kernel": event_ms(lambda: tokenize._enqueue(packed, len(flat), vocabulary, None, -100, True, PAD, ids, lengths), reps, warmup, 20)}
        row["host_over_device"] = round(row["host"]["median_ms"] / row["device"]["median_ms"], 1)
        out[name] = row
    return out


def part_fit(steps: int, reps: int, legs: tuple) -> dict:
    from music2midi_amd.model import Music2MIDI
    rng = np.random.default_rng(1)
    wav = torch.from_numpy(synth.waveform_batch(500, 16, 48000, "music")).cuda()
    idx = torch.from_numpy(synth.cond_index_batch(21, 16)).cuda()
    batches = [ModelInputs(input_waveform=wav, notes_batch=tuple(clip(rng, 90, 3.0) for _ in range(16)), cond_index=idx) for _ in range(steps)]

    def model(leg):
        cfg = copy.deepcopy(DEFAULT_CONFIG)
        cfg["trainer"]["log_every_n_steps"] = 10 ** 9             # no greedy decode inside the steps
        if leg == "device":
            cfg["trainer"]["device_labels"] = True
        torch.manual_seed(5)
        m = Music2MIDI(cfg).cuda()
        m.train_precision = "bf16"
        return m

    # one pass over the batches by one model per leg, from the same seed: the losses of the two paths, and the warm-up of the timed
    # model (trainer, one graph per label width, code objects).  The legs are then timed on ONE model, the key switched per call: two
    # model instances differ by 1-2 % in step rate whatever their label path (where their buffers landed), which is the size of
    # what is being measured.
    first = {}
    for leg in reversed(legs):
        m = model(leg)
        first[leg] = m.fit_batches(batches)
    rates = {leg: [] for leg in legs}
    for _ in range(reps):
        for leg in legs:
            if leg == "device":
                m.config.trainer.device_labels = True
            else:
                m.config.trainer.pop("device_labels", None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.fit_batches(batches)
            torch.cuda.synchronize()
            rates[leg].append(steps / (time.perf_counter() - t0))
    m.config.trainer.pop("device_labels", None)
    out = {"steps": steps, "clips": 16, "notes_per_clip": 90, "precision": "bf16",
           "label_widths": sorted({int(m._labels(b.notes_batch).shape[1]) for b in batches})}
    for leg in legs:
        q = np.percentile(np.asarray(rates[leg]), [25, 50, 75])
        out[leg] = {"steps_per_s": round(float(q[1]), 2), "q25": round(float(q[0]), 2), "q75": round(float(q[2]), 2),
                    "ms_per_step": round(1e3 / float(q[1]), 3), "all_runs": [round(r, 2) for r in rates[leg]]}
    if len(legs) == 2:
        out["first_pass_losses_equal"] = first[legs[0]] == first[legs[1]]
        out["device_over_host"] = round(out["device"]["steps_per_s"] / out["host"]["steps_per_s"], 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fit-steps", type=int, default=50)
    ap.add_argument("--fit-reps", type=int, default=5)
    ap.add_argument("--parts", default="calls,fit")
    args = ap.parse_args()
    parts = [p for p in args.parts.split(",") if p]
    if any(p not in ("calls", "fit", "fit_host") for p in parts):
        ap.error("--parts takes calls, fit, fit_host")
    if not torch.cuda.is_available():
        raise SystemExit("tokenize_bench needs a GPU: nothing here is measured on the host alone")
    out = {"metric": "label tokenising, device vs host", "reps": args.reps, "bucket": BUCKET}
    if "calls" in parts:
        out["calls"] = part_calls(args.reps, args.warmup)
    if "fit" in parts:
        out["fit"] = part_fit(args.fit_steps, args.fit_reps, ("host", "device"))
    if "fit_host" in parts:
        out["fit_host"] = part_fit(args.fit_steps, args.fit_reps, ("host",))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
