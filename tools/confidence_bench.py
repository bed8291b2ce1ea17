#!/usr/bin/env python3
"""Time of per-note confidence: the scored detokenise (scoring.detokenize_scored, m2m_score_detokenize_scored) against the plain one
(scoring.detokenize, m2m_score_detokenize) and against the host definition (confidence.decode_with_confidence) on the same ids, and
``Music2MIDI.generate_notes(return_confidence=True)`` against plain ``generate_notes`` on one recording.

    python tools/confidence_bench.py [--runs 30] [--host-reps 3] [--corrupt 0.05] [--legs plain,scored,host,notes_plain,notes_scored]

Detokenise legs, at the two shapes of tools/chroma_bench.py (32 rows x 1 023 ids, 128 rows x 346 ids; the labels' own tokens with
``--corrupt`` of the positions replaced by random ids; log-probabilities -Exp(0.12)).  After 5 warm calls, the median over ``--runs``
of the time between two events around one call (allocation of the outputs and the launch; nothing is copied to the host):
  plain_ms   scoring.detokenize            8 bytes read per id, 12 written per note
  scored_ms  scoring.detokenize_scored     4 more bytes read per id, 8 more written per note
  host_ms    median of ``--host-reps`` passes of confidence.decode_with_confidence on this machine's CPUs (ids already on the host)
The scored notes must equal the host's, and the two float32 parts bit for bit.
Whole-call legs: random-init weights (synth seed 0, bf16), one recording of 96 s = 32 segments of 3 s; the rows never emit EOS, so
every call decodes 1 023 columns.  After 2 warm calls, the median over ``--runs`` of the host clock around the call, which ends with
the notes on the host:
  notes_plain_ms   generate_notes(audio_y)                           greedy head, MidiTokenizer.decode on the host
  notes_scored_ms  generate_notes(audio_y, return_confidence=True)   scored head (logprobs), detokenise on the device
``--legs plain,notes_plain`` needs nothing of the confidence surface: those are the legs to run on an earlier commit for a
same-box comparison.  Prints one JSON line.
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

SHAPES = [dict(rows=32, length=1023, notes=250, seconds=10.0), dict(rows=128, length=346, notes=90, seconds=3.0)]
LEGS = ("plain", "scored", "host", "notes_plain", "notes_scored")


def _event_ms(fns, runs):
    """{name: [ms per run]} of the calls in `fns`, timed between two events each, alternating run by run."""
    import torch
    out = {name: [] for name in fns}
    for _ in range(runs):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1))
    return out


def _summary(ms):
    return {"median_ms": statistics.median(ms), "min_max_ms": [min(ms), max(ms)]}


def detokenise_legs(legs, runs, host_reps, corrupt):
    import numpy as np
    import torch
    from music2midi_amd import scoring
    from music2midi_amd.config import DEFAULT_CONFIG, load_config
    from music2midi_amd.tokenizer import EOS, ONSET, PAD, MidiTokenizer

    tok = MidiTokenizer(load_config(copy.deepcopy(DEFAULT_CONFIG)))
    results = []
    for shape in SHAPES:
        R, L, n, span = shape["rows"], shape["length"], shape["notes"], shape["seconds"]
        rng = np.random.default_rng(R)
        ids = np.full((R, L), PAD, dtype=np.int64)
        for r in range(R):
            dur = rng.uniform(0.05, 1.0, n)
            start = rng.uniform(0.0, span - dur)
            row = tok._tokenize(np.stack([start, start + dur, rng.integers(40, 80, n), np.full(n, 80.0)], axis=1)).numpy()[:L]
            ids[r, :len(row)] = row
        repl = rng.integers(0, 400, ids.shape)
        repl[repl == EOS] = ONSET
        ids = np.where(rng.random(ids.shape) < corrupt, repl, ids)
        lp = (-rng.exponential(0.12, ids.shape)).astype(np.float32)
        ids_dev, lp_dev = torch.from_numpy(ids).cuda(), torch.from_numpy(lp).cuda()
        res = {"rows": R, "ids_per_row": L, "runs": runs}
        fns = {}
        if "plain" in legs:
            fns["plain"] = lambda: scoring.detokenize(tok, ids_dev)
        if "scored" in legs:
            fns["scored"] = lambda: scoring.detokenize_scored(tok, ids_dev, lp_dev)
            fns["scored_half"] = lambda: scoring.detokenize_scored(tok, ids_dev, lp_dev, min_confidence=0.5)
        for fn in fns.values():
            for _ in range(5):
                dn = fn()
        for name, ms in _event_ms(fns, runs).items():
            res[name] = _summary(ms)
        if fns:
            dn = fns["scored" if "scored" in fns else "plain"]()
            res["notes"] = int(dn.counts.sum())
        if "scored" in fns:
            res["bytes_ratio"] = (12 * R * L + 20 * res["notes"]) / (8 * R * L + 12 * res["notes"])
            if "plain" in fns:
                res["scored_over_plain"] = res["scored"]["median_ms"] / res["plain"]["median_ms"]
        if "host" in legs and host_reps > 0:
            from music2midi_amd import confidence
            host = []
            for _ in range(host_reps):
                h0 = time.perf_counter()
                notes, conf = confidence.decode_with_confidence(tok, ids, lp)
                host.append((time.perf_counter() - h0) * 1e3)
            res["host"] = _summary(host)
            if "scored" in legs:
                res["host_over_scored"] = res["host"]["median_ms"] / res["scored"]["median_ms"]
                parts = [confidence.note_logprobs(tok, ids[r], lp[r])[1] for r in range(R)]
                res["equal_to_host"] = bool(
                    all(np.array_equal(a, b) for a, b in zip(dn.to_numpy(), notes))
                    and all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(dn.note_lp_numpy(), parts)))
        results.append(res)
    return results


def whole_call_legs(legs, runs):
    import torch
    from music2midi_amd import synth
    from music2midi_amd.checkpoint import load_t5_state
    from music2midi_amd.config import DEFAULT_CONFIG, T5Geometry
    from music2midi_amd.model import Music2MIDI

    m = Music2MIDI(copy.deepcopy(DEFAULT_CONFIG), precision="bf16")
    load_t5_state(m.model, synth.t5_state_dict(T5Geometry(DEFAULT_CONFIG["model"]["t5"]), seed=0), strict=False)
    m = m.cuda().eval()
    audio = synth.waveform(0, 96 * 16000)
    calls = {"notes_plain": lambda: m.generate_notes(audio_y=audio),
             "notes_scored": lambda: m.generate_notes(audio_y=audio, return_confidence=True)}
    res = {"segments": 32, "runs": runs}
    calls = {name: fn for name, fn in calls.items() if name in legs}
    times, notes = {name: [] for name in calls}, {}
    for fn in calls.values():
        for _ in range(2):
            fn()
    for _ in range(runs):                                       # alternating, run by run
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
            notes[name] = int(len(out[0] if isinstance(out, tuple) else out))
    for name in calls:
        res[name] = dict(_summary(times[name]), notes=notes[name])
    if "notes_plain" in res and "notes_scored" in res:
        res["scored_over_plain"] = res["notes_scored"]["median_ms"] / res["notes_plain"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=3, help="0 skips the host leg")
    ap.add_argument("--corrupt", type=float, default=0.05)
    ap.add_argument("--legs", default=",".join(LEGS))
    args = ap.parse_args()
    legs = [n for n in args.legs.split(",") if n]
    if any(n not in LEGS for n in legs):
        ap.error(f"--legs takes {list(LEGS)}")
    if args.runs < 20:
        ap.error("--runs must be at least 20")

    from music2midi_amd import native
    native.require_gpu()
    out = {"metric": "per-note confidence", "legs": legs}
    if any(n in legs for n in ("plain", "scored", "host")):
        out["shapes"] = detokenise_legs(legs, args.runs, args.host_reps, args.corrupt)
    if any(n.startswith("notes_") for n in legs):
        out["generate_notes"] = whole_call_legs(legs, args.runs)
    print(json.dumps(out), flush=True)
    if any(r.get("equal_to_host") is False for r in out.get("shapes", [])):
        raise SystemExit("the device notes differ from the host definition's")


if __name__ == "__main__":
    main()
