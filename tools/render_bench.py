#!/usr/bin/env python3
"""The note renderer (music2midi_amd/render.py, csrc/render.hip) on one GPU against its host definition.

    python tools/render_bench.py [--reps 30] [--warmup 3] [--parts shapes,generate,fit] [--fit-steps 30] [--fit-reps 3]

Every figure is the median of `--reps` warm runs with the quartiles next to it.  Kernels are timed by device events, calls by the
host clock ending in a synchronise.  Notes come from a seed: uniform onsets, 0.05..1 s long, pitches 21..108.

  shapes    for one recording of 240 s with 20 000 notes at 16 kHz and at 48 kHz, 16 clips x 3 s x 90 notes and 128 x 3 s x 90
            notes at 16 kHz:
              kernel   one launch of m2m_render_notes_f32 on lists uploaded beforehand
              copy     a device-to-device copy of the output's bytes, for scale
              call     render.render from numpy notes to the tensor: pack, tile lists, one upload, the launch
              host     render.render_host on this machine's CPUs (one run at the 240 s shapes, three at the others)
            and the device result compared with the host's bit for bit
  generate  Music2MIDI.generate_audio against generate_notes on a 240 s recording (random-init weights, bf16, decoded under the
            MIDI grammar so that the random model writes notes)
  fit       Music2MIDI.fit_batches steps per second, bf16, fed from render.synthetic_batch (a fresh labelled batch per step)
            against one pre-built batch fed over and over
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

from music2midi_amd import render  # noqa: E402
from music2midi_amd.config import DEFAULT_CONFIG  # noqa: E402

SHAPES = [("240s_16k", 16000, 1, 240.0, 20000), ("240s_48k", 48000, 1, 240.0, 20000), ("16x3s_16k", 16000, 16, 3.0, 90),
          ("128x3s_16k", 16000, 128, 3.0, 90)]


def notes_for(seed: int, n: int, seconds: float) -> np.ndarray:
    rng = np.random.default_rng(seed)
    onset = rng.uniform(0.0, seconds, n)
    return np.stack([onset, onset + rng.uniform(0.05, 1.0, n), rng.integers(21, 109, n).astype(np.float64),
                     rng.integers(1, 128, n).astype(np.float64)], axis=1)


def stats(values: list, unit: str = "ms") -> dict:
    q = np.percentile(np.asarray(values, dtype=np.float64), [25, 50, 75])
    return {f"median_{unit}": round(float(q[1]), 4), f"q25_{unit}": round(float(q[0]), 4), f"q75_{unit}": round(float(q[2]), 4), "runs": len(values)}


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


def event_ms(fn, reps: int, warmup: int) -> dict:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return stats(out)


def part_shapes(reps: int, warmup: int) -> dict:
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = {}
    for name, fs, clips, seconds, per_clip in SHAPES:
        voice = render.default_voice(fs)
        n = int(fs * seconds)
        batch = [notes_for(100 + c, per_clip, seconds) for c in range(clips)]
        packed = [render.pack(x, fs, n, voice) for x in batch]
        words, counts = render.device_lists(packed, n, voice)
        lists = torch.from_numpy(words).to(dev)
        out = torch.empty((clips, n), dtype=torch.float32, device=dev)
        other = torch.empty_like(out)
        row = {"fs": fs, "clips": clips, "samples_per_clip": n, "notes": int(counts[0]), "list_entries": int(counts[2]),
               "upload_bytes": int(words.nbytes), "output_bytes": int(out.numel() * 4)}
        row["kernel"] = event_ms(lambda: render.launch(lists, counts, voice, out), reps, warmup)
        row["copy"] = event_ms(lambda: other.copy_(out), reps, warmup)
        row["call"] = wall_ms(lambda: render.render(batch, fs, n, voice), reps, warmup)
        host_runs = 1 if seconds > 10 else 3
        ms, want = [], None
        for _ in range(host_runs):
            t0 = time.perf_counter()
            want = render.render_batch_host(batch, fs, n, voice)
            ms.append((time.perf_counter() - t0) * 1e3)
        row["host"] = stats(ms)
        row["equal_to_host"] = bool(np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)))
        row["note_samples_per_s"] = round(float(sum((np.minimum(p.off + voice.release, n) - np.maximum(p.on, 0)).sum() for p in packed))
                                          / (row["kernel"]["median_ms"] * 1e-3), 0)
        row["host_over_call"] = round(row["host"]["median_ms"] / row["call"]["median_ms"], 1)
        rows[name] = row
        print(json.dumps({name: row}), file=sys.stderr, flush=True)
    return rows


def part_generate(reps: int) -> dict:
    from music2midi_amd import synth
    from music2midi_amd.model import Music2MIDI
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["inference"]["midi_grammar"] = True                                   # random weights write no notes otherwise
    torch.manual_seed(5)
    m = Music2MIDI(cfg).cuda().eval()
    m.model.set_precision("bf16")
    fs = cfg["model"]["sample_rate"]
    clip = np.concatenate([synth.waveform(k, 24 * fs, "music") for k in range(10)])
    notes, sound = m.generate_audio(audio_y=clip, fs=48000)                   # warm
    out = {"seconds": len(clip) / fs, "notes": int(len(notes)), "audio_samples": int(sound.shape[0]), "fs": 48000}
    a, b = [], []
    for _ in range(reps):
        for leg, fn in ((a, lambda: m.generate_notes(audio_y=clip)), (b, lambda: m.generate_audio(audio_y=clip, fs=48000))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            leg.append((time.perf_counter() - t0) * 1e3)
    out["generate_notes"], out["generate_audio"] = stats(a), stats(b)
    out["audio_over_notes"] = round(out["generate_audio"]["median_ms"] / out["generate_notes"]["median_ms"], 4)
    return out


def part_fit(steps: int, reps: int) -> dict:
    from music2midi_amd.model import Music2MIDI
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["trainer"]["log_every_n_steps"] = 10 ** 9                             # no greedy decode inside the steps
    cfg["trainer"]["device_labels"] = True
    clips = int(cfg["dataloader"]["batch_size"])
    torch.manual_seed(5)
    m = Music2MIDI(cfg).cuda()
    m.train_precision = "bf16"
    built = render.synthetic_batch(np.random.default_rng(1), clips, cfg)

    def fresh(seed):
        rng = np.random.default_rng(seed)
        return (render.synthetic_batch(rng, clips, cfg) for _ in range(steps))
    legs = {"prebuilt": lambda seed: m.fit_batches([built] * steps), "synthetic": lambda seed: m.fit_batches(fresh(seed))}
    for leg, run in legs.items():                                             # the warm pass: trainer, one graph per label width
        losses = run(0)
        assert len(losses) == steps and all(np.isfinite(losses)), (leg, losses[:4])
    rates = {leg: [] for leg in legs}
    for r in range(reps):
        for leg, run in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(1 + r)
            torch.cuda.synchronize()
            rates[leg].append(steps / (time.perf_counter() - t0))
    rng = np.random.default_rng(9)
    out = {"steps": steps, "clips": clips, "precision": "bf16", "batch_alone": wall_ms(lambda: render.synthetic_batch(rng, clips, cfg), 30, 3)}
    for leg in legs:
        q = np.percentile(np.asarray(rates[leg]), [25, 50, 75])
        out[leg] = {"steps_per_s": round(float(q[1]), 2), "q25": round(float(q[0]), 2), "q75": round(float(q[2]), 2),
                    "all_runs": [round(v, 2) for v in rates[leg]]}
    out["synthetic_over_prebuilt"] = round(out["synthetic"]["steps_per_s"] / out["prebuilt"]["steps_per_s"], 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fit-steps", type=int, default=30)
    ap.add_argument("--fit-reps", type=int, default=3)
    ap.add_argument("--generate-reps", type=int, default=3)
    ap.add_argument("--parts", default="shapes,generate,fit")
    args = ap.parse_args()
    parts = [p for p in args.parts.split(",") if p]
    if any(p not in ("shapes", "generate", "fit") for p in parts):
        ap.error("--parts takes shapes, generate, fit")
    if not torch.cuda.is_available():
        raise SystemExit("render_bench needs a GPU: nothing here is measured on the host alone")
    out = {"metric": "notes to audio on the device", "reps": args.reps, "tile": render.tile_size()}
    if "shapes" in parts:
        out["shapes"] = part_shapes(args.reps, args.warmup)
    if "generate" in parts:
        out["generate"] = part_generate(args.generate_reps)
    if "fit" in parts:
        out["fit"] = part_fit(args.fit_steps, args.fit_reps)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
