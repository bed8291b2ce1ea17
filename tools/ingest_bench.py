#!/usr/bin/env python3
"""Audio ingest on the device against the host's (audio.load_audio: numpy + scipy) on one GPU.

    python tools/ingest_bench.py [--reps 30] [--warmup 3] [--parts kernels,calls,e2e] [--seconds 240] [--e2e-reps 5]

Files are written to a temporary directory from a seed: 16-bit stereo at 44.1 kHz and at 48 kHz, `--seconds` long, and a 3 s clip
at 44.1 kHz.  Every figure is the median of `--reps` warm runs (`--e2e-reps` for the end-to-end part), with the quartiles next to it.

  kernels  event timing of the decode kernel (m2m_ingest_pcm) and the resample kernel (m2m_ingest_resample_f32, padded to whole
           3 s segments), next to a plain device-to-device copy of the decode kernel's input bytes timed the same way
  calls    wall clock, ending in a synchronise, of ingest.load_audio_device(path, 16000) against
           torch.from_numpy(audio.load_audio(path, 16000)).to(device), file in the page cache, and their samples compared
  e2e      Music2MIDI.generate_notes(audio_path=...) of the long 44.1 kHz file, random-init weights (synth seed 0), fp32, with and
           without config.inference.device_ingest, interleaved; the ingest share is the time of _padded_segments inside the call.
           `--parts e2e_host` times the run without the key only and needs nothing of the ingest module: it is the leg to run on
           an earlier commit for a same-machine comparison.
Prints one JSON line.
"""
from __future__ import annotations

import argparse
import copy
import json
import struct
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from music2midi_amd import audio, synth  # noqa: E402
from music2midi_amd.checkpoint import load_t5_state  # noqa: E402
from music2midi_amd.config import DEFAULT_CONFIG, T5Geometry  # noqa: E402

SR = 16000


def write_wav(path: Path, rate: int, seconds: float, seed: int) -> Path:
    """16-bit stereo: noise plus two sines, the channels at different levels."""
    n = int(rate * seconds)
    t = np.arange(n) / rate
    y = 0.25 * np.random.default_rng(seed).standard_normal(n) + 0.2 * np.sin(2 * np.pi * 440 * t) + 0.15 * np.sin(2 * np.pi * 1318.5 * t)
    body = np.round(np.stack([y, 0.7 * y], axis=1).clip(-1, 1) * 32767).astype("<i2").tobytes()
    fmt = struct.pack("<HHIIHH", 1, 2, rate, rate * 4, 4, 16)
    chunks = b"fmt " + struct.pack("<I", 16) + fmt + b"data" + struct.pack("<I", len(body)) + body
    path.write_bytes(b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks)
    return path


def stats(ms: list) -> dict:
    q = np.percentile(np.asarray(ms, dtype=np.float64), [25, 50, 75])
    return {"median_ms": round(float(q[1]), 4), "q25_ms": round(float(q[0]), 4), "q75_ms": round(float(q[2]), 4), "runs": len(ms)}


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


def part_kernels(files: dict, reps: int, warmup: int) -> dict:
    from music2midi_amd import ingest
    out = {}
    for name, path in files.items():
        rate = audio.read_wav(path)[1]
        raw = path.read_bytes()
        lay = audio.wav_layout(path, raw)
        frames = lay.data_size // 4
        body = torch.from_numpy(np.frombuffer(raw, np.uint8, frames * 4, lay.data_offset).copy()).cuda()
        sink = torch.empty_like(body)
        mono = ingest.decode_pcm_device(body, frames, 2, "s16")
        up, down = ingest.ratio(rate, SR)
        n_out = ingest.resampled_length(frames, up, down)
        capacity = -(-n_out // (3 * SR)) * (3 * SR)
        row = {"frames": frames, "up": up, "down": down, "taps_per_output": 20 * max(up, down) // up + 1, "n_out": n_out,
               "bytes_in": int(body.numel()), "bytes_out": 4 * capacity,
               "copy_of_input_bytes": event_ms(lambda: sink.copy_(body), reps, warmup),
               "decode": event_ms(lambda: ingest.decode_pcm_device(body, frames, 2, "s16"), reps, warmup),
               "resample": event_ms(lambda: ingest._resample(mono, up, down, capacity), reps, warmup)}
        row["resample_over_copy"] = round(row["resample"]["median_ms"] / row["copy_of_input_bytes"]["median_ms"], 2)
        row["multiply_adds_per_s"] = round(n_out * row["taps_per_output"] / (row["resample"]["median_ms"] * 1e-3), 0)
        out[name] = row
    return out


def part_calls(files: dict, reps: int, warmup: int) -> dict:
    from music2midi_amd import ingest
    out = {}
    for name, path in files.items():
        dev = ingest.load_audio_device(path, SR)
        host = torch.from_numpy(audio.load_audio(path, SR)).cuda()
        row = {"samples_equal": bool(torch.equal(dev, host)),
               "device": wall_ms(lambda: ingest.load_audio_device(path, SR), reps, warmup),
               "host": wall_ms(lambda: torch.from_numpy(audio.load_audio(path, SR)).cuda(), max(3, reps // 3), 1)}
        row["host_over_device"] = round(row["host"]["median_ms"] / row["device"]["median_ms"], 1)
        out[name] = row
    return out


def part_e2e(path: Path, reps: int, legs: tuple) -> dict:
    from music2midi_amd.model import Music2MIDI
    geom = T5Geometry(DEFAULT_CONFIG["model"]["t5"])
    m = Music2MIDI(copy.deepcopy(DEFAULT_CONFIG), precision="fp32")
    load_t5_state(m.model, synth.t5_state_dict(geom, seed=0), strict=False)
    m = m.cuda().eval()
    inner = m._padded_segments
    spent = []

    def timed_segments(*a, **k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = inner(*a, **k)
        torch.cuda.synchronize()
        spent.append((time.perf_counter() - t0) * 1e3)
        return r
    m._padded_segments = timed_segments

    def run(leg):
        if leg == "device":
            m.config.inference.device_ingest = True
        else:
            m.config.inference.pop("device_ingest", None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        notes = m.generate_notes(audio_path=path)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, spent.pop(), notes

    notes = {leg: run(leg)[2] for leg in legs}                       # warm-up: sessions, code objects, the filter
    total, ingest_ms = {leg: [] for leg in legs}, {leg: [] for leg in legs}
    for _ in range(reps):
        for leg in legs:
            t, s, _ = run(leg)
            total[leg].append(t)
            ingest_ms[leg].append(s)
    out = {leg: {"generate_notes": stats(total[leg]), "ingest": stats(ingest_ms[leg]), "all_runs_ms": [round(t, 1) for t in total[leg]]}
           for leg in legs}
    for leg in legs:
        out[leg]["ingest_share"] = round(out[leg]["ingest"]["median_ms"] / out[leg]["generate_notes"]["median_ms"], 3)
    if len(legs) == 2:
        out["notes_equal"] = bool(np.array_equal(notes[legs[0]], notes[legs[1]]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--e2e-reps", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--parts", default="kernels,calls,e2e")
    args = ap.parse_args()
    parts = [p for p in args.parts.split(",") if p]
    if any(p not in ("kernels", "calls", "e2e", "e2e_host") for p in parts):
        ap.error("--parts takes kernels, calls, e2e, e2e_host")
    if not torch.cuda.is_available():
        raise SystemExit("ingest_bench needs a GPU: nothing here is measured on the host alone")
    out = {"metric": "audio ingest, device vs host", "target_rate": SR, "seconds": args.seconds, "reps": args.reps}
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        files = {"long_44100": write_wav(tmp / "long_44100.wav", 44100, args.seconds, 0),
                 "long_48000": write_wav(tmp / "long_48000.wav", 48000, args.seconds, 1),
                 "clip_3s_44100": write_wav(tmp / "clip_44100.wav", 44100, 3.0, 2)}
        if "kernels" in parts:
            out["kernels"] = part_kernels(files, args.reps, args.warmup)
        if "calls" in parts:
            out["calls"] = part_calls(files, args.reps, args.warmup)
        if "e2e" in parts:
            out["e2e"] = part_e2e(files["long_44100"], args.e2e_reps, ("host", "device"))
        if "e2e_host" in parts:
            out["e2e_host"] = part_e2e(files["long_44100"], args.e2e_reps, ("host",))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
