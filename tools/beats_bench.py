#!/usr/bin/env python3
"""The beat tracker (music2midi_amd/beats.py, csrc/beats.hip) on one GPU against its host definition.

    python tools/beats_bench.py [--reps 30] [--warmup 3] [--parts single,batch,notes,generate,filter] [--host-runs 1]

Every device figure is the median of `--reps` warm runs with the quartiles next to it.  Launches are timed by device events on inputs
prepared beforehand, whole calls by the host clock ending in a synchronise.  A clip is made as tests/beats_cases.py makes one: beats
with a sinusoidal drift, notes on 90 % of them and on 30 % of the off-beat eighths, rendered by render.render_host.

  single    one recording of 240 s (12 001 frames): the envelope launch, the track launch, track as a whole; track_host on this
            machine's CPUs (`--host-runs` runs)
  batch     16 recordings of 30 s: the same through track_batch
  notes     128 covers of 30 s through track_notes against track_notes_host
  generate  Music2MIDI.generate(beat_grid=True) against plain generate on the 240 s recording (a random-init model under the grammar)
  filter    filter_metrics as a share of align_notes on one 30 s pair
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

from music2midi_amd import align, beats, render  # noqa: E402


def make_clip(seed: int, bpm: float, drift: float, seconds: float, with_audio: bool = True) -> dict:
    rng = np.random.default_rng(seed)
    phase = rng.uniform(0, 2 * np.pi)
    t, grid = rng.uniform(0.1, 0.5), []
    while t < seconds - 0.3:
        grid.append(t)
        t += 60.0 / bpm * (1.0 + drift * np.sin(2 * np.pi * t / seconds + phase))
    grid = np.array(grid)
    rows = []
    for k, b in enumerate(grid):
        step = (grid[k + 1] - b) if k + 1 < len(grid) else (b - grid[k - 1])
        for at, chance in ((b, 0.9), (b + step / 2, 0.3)):
            if rng.random() < chance:
                onset = max(0.0, at + rng.normal(0.0, 0.010))
                for pitch in rng.choice(np.arange(48, 85), rng.integers(1, 4), replace=False):
                    rows.append([onset, min(onset + 0.8 * step, seconds - 0.05), float(pitch), 80.0])
    notes = np.array(rows, dtype=np.float64)
    notes = notes[np.argsort(notes[:, 0], kind="stable")]
    audio = render.render_host(notes, align.FS, int(seconds * align.FS), normalize=True) if with_audio else None
    return dict(audio=audio, notes=notes, beats=grid, bpm=bpm, frames=align.num_frames(int(seconds * align.FS)))


def f_measure(found, truth, window: float = 0.070) -> float:
    i = j = hits = 0
    while i < len(found) and j < len(truth):
        if abs(found[i] - truth[j]) <= window:
            hits, i, j = hits + 1, i + 1, j + 1
        elif found[i] < truth[j]:
            i += 1
        else:
            j += 1
    return round(2.0 * hits / max(1, len(found) + len(truth)), 3)


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


def host_ms(fn, runs: int):
    ms, result = [], None
    for _ in range(runs):
        t0 = time.perf_counter()
        result = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms), result


def track_launch(env, frames, dev, reps, warmup) -> dict:
    """The m2m_beat_track launch alone: tables, workspace and outputs are made beforehand."""
    import ctypes as C
    from music2midi_amd import native
    lib = native.load()
    n = len(frames)
    fr = np.ascontiguousarray(frames, dtype=np.int32)
    need = int(lib.m2m_beat_track_workspace_bytes(fr.ctypes.data_as(C.c_void_p), n))
    room = fr.astype(np.int64) // 8 + 2
    clips = np.zeros((n, 4), dtype=np.int32)
    clips[:, 0], clips[:, 1], clips[:, 3] = align._offsets(frames)[:-1], fr, np.cumsum(room) - room
    prior, table = beats._tables_device(None, None, dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    P = torch.empty(n, dtype=torch.int32, device=dev)
    score = torch.empty((n, 101), dtype=torch.int64, device=dev)
    out = torch.empty(int(room.sum()), dtype=torch.int32, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)

    def launch():
        native.check(lib.m2m_beat_track(env.data_ptr(), int(env.shape[0]), clips.ctypes.data_as(C.c_void_p), n, prior.data_ptr(), table.data_ptr(), 25,
                                        ws.data_ptr(), need, P.data_ptr(), score.data_ptr(), out.data_ptr(), int(room.sum()), count.data_ptr(),
                                        native.stream_handle(dev)), "m2m_beat_track")
    return event_ms(launch, reps, warmup)


def audio_part(clips: list, reps: int, warmup: int, host_runs: int) -> dict:
    dev = torch.device("cuda", torch.cuda.current_device())
    out = {"clips": len(clips), "seconds": len(clips[0]["audio"]) / align.FS}
    ys = [torch.from_numpy(c["audio"]).to(dev) for c in clips]
    out["band_energies"] = wall_ms(lambda: align._band_log_energies_device(ys, dev), reps, warmup)
    L, frames = align._band_log_energies_device(ys, dev)
    out["frames"] = frames
    out["envelope_launch"] = event_ms(lambda: beats._envelope_device(L, frames, dev), reps, warmup)
    env = beats._envelope_device(L, frames, dev)
    out["track_launch"] = track_launch(env, frames, dev, reps, warmup)
    audios = [c["audio"] for c in clips]
    out["call"] = wall_ms(lambda: beats.track_batch(audios), reps, warmup)
    got = beats.track_batch(audios)
    out["host"], want = host_ms(lambda: [beats.track_host(a) for a in audios], host_runs)
    out["device_f"] = [f_measure(r.beat_times, c["beats"]) for r, c in zip(got, clips)]
    out["host_f"] = [f_measure(r.beat_times, c["beats"]) for r, c in zip(want, clips)]
    out["periods"] = [int(r.period) for r in got]
    out["same_beats_as_host"] = [bool(np.array_equal(g.beat_frames, w.beat_frames)) for g, w in zip(got, want)]
    out["host_over_call"] = round(out["host"]["median_ms"] / out["call"]["median_ms"], 1)
    return out


def notes_part(clips: list, reps: int, warmup: int, host_runs: int) -> dict:
    dev = torch.device("cuda", torch.cuda.current_device())
    covers, frames = [c["notes"] for c in clips], [c["frames"] for c in clips]
    out = {"covers": len(clips)}
    env = torch.from_numpy(np.concatenate([beats.note_envelope(n, f) for n, f in zip(covers, frames)])).to(dev)
    out["track_launch"] = track_launch(env, frames, dev, reps, warmup)
    out["call"] = wall_ms(lambda: beats.track_notes(covers, frames), reps, warmup)
    got = beats.track_notes(covers, frames)
    out["host"], want = host_ms(lambda: [beats.track_notes_host(n, f) for n, f in zip(covers, frames)], host_runs)
    out["same_beats_as_host"] = all(np.array_equal(g.beat_frames, w.beat_frames) and g.period == w.period for g, w in zip(got, want))
    out["f_at_least_0.9"] = int(sum(f_measure(r.beat_times, c["beats"]) >= 0.9 for r, c in zip(got, clips)))
    out["host_over_call"] = round(out["host"]["median_ms"] / out["call"]["median_ms"], 1)
    return out


def generate_part(clip: dict, reps: int, warmup: int) -> dict:
    from music2midi_amd import audio
    from music2midi_amd.config import DEFAULT_CONFIG
    from music2midi_amd.model import Music2MIDI
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["inference"]["midi_grammar"] = True
    torch.manual_seed(0)
    model = Music2MIDI(cfg).cuda().eval()
    y = audio.resample(clip["audio"], align.FS, 16000).astype(np.float32)
    out = {"seconds": len(y) / 16000}
    out["generate"] = wall_ms(lambda: model.generate(audio_y=y, sr=16000), reps, warmup)
    out["generate_beat_grid"] = wall_ms(lambda: model.generate(audio_y=y, sr=16000, beat_grid=True), reps, warmup)
    out["generate_beats"] = wall_ms(lambda: model.generate_beats(audio_y=y, sr=16000), reps, warmup)
    out["beat_grid_over_plain"] = round(out["generate_beat_grid"]["median_ms"] / out["generate"]["median_ms"], 3)
    return out


def filter_part(clip: dict, reps: int, warmup: int) -> dict:
    seconds = len(clip["audio"]) / align.FS
    out = {"seconds": seconds}
    out["align_notes"] = wall_ms(lambda: align.align_notes(clip["audio"], clip["notes"]), reps, warmup)
    result = align.align_notes(clip["audio"], clip["notes"])
    out["filter_metrics"] = wall_ms(lambda: beats.filter_metrics(result, clip["notes"], seconds), reps, warmup)
    out["metrics"] = {k: round(float(v), 4) for k, v in beats.filter_metrics(result, clip["notes"], seconds).items()}
    out["filter_over_align"] = round(out["filter_metrics"]["median_ms"] / out["align_notes"]["median_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-runs", type=int, default=1)
    ap.add_argument("--parts", default="single,batch,notes,generate,filter")
    args = ap.parse_args()
    parts = [p for p in args.parts.split(",") if p]
    if any(p not in ("single", "batch", "notes", "generate", "filter") for p in parts):
        ap.error("--parts takes single, batch, notes, generate, filter")
    if not torch.cuda.is_available():
        raise SystemExit("beats_bench needs a GPU: nothing here is measured on the host alone")
    out = {"metric": "beats tracked on the device", "reps": args.reps}
    long_clip = make_clip(1, 108.0, 0.02, 240.0) if {"single", "generate"} & set(parts) else None
    if "single" in parts:
        out["single"] = audio_part([long_clip], args.reps, args.warmup, args.host_runs)
        print(json.dumps({"single": out["single"]}), file=sys.stderr, flush=True)
    if "batch" in parts:
        out["batch"] = audio_part([make_clip(10 + k, 92.0 + 2.5 * k, 0.02, 30.0) for k in range(16)], args.reps, args.warmup, args.host_runs)
        print(json.dumps({"batch": out["batch"]}), file=sys.stderr, flush=True)
    if "notes" in parts:
        out["notes"] = notes_part([make_clip(100 + k, 92.0 + 40.0 * k / 127, 0.02, 30.0, with_audio=False) for k in range(128)], args.reps,
                                  args.warmup, args.host_runs)
    if "generate" in parts:
        out["generate"] = generate_part(long_clip, max(3, args.reps // 6), 1)
    if "filter" in parts:
        out["filter"] = filter_part(make_clip(3, 108.0, 0.03, 30.0), args.reps, args.warmup)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
