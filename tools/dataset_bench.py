#!/usr/bin/env python3
"""The device-resident training dataset (music2midi_amd/dataset.py, csrc/dataset.hip) against the ways a batch's audio could be
produced before it, on one GPU.

    python tools/dataset_bench.py [--reps 30] [--warmup 3] [--recordings 16] [--seconds 240] [--fit-steps 50] [--fit-reps 5]
                                  [--parts crops,kernel,fit]

A data directory in the reference's layout is written to a temporary directory from a seed: `--recordings` 16-bit stereo files at
44.1 kHz, `--seconds` long, with 90 notes in every 3 s segment.  A batch is 16 clips of 3 s -> [16, 66150] fp32 at 22 050 Hz.
Every figure is the median of `--reps` warm runs with the quartiles next to it (the host crop: a tenth of the runs, at least 3).

  crops   wall clock, ending in a synchronise, of one batch's audio from fixed (recording, start) pairs:
            host      torch.from_numpy(crop_host(...)).to(device)             read_wav of the whole file, slice, mean, resample
            ingest    16 x ingest.load_audio_device(offset=, duration=) + torch.stack     what the parent commit can do on the device
            resident  crop_device, the sample bytes in device memory
            streamed  crop_device, resident_bytes = 0: the slices' bytes through one pinned buffer and one copy
          and the four results compared bit for bit
  kernel  device events over 20 launches of m2m_dataset_crop_f32 on the resident clips (table copy included)
  fit     Music2MIDI.fit_batches, bf16, trainer.device_labels, `--fit-steps` steps, one model, the legs interleaved after a warm pass:
            prebuilt            one batch built beforehand, fed over and over (the loop of tools/tokenize_bench.py)
            prebuilt_augmented  the same with fit_batches(augment=rng): the pitch shift per step, no crop
            dataset             batches from Music2MIDIDataModule.train_batches: draw, crop, notes, augmentation per step
Prints one JSON line.
"""
from __future__ import annotations

import argparse
import copy
import ctypes as C
import itertools
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
import yaml  # noqa: E402

from music2midi_amd.config import DEFAULT_CONFIG  # noqa: E402

RATE, SEGMENT, CLIPS = 44100, 3, 16


def write_data_dir(root: Path, recordings: int, seconds: float) -> list:
    n = int(RATE * seconds)
    t = np.arange(n) / RATE
    base = 0.25 * np.random.default_rng(0).standard_normal(n) + 0.2 * np.sin(2 * np.pi * 440 * t) + 0.15 * np.sin(2 * np.pi * 1318.5 * t)
    rows = []
    for k in range(int(seconds // SEGMENT)):
        for j in range(90):
            onset = k * SEGMENT + (j + 0.5) * SEGMENT / 91
            rows.append([onset, onset + 0.2, 40 + j % 48, 80])
    notes = np.asarray(rows, dtype=np.float64)
    for sub in ("audio", "midi_numpy", "metadata"):
        (root / sub).mkdir()
    ids = [f"rec{r:03d}" for r in range(recordings)]
    for r, pid in enumerate(ids):
        y = np.roll(base, r * 7919) * (0.6 + 0.02 * r)
        body = np.round(np.stack([y, 0.7 * y], axis=1).clip(-1, 1) * 32767).astype("<i2").tobytes()
        fmt = struct.pack("<HHIIHH", 1, 2, RATE, RATE * 4, 4, 16)
        chunks = b"fmt " + struct.pack("<I", 16) + fmt + b"data" + struct.pack("<I", len(body)) + body
        (root / "audio" / f"{pid}.wav").write_bytes(b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks)
        np.save(root / "midi_numpy" / f"{pid}.npy", notes)
        (root / "metadata" / f"{pid}.yaml").write_text(yaml.safe_dump({"piano": {"genre": "pop", "difficulty": "advanced"}}))
    np.savez(root / "dataset_split.npz", train_id=np.array(ids, dtype=object), val_id=np.array(ids[:1], dtype=object))
    return ids


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


def part_crops(root: Path, ids: list, cfg: dict, reps: int, warmup: int) -> dict:
    from music2midi_amd import ingest
    from music2midi_amd.dataset import Music2MIDIDataset
    resident = Music2MIDIDataset(root, ids, cfg, device="cuda")
    streamed = Music2MIDIDataset(root, ids, cfg, device="cuda", resident_bytes=0)
    rng = np.random.default_rng(1)
    indices = [int(i) for i in rng.integers(0, len(ids), CLIPS)]
    starts = resident.draw(indices, rng)[0]
    sr = cfg["dataset"]["sample_rate"]

    def by_ingest():
        return torch.stack([ingest.load_audio_device(resident.audio_paths[i], sr, offset=s, duration=SEGMENT) for i, s in zip(indices, starts)])

    def by_host():
        return torch.from_numpy(resident.crop_host(indices, starts)).to("cuda")
    want = by_host()
    out = {"clips": CLIPS, "samples_per_clip": int(want.shape[1]), "residency": {k: len(v) for k, v in resident.residency()._asdict().items()},
           "resident_bytes": resident.resident_bytes(), "streamed_bytes_per_batch": CLIPS * SEGMENT * RATE * 4,
           "equal_to_host": {"ingest": bool(torch.equal(by_ingest(), want)), "resident": bool(torch.equal(resident.crop_device(indices, starts), want)),
                             "streamed": bool(torch.equal(streamed.crop_device(indices, starts), want))},
           "host": wall_ms(by_host, max(3, reps // 10), 1),
           "ingest": wall_ms(by_ingest, reps, warmup),
           "resident": wall_ms(lambda: resident.crop_device(indices, starts), reps, warmup),
           "streamed": wall_ms(lambda: streamed.crop_device(indices, starts), reps, warmup)}
    for k in ("host", "ingest", "streamed"):
        out[f"{k}_over_resident"] = round(out[k]["median_ms"] / out["resident"]["median_ms"], 2)
    return out


def part_kernel(root: Path, ids: list, cfg: dict, reps: int, warmup: int, inner: int = 20) -> dict:
    from music2midi_amd import ingest, native
    from music2midi_amd.dataset import Music2MIDIDataset
    ds = Music2MIDIDataset(root, ids, cfg, device="cuda")
    dev = ds.device
    rng = np.random.default_rng(1)
    indices = [int(i) for i in rng.integers(0, len(ids), CLIPS)]
    starts = ds.draw(indices, rng)[0]
    clips = (native.DatasetClip * CLIPS)()
    for c, i, s in zip(clips, indices, starts):
        rec = ds._recordings[i]
        c.bytes_dev = rec.body.data_ptr() + rec.first(s) * rec.frame_bytes
        c.h_phase_dev = ingest._filter_on(dev, rec.up, rec.down).data_ptr()
        c.n_frames, c.channels, c.format, c.up, c.down, c.half = rec.count, rec.n_ch, ingest.FORMATS[rec.kind][0], rec.up, rec.down, 10 * max(rec.up, rec.down)
    T = ds.segment_samples
    table = torch.empty(C.sizeof(clips), dtype=torch.uint8, device=dev)
    out = torch.empty((CLIPS, T), dtype=torch.float32, device=dev)
    lib, stream = native.load(), native.stream_handle(dev)

    def launches():
        for _ in range(inner):
            native.check(lib.m2m_dataset_crop_f32(clips, CLIPS, table.data_ptr(), out.data_ptr(), T, T, stream), "m2m_dataset_crop_f32")
    for _ in range(warmup):
        launches()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launches()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    row = {"per_launch": stats(ms), "launches_per_event_pair": inner, "bytes_in": CLIPS * SEGMENT * RATE * 4, "bytes_out": CLIPS * T * 4,
           "taps_per_output": 20 * max(ds._recordings[0].up, ds._recordings[0].down) // ds._recordings[0].up + 1}
    row["bytes_per_s"] = round((row["bytes_in"] + row["bytes_out"]) / (row["per_launch"]["median_ms"] * 1e-3), 0)
    return row


def part_fit(root: Path, cfg: dict, steps: int, reps: int) -> dict:
    from music2midi_amd.dataset import Music2MIDIDataModule
    from music2midi_amd.model import Music2MIDI
    cfg = copy.deepcopy(cfg)
    cfg["trainer"]["log_every_n_steps"] = 10 ** 9                 # no greedy decode inside the steps
    cfg["trainer"]["device_labels"] = True
    dm = Music2MIDIDataModule(root, cfg, device="cuda")
    dm.setup()
    plain = dm.train_set.batch(list(range(CLIPS)), np.random.default_rng(2), augment=False)
    built = dm.train_set.batch(list(range(CLIPS)), np.random.default_rng(2))
    torch.manual_seed(5)
    m = Music2MIDI(cfg).cuda()
    m.train_precision = "bf16"
    epochs = -(-steps * CLIPS // len(dm.train_set))

    def run(leg, seed):
        if leg == "prebuilt":
            return m.fit_batches([built] * steps)
        if leg == "prebuilt_augmented":
            return m.fit_batches([plain] * steps, augment=np.random.default_rng(seed))
        return m.fit_batches(itertools.islice(dm.train_batches(np.random.default_rng(seed), epochs=epochs), steps))
    legs = ("prebuilt", "prebuilt_augmented", "dataset")
    for leg in legs:                                             # the warm pass: trainer, one graph per label width, augmentation workspaces
        losses = run(leg, 0)
        assert len(losses) == steps and all(np.isfinite(losses)), (leg, losses[:4])
    rates = {leg: [] for leg in legs}
    for r in range(reps):
        for leg in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(leg, 1 + r)
            torch.cuda.synchronize()
            rates[leg].append(steps / (time.perf_counter() - t0))
    # the host's share of a dataset step: building the batch alone, nothing else in flight
    rng = np.random.default_rng(9)
    batch_ms = wall_ms(lambda: dm.train_set.batch(rng.permutation(len(dm.train_set))[:CLIPS], rng), 30, 3)
    out = {"steps": steps, "clips": CLIPS, "precision": "bf16", "batch_alone": batch_ms}
    for leg in legs:
        q = np.percentile(np.asarray(rates[leg]), [25, 50, 75])
        out[leg] = {"steps_per_s": round(float(q[1]), 2), "q25": round(float(q[0]), 2), "q75": round(float(q[2]), 2),
                    "ms_per_step": round(1e3 / float(q[1]), 3), "all_runs": [round(v, 2) for v in rates[leg]]}
    out["dataset_over_prebuilt"] = round(out["dataset"]["steps_per_s"] / out["prebuilt"]["steps_per_s"], 3)
    out["dataset_over_prebuilt_augmented"] = round(out["dataset"]["steps_per_s"] / out["prebuilt_augmented"]["steps_per_s"], 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--recordings", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--fit-steps", type=int, default=50)
    ap.add_argument("--fit-reps", type=int, default=5)
    ap.add_argument("--parts", default="crops,kernel,fit")
    args = ap.parse_args()
    parts = [p for p in args.parts.split(",") if p]
    if any(p not in ("crops", "kernel", "fit") for p in parts):
        ap.error("--parts takes crops, kernel, fit")
    if args.recordings < 1 or args.seconds < 2 * SEGMENT + 1:
        ap.error("at least one recording of at least 7 s")
    if not torch.cuda.is_available():
        raise SystemExit("dataset_bench needs a GPU: nothing here is measured on the host alone")
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    assert cfg["dataset"]["segment_duration"] == SEGMENT and cfg["dataloader"]["batch_size"] == CLIPS
    out = {"metric": "training batches from a device-resident dataset", "recordings": args.recordings, "seconds": args.seconds, "reps": args.reps}
    with tempfile.TemporaryDirectory() as tmp:
        root = Path(tmp)
        ids = write_data_dir(root, args.recordings, args.seconds)
        if "crops" in parts:
            out["crops"] = part_crops(root, ids, cfg, args.reps, args.warmup)
        if "kernel" in parts:
            out["kernel"] = part_kernel(root, ids, cfg, args.reps, args.warmup)
        if "fit" in parts:
            out["fit"] = part_fit(root, cfg, args.fit_steps, args.fit_reps)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
