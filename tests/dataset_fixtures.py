"""Tiny data directories in the reference's layout (dataset_split.npz, audio/, midi_numpy/, metadata/) for the dataset tests."""
import copy

import numpy as np
import yaml

from music2midi_amd.config import DEFAULT_CONFIG

from wav_fixtures import wav_bytes


def config(segment_duration=0.5, batch_size=2, **dataset):
    """The default configuration with the tests' dataset settings: 0.5 s segments at 22 050 Hz, at most 30 notes per second."""
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["dataset"].update(segment_duration=segment_duration, sample_rate=22050, max_notes_per_second=30, **dataset)
    cfg["dataloader"]["batch_size"] = batch_size
    return cfg


def signal(n, seed, rate, scale=0.9):
    """Noise plus two sines, as the ingest tests use."""
    t = np.arange(n) / rate
    y = 0.25 * np.random.default_rng(seed).standard_normal(n) + 0.2 * np.sin(2 * np.pi * 440 * t) + 0.15 * np.sin(2 * np.pi * 1318.5 * t)
    return (scale * y).astype(np.float32)


def encode(chans, kind):
    """float [n, n_ch] in [-1, 1] -> (format tag, bits, interleaved bytes) of one of read_wav's sample formats."""
    chans = np.asarray(chans, dtype=np.float64).clip(-1, 1)
    if kind == "u8":
        return 1, 8, np.round(chans * 127 + 128).astype(np.uint8).tobytes()
    if kind == "s16":
        return 1, 16, np.round(chans * 32767).astype("<i2").tobytes()
    if kind == "s24":
        v = np.round(chans * 8388607).astype(np.int32)
        return 1, 24, (v & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    if kind == "s32":
        return 1, 32, np.round(chans * 2147483647).astype("<i4").tobytes()
    if kind == "f32":
        return 3, 32, chans.astype("<f4").tobytes()
    return 3, 64, chans.astype("<f8").tobytes()


def wav(kind, n_ch, rate, seconds, seed, before_data=b"", mono=None):
    """A RIFF/WAVE file's bytes: `mono` (default: signal()) at a different level in every channel."""
    y = signal(int(round(rate * seconds)), seed, rate) if mono is None else np.asarray(mono)
    chans = np.stack([y * (1.0 - 0.1 * c) for c in range(n_ch)], axis=1)
    tag, bits, body = encode(chans, kind)
    return wav_bytes(tag, n_ch, rate, bits, body, before_data=before_data)


def notes_with(counts, segment_duration):
    """[n, 4] notes with counts[k] onsets inside segment k of the grid; offsets 0.1 s later, pitches from 60, velocity 80."""
    rows = []
    for k, c in enumerate(counts):
        for j in range(c):
            onset = k * segment_duration + (j + 0.5) * segment_duration / (c + 1)
            rows.append([onset, onset + 0.1, 60 + (j % 12), 80])
    return np.asarray(rows, dtype=np.float64).reshape(-1, 4)


def add_recording(data_dir, piano_id, wav_file, notes, genre="pop", difficulty="beginner", difficulty_first=False):
    for sub in ("audio", "midi_numpy", "metadata"):
        (data_dir / sub).mkdir(parents=True, exist_ok=True)
    (data_dir / "audio" / f"{piano_id}.wav").write_bytes(wav_file)
    np.save(data_dir / "midi_numpy" / f"{piano_id}.npy", notes)
    piano = {"difficulty": difficulty, "genre": genre} if difficulty_first else {"genre": genre, "difficulty": difficulty}
    (data_dir / "metadata" / f"{piano_id}.yaml").write_text(yaml.safe_dump({"piano": piano}, sort_keys=False))


def write_split(data_dir, train_ids, val_ids):
    np.savez(data_dir / "dataset_split.npz", train_id=np.array(list(train_ids), dtype=object), val_id=np.array(list(val_ids), dtype=object))
