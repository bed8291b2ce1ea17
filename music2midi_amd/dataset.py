"""The training dataset and its data module, with the recordings' sample bytes resident on the device.

ref: music2midi/dataset.py:15-167 - ``Music2MIDIDataset.__getitem__`` draws a segment of one recording, keeps it when it holds
1..``max_notes_per_second * segment_duration`` notes, loads and resamples that segment from the file, cuts and shifts the notes,
then normalises with probability 1/2 and transposes by ``randint(-6, 6)`` semitones; a ``DataLoader`` collates the items.  Here the
same data directory is read without librosa, joblib, OmegaConf or Lightning:

    data_dir/dataset_split.npz     train_id, val_id (allow_pickle=True)
    data_dir/audio/{id}.wav        RIFF/WAVE
    data_dir/midi_numpy/{id}.npy   [n, 4]: onset, offset, pitch, velocity
    data_dir/metadata/{id}.yaml    piano.genre, piano.difficulty, ... -> cond_index through config.conditioning, in its key order

    get_notes_segment(notes, start, end, shift_to_start_time=False)
    Music2MIDIDataset(data_dir, piano_ids, config_path, device=None, resident_bytes=None)
        .draw(indices, rng) -> (start_times, normalize, n_steps)      the reference's draws, in its order, from a np.random.Generator
        .crop_host(indices, start_times) -> np.float32 [B, T]         THE DEFINITION of a batch's audio
        .crop_device(indices, start_times) -> cuda fp32 [B, T]        one kernel (csrc/dataset.hip), the same samples bit for bit
        .batch(indices, rng, augment=True, device_crop=None) -> ModelInputs
    Music2MIDIDataModule(data_dir, config_path="config.yaml", device=None, resident_bytes=None)
        .setup(); .train_batches(rng, epochs=1); .val_batches(rng)    iterables of ModelInputs for Music2MIDI.fit_batches

A clip is resampled ON ITS OWN: the recording's frames before and behind ``[first, first + count)`` do not exist for the filter, as
with ``librosa.load(offset=, duration=)`` and ``ingest.load_audio_device(offset=, duration=)``.

With a device, every recording the kernel takes is uploaded once (its ``data`` chunk as one uint8 tensor) until ``resident_bytes``
is spent; the rest of those are *streamed* - per batch only the bytes of the drawn slices go through one pinned buffer and one copy -
and the same kernel reads them.  What the kernel does not take (``ingest.eligible`` says no, a rate ratio whose tile window exceeds
the kernel's LDS window, a segment of 2^31 bytes or more) is cropped by ``crop_host`` and uploaded into its row.  That routing is
decided per recording at construction and reported by ``residency()``; it is not a fallback for a missing kernel: without the
library ``crop_device`` raises ``native.NativeError``.

Stated differences from the reference: the draws come from a ``np.random.Generator`` instead of numpy's legacy global state, and
the epoch order is ``rng.permutation`` instead of torch's ``RandomSampler``; a recording without a candidate segment, without an
acceptable one, or whose segment resamples to another length than the others' raises ``ValueError`` at construction, naming the id
(the reference raises inside ``choice``, loops forever, fails in ``torch.stack``); ``num_workers`` is ignored.
"""
from __future__ import annotations

import ctypes as C
import mmap
from collections import Counter
from fractions import Fraction
from math import gcd
from pathlib import Path
from typing import Iterable, Iterator, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
import yaml

from . import audio, native
from .config import load_config
from .input import ModelInputs

MAX_CLIPS = 65535                        # M2M_DATASET_MAX_CLIPS
LDS_WINDOW = 4096                        # M2M_DATASET_LDS_WINDOW
MAX_SEGMENT_BYTES = (1 << 31) - 1


def get_notes_segment(notes: np.ndarray, start_time: float, end_time: float, shift_to_start_time: bool = False) -> np.ndarray:
    """ref: music2midi/dataset.py:145-154 - the notes whose onset lies in ``[start_time, end_time)``, as a float64 copy (the boolean
    mask copies in the reference too); with ``shift_to_start_time`` the onset and offset columns are moved by ``-start_time``."""
    notes = np.asarray(notes, dtype=np.float64).reshape(-1, 4)
    ret = notes[(notes[:, 0] >= start_time) & (notes[:, 0] < end_time)]
    if shift_to_start_time:
        ret[:, :2] -= start_time
    return ret


class Residency(NamedTuple):
    """The ids of a dataset's recordings by the way their audio reaches a batch."""
    resident: list
    streamed: list
    host: list


def _host_ratio(rate: float, sr: float) -> Tuple[int, int]:
    """(up, down) as ``audio.resample`` picks them; (1, 1) for equal rates."""
    if rate == sr:
        return 1, 1
    frac = Fraction(float(sr) / float(rate)).limit_denominator(1000)
    up, down = frac.numerator, frac.denominator
    g = gcd(up, down)
    return (up // g, down // g) if g else (up, down)


class _Recording:
    """One recording: what its RIFF header says, the segment's extent in frames, and where its sample bytes are."""

    def __init__(self, piano_id: str, path: str, sr: float, segment_duration: float):
        self.id, self.path = piano_id, path
        with open(path, "rb") as f:
            try:
                raw = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
            except ValueError:                               # an empty file cannot be mapped
                raw = b""
            try:
                lay = audio.wav_layout(path, raw)
            finally:
                if raw:
                    raw.close()
        self.kind = audio.wav_sample_format(path, lay.tag, lay.bits)
        self.rate, self.n_ch, self.width, self.data_offset = lay.rate, lay.n_ch, lay.bits // 8, lay.data_offset
        self.frame_bytes = self.width * self.n_ch
        self.frames = lay.data_size // self.frame_bytes
        self.duration = self.frames / self.rate              # librosa.get_duration(path=) of a WAVE file
        self.count = int(segment_duration * self.rate)       # frames of a segment, as load_audio_device counts them
        self.up, self.down = _host_ratio(self.rate, sr)
        self.n_out = self.count if self.rate == sr else -(-self.count * self.up // self.down)
        self.route = "host"
        self.body: Optional[torch.Tensor] = None             # resident: the data chunk on the device
        self.map = None                                      # streamed: the file, mapped
        self.bytes: Optional[np.ndarray] = None              # streamed: the data chunk, a view of the mapping

    def first(self, start_time: float) -> int:
        first = int(start_time * self.rate)
        if first < 0 or first + self.count > self.frames:
            raise ValueError(f"{self.id}: a segment at {start_time} s needs frames {first}..{first + self.count} of {self.frames}")
        return first


class Music2MIDIDataset:
    """ref: music2midi/dataset.py:81-142, by batches instead of items (see the module's docstring).

    ``device``: a CUDA device, or ``None`` for a host-only dataset (``crop_host``; the augmentation of ``batch`` then runs through
    the host definitions of ``music2midi_amd.audio``).  ``resident_bytes``: how many bytes of sample data may stay on the device;
    ``None`` takes every recording, otherwise recordings go in, in the order of ``piano_ids``, until the first that no longer fits;
    that one and those behind it are streamed."""

    def __init__(self, data_dir, piano_ids: Sequence[str], config_path, device=None, resident_bytes: Optional[int] = None):
        self.config = load_config(config_path)
        self.data_dir = Path(data_dir)
        self.piano_ids = [str(p) for p in piano_ids]
        ds = self.config.dataset
        self.segment_duration = ds.segment_duration
        self.sample_rate = ds.sample_rate
        self.max_num_notes = ds.max_notes_per_second * self.segment_duration
        key_dict = {key: {item: i for i, item in enumerate(self.config.conditioning.get(key))} for key in self.config.conditioning.keys()}
        self.audio_paths = [str(self.data_dir / "audio" / f"{p}.wav") for p in self.piano_ids]
        self.midi_notes = [np.asarray(np.load(self.data_dir / "midi_numpy" / f"{p}.npy"), dtype=np.float64).reshape(-1, 4)
                           for p in self.piano_ids]
        self.cond_indices = []
        for p in self.piano_ids:
            with open(self.data_dir / "metadata" / f"{p}.yaml", "r") as f:
                meta = yaml.safe_load(f)
            self.cond_indices.append([v[meta["piano"][k]] for k, v in key_dict.items()])
        self._recordings = [_Recording(p, path, self.sample_rate, self.segment_duration)
                            for p, path in zip(self.piano_ids, self.audio_paths)]
        self._candidates, self._acceptable = [], []
        for rec, notes in zip(self._recordings, self.midi_notes):
            cand = np.arange(0, rec.duration - self.segment_duration, self.segment_duration)
            if len(cand) == 0:
                raise ValueError(f"{rec.id}: {rec.duration} s hold no segment of {self.segment_duration} s "
                                 f"(the grid arange(0, duration - segment, segment) is empty)")
            ok = np.array([0 < len(get_notes_segment(notes, s, s + self.segment_duration)) <= self.max_num_notes for s in cand])
            if not ok.any():
                raise ValueError(f"{rec.id}: none of its {len(cand)} segments holds 1..{self.max_num_notes} notes")
            self._candidates.append(cand)
            self._acceptable.append(ok)
        # the common resampled length: the one most recordings have (the first's on a tie); torch.stack needs one
        lengths = Counter(rec.n_out for rec in self._recordings)
        best = max(lengths.values())
        self.segment_samples = next(rec.n_out for rec in self._recordings if lengths[rec.n_out] == best) if self._recordings else 0
        for rec in self._recordings:
            if rec.n_out != self.segment_samples:
                raise ValueError(f"{rec.id}: a {self.segment_duration} s segment at {rec.rate} Hz resamples to {rec.n_out} samples, "
                                 f"the other recordings' to {self.segment_samples}")
        self.device = None
        if device is not None:
            from . import ingest
            self.device = ingest._cuda_device(device)
            self._make_resident(resident_bytes)

    # ------------------------------------------------------------------ the reference's surface
    def __len__(self) -> int:
        return len(self._recordings)

    def duration(self, i: int) -> float:
        """Frames / rate from the RIFF header: ``librosa.get_duration(path=)`` of a WAVE file."""
        return self._recordings[i].duration

    def candidates(self, i: int) -> np.ndarray:
        """The reference's grid of start times, ``np.arange(0, duration - segment_duration, segment_duration)``."""
        return self._candidates[i]

    def acceptable(self, i: int) -> np.ndarray:
        """Per candidate: ``0 < len(get_notes_segment(...)) <= max_notes_per_second * segment_duration``."""
        return self._acceptable[i]

    def residency(self) -> Residency:
        by = {"resident": [], "streamed": [], "host": []}
        for rec in self._recordings:
            by[rec.route].append(rec.id)
        return Residency(**by)

    # ------------------------------------------------------------------ residency
    def _make_resident(self, budget: Optional[int]) -> None:
        from . import ingest
        lib = native.load()
        left = None if budget is None else int(budget)
        for rec in self._recordings:
            if not ingest.eligible(rec.path, self.sample_rate):
                continue
            if rec.up != rec.down and lib.m2m_dataset_crop_window(rec.up, rec.down) > LDS_WINDOW:
                continue
            if rec.count * rec.frame_bytes > MAX_SEGMENT_BYTES:
                continue
            n_bytes = rec.frames * rec.frame_bytes
            f = open(rec.path, "rb")
            try:
                if left is None or n_bytes <= left:
                    # a private mapping is writable without touching the file, which lets torch wrap the pages without a copy
                    raw = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_COPY)
                    with torch.cuda.device(self.device):
                        rec.body = torch.from_numpy(np.frombuffer(raw, np.uint8, n_bytes, rec.data_offset)).to(self.device)
                    del raw
                    rec.route = "resident"
                    if left is not None:
                        left -= n_bytes
                else:
                    left = 0                                 # the budget is spent: everything behind is streamed as well
                    rec.map = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
                    rec.bytes = np.frombuffer(rec.map, np.uint8, n_bytes, rec.data_offset)
                    rec.route = "streamed"
            finally:
                f.close()
            if rec.up != rec.down:
                ingest._filter_on(self.device, rec.up, rec.down)          # designed and uploaded once per ratio
        torch.cuda.current_stream(self.device).synchronize()                # the uploads: any stream may read them from here on

    def resident_bytes(self) -> int:
        """Bytes of sample data this dataset keeps on the device."""
        return sum(int(rec.body.numel()) for rec in self._recordings if rec.body is not None)

    # ------------------------------------------------------------------ draws
    def draw(self, indices: Iterable[int], rng: np.random.Generator) -> Tuple[list, list, list]:
        """The reference's draws per clip (ref dataset.py:110-132), in batch order and in its order: ``rng.choice(candidates)``
        until an acceptable segment comes up, then ``rng.random() < 0.5`` (normalise), then ``rng.integers(-6, 6)`` (semitones) -
        the last two as ``augment.draw`` makes them.  Returns ``(start_times, normalize, n_steps)``."""
        start_times, normalize, n_steps = [], [], []
        for i in indices:
            cand, ok = self._candidates[int(i)], self._acceptable[int(i)]
            while True:
                start = rng.choice(cand)
                if ok[int(np.flatnonzero(cand == start)[0])]:
                    break
            start_times.append(float(start))
            normalize.append(bool(rng.random() < 0.5))
            n_steps.append(int(rng.integers(-6, 6)))
        return start_times, normalize, n_steps

    # ------------------------------------------------------------------ audio
    def crop_host(self, indices: Sequence[int], start_times: Sequence[float]) -> np.ndarray:
        """THE DEFINITION: per clip ``read_wav(path)[0][first:first + count]`` with ``first = int(start * rate)`` and
        ``count = int(segment_duration * rate)``, averaged over the channels as ``audio.load_audio`` averages, then
        ``audio.resample`` of that slice alone to ``config.dataset.sample_rate``.  float32 [B, T]."""
        out = np.zeros((len(indices), self.segment_samples), dtype=np.float32)
        for b, (i, start) in enumerate(zip(indices, start_times)):
            rec = self._recordings[int(i)]
            first = rec.first(start)
            y, rate = audio.read_wav(rec.path)
            y = y[first:first + rec.count].mean(axis=1)
            out[b] = audio.resample(y, rate, self.sample_rate).astype(np.float32)
        return out

    def crop_device(self, indices: Sequence[int], start_times: Sequence[float]) -> torch.Tensor:
        """``crop_host`` as a CUDA fp32 [B, T] tensor, bit for bit, enqueued on the current stream: one descriptor table, one
        launch of csrc/dataset.hip over the resident and the streamed clips (the streamed slices go through one pinned buffer and
        one copy first); rows of recordings the kernel does not take come from ``crop_host``."""
        if self.device is None:
            raise ValueError("crop_device: this dataset was built without a device")
        from . import ingest
        indices = [int(i) for i in indices]
        if len(indices) != len(start_times):
            raise ValueError(f"crop_device: {len(indices)} indices for {len(start_times)} start times")
        B, T, dev = len(indices), self.segment_samples, self.device
        recs = [self._recordings[i] for i in indices]
        firsts = [rec.first(s) for rec, s in zip(recs, start_times)]
        on_device = [b for b in range(B) if recs[b].route != "host"]
        on_host = [b for b in range(B) if recs[b].route == "host"]
        if len(on_device) > MAX_CLIPS:
            raise ValueError(f"crop_device: {len(on_device)} clips in one call (the kernel takes {MAX_CLIPS})")
        with torch.cuda.device(dev):
            out = torch.empty((B, T), dtype=torch.float32, device=dev)
            if on_device:
                # the streamed slices: gathered into one pinned buffer (each at a multiple of 8 bytes), one copy
                at, total = {}, 0
                for b in on_device:
                    if recs[b].route == "streamed":
                        at[b] = total
                        total += -(-recs[b].count * recs[b].frame_bytes // 8) * 8
                stage = None
                if total:
                    pinned = torch.empty(total, dtype=torch.uint8, pin_memory=True)
                    view = pinned.numpy()
                    for b, o in at.items():
                        rec, n_bytes = recs[b], recs[b].count * recs[b].frame_bytes
                        view[o:o + n_bytes] = rec.bytes[firsts[b] * rec.frame_bytes:firsts[b] * rec.frame_bytes + n_bytes]
                    stage = pinned.to(dev, non_blocking=True)
                clips = (native.DatasetClip * len(on_device))()
                for clip, b in zip(clips, on_device):
                    rec = recs[b]
                    clip.bytes_dev = (stage.data_ptr() + at[b]) if b in at else rec.body.data_ptr() + firsts[b] * rec.frame_bytes
                    clip.h_phase_dev = None if rec.up == rec.down else ingest._filter_on(dev, rec.up, rec.down).data_ptr()
                    clip.n_frames, clip.channels, clip.format = rec.count, rec.n_ch, ingest.FORMATS[rec.kind][0]
                    clip.up, clip.down, clip.half, clip.reserved = rec.up, rec.down, 10 * max(rec.up, rec.down), 0
                table = torch.empty(C.sizeof(clips), dtype=torch.uint8, device=dev)
                rows = out if not on_host else torch.empty((len(on_device), T), dtype=torch.float32, device=dev)
                native.check(native.load().m2m_dataset_crop_f32(clips, len(on_device), table.data_ptr(), rows.data_ptr(), rows.stride(0), T,
                                                                native.stream_handle(dev)), "m2m_dataset_crop_f32")
                if on_host:
                    out.index_copy_(0, torch.tensor(on_device, device=dev), rows)
            if on_host:
                host = self.crop_host([indices[b] for b in on_host], [start_times[b] for b in on_host])
                out.index_copy_(0, torch.tensor(on_host, device=dev), torch.from_numpy(host).to(dev))
        return out

    # ------------------------------------------------------------------ batches
    def batch(self, indices: Sequence[int], rng: np.random.Generator, augment: bool = True, device_crop: Optional[bool] = None) -> ModelInputs:
        """The reference's items of ``indices``, collated (ref dataset.py:102-139, 163-167): draw, crop, notes segment, then - with
        ``augment`` - ``augment.transpose_batch(inputs, n_steps, normalize)``.  ``device_crop``: ``crop_device`` or ``crop_host``
        (uploaded when the dataset has a device); ``None`` means the device whenever the dataset has one.  ``notes_batch`` is a
        tuple of host float64 arrays as the reference's ``collate_fn`` leaves them, ``cond_index`` a long tensor [B, n_cond] (on the
        dataset's device when it has one)."""
        indices = [int(i) for i in indices]
        start_times, normalize, n_steps = self.draw(indices, rng)
        on_device = (self.device is not None) if device_crop is None else bool(device_crop)
        if on_device:
            waveform = self.crop_device(indices, start_times)
        else:
            waveform = torch.from_numpy(self.crop_host(indices, start_times))
            if self.device is not None:
                waveform = waveform.to(self.device)
        notes = tuple(get_notes_segment(self.midi_notes[i], s, s + self.segment_duration, shift_to_start_time=True)
                      for i, s in zip(indices, start_times))
        cond = torch.tensor([self.cond_indices[i] for i in indices], dtype=torch.long).reshape(len(indices), -1)
        if self.device is not None:
            # next to the waveform, through pinned memory: a pageable copy inside the step would make the host wait for the stream
            cond = cond.pin_memory().to(self.device, non_blocking=True)
        inputs = ModelInputs(input_waveform=waveform, notes_batch=notes, cond_index=cond)
        if not augment:
            return inputs
        if waveform.is_cuda:
            from .augment import transpose_batch
            return transpose_batch(inputs, n_steps, normalize)
        # a host-only dataset: the host definitions, clip by clip, in the reference's order
        waves, shifted = [], []
        for y, n, step, norm in zip(waveform.numpy(), notes, n_steps, normalize):
            y, n = audio.transpose(audio.normalize(y) if norm else y, n, step, self.sample_rate)
            waves.append(y)
            shifted.append(n)
        return ModelInputs(input_waveform=torch.from_numpy(np.stack(waves)), notes_batch=tuple(shifted), cond_index=cond)


class Music2MIDIDataModule:
    """ref: music2midi/dataset.py:42-78 without Lightning: ``setup()`` builds the train and the validation set from
    ``data_dir/dataset_split.npz``; ``train_batches`` / ``val_batches`` are what the two ``DataLoader``s yield, as iterables of
    ``ModelInputs`` for ``Music2MIDI.fit_batches``.  The batch size is ``config.dataloader.batch_size``, the last batch may be
    partial (``drop_last`` is False), ``num_workers`` is ignored.  The epoch order of the training set is one
    ``rng.permutation(len)`` per epoch - a ``Generator`` permutation, NOT torch's ``RandomSampler`` - and the validation set goes
    in order; both sets draw their segments and augmentations from the same ``rng``, as both are the reference's one Dataset class.
    ``resident_bytes`` is the budget of the training set; the validation set gets what that leaves."""

    def __init__(self, data_dir, config_path="config.yaml", device=None, resident_bytes: Optional[int] = None):
        self.config_path = config_path
        self.config = load_config(config_path)
        self.data_dir = Path(data_dir)
        self.device, self.resident_bytes = device, resident_bytes
        self.dataset_split_ids = np.load(self.data_dir / "dataset_split.npz", allow_pickle=True)
        self.train_set: Optional[Music2MIDIDataset] = None
        self.val_set: Optional[Music2MIDIDataset] = None

    def setup(self, stage=None) -> None:
        self.train_set = Music2MIDIDataset(self.data_dir, list(self.dataset_split_ids["train_id"]), self.config_path, self.device,
                                           self.resident_bytes)
        left = None if self.resident_bytes is None else max(0, int(self.resident_bytes) - self.train_set.resident_bytes())
        self.val_set = Music2MIDIDataset(self.data_dir, list(self.dataset_split_ids["val_id"]), self.config_path, self.device, left)

    def _batches(self, dataset: Music2MIDIDataset, order: np.ndarray, rng: np.random.Generator) -> Iterator[ModelInputs]:
        size = int(self.config.dataloader.batch_size)
        for lo in range(0, len(order), size):
            yield dataset.batch([int(i) for i in order[lo:lo + size]], rng)

    def train_batches(self, rng: np.random.Generator, epochs: int = 1, indices: Optional[Sequence[int]] = None) -> Iterator[ModelInputs]:
        """``epochs`` passes over the training set (or over ``indices`` of it: a rank's shard), each in a fresh permutation."""
        if self.train_set is None:
            self.setup()
        pool = np.arange(len(self.train_set)) if indices is None else np.asarray(list(indices), dtype=np.int64)
        for _ in range(int(epochs)):
            yield from self._batches(self.train_set, pool[rng.permutation(len(pool))], rng)

    def val_batches(self, rng: np.random.Generator, indices: Optional[Sequence[int]] = None) -> Iterator[ModelInputs]:
        if self.val_set is None:
            self.setup()
        pool = np.arange(len(self.val_set)) if indices is None else np.asarray(list(indices), dtype=np.int64)
        yield from self._batches(self.val_set, pool, rng)
