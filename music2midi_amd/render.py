"""Notes -> audio: a wavetable voice whose every sample is defined to the bit, on the host (numpy) and on the device (csrc/render.hip).

The reference's callers turn notes into sound through ``PrettyMIDI.fluidsynth`` (ref: webui.py:66, the preview next to the MIDI
file) and ``PrettyMIDI.synthesize`` (its data preparation); neither package is in the build image.  The timbre here is NOT a
SoundFont's: it is one built-in voice, chosen so that every per-sample step is integer arithmetic or ONE rounded fp32 operation and
no transcendental function is evaluated per sample.  The device therefore equals the host with ``np.array_equal``.

    Voice(fs, ...)                                                   everything that is computed once (float64, rounded once)
    pack(notes, fs, n_samples) -> Packed                             sample-grid notes, dropped and stably sorted
    render_host(notes, fs, n_samples=None, voice=None, normalize=False) -> np.float32 [n_samples]        THE DEFINITION
    render_batch_host(notes_batch, fs, n_samples) -> np.float32 [B, n_samples]
    tile_lists(packed_batch, n_samples, tile, release) -> (start [B * tiles + 1], entries)                the kernel's CSR
    device_lists(packed_batch, n_samples, voice), launch(lists, counts, voice, out)                       the two halves of render
    render(notes, fs, n_samples=None, voice=None, normalize=False, device=None) -> cuda fp32 [n_samples] or [B, n_samples]
    synthetic_batch(rng, B, config, voice=None, device=None) -> ModelInputs                               labelled clips, no dataset

The voice.  ``f_p = 440 * 2^((p - 69) / 12)``.
  wave   fp32 [harmonics][table_size + 1]: table m (row m - 1) is one period of ``sum_{h=1..m} sin(2 pi h k / table_size) / h``
         scaled to peak 1, plus a guard entry equal to entry 0.  Pitch p uses table ``min(harmonics, floor((fs/2 - 1) / f_p))``; a
         pitch with ``f_p >= fs/2`` (or no table: ``(fs/2 - 1) / f_p < 1``) is silent.
  inc    uint32 [128]: ``floor(f_p / fs * 2^32 + 0.5)``, the phase step per sample.
  decay  fp32 [J + 1]: ``exp(-j / 64)``;  dec  uint32 [128]: ``floor(64 / (tau_p fs) * 65536 + 0.5)``, decay steps per sample in
         units of 2^-16, ``tau_p = tau[0] * 2^(-(p - 21) / tau[1]) + tau[2]`` seconds.
  A = max(1, int(attack * fs)), R = max(1, int(release * fs)) samples; invA, invR their fp32 reciprocals;
  gain = fp32(0.25) * (fp32(velocity) / fp32(127)).

A sample.  For a packed note and output sample n in ``[max(on, 0), min(off + R, n_samples))``, ``k = n - on``:
  1. ``phase = (uint32)(k * inc[p])``; ``i = phase >> s``, ``fr = fp32(phase & (2^s - 1)) * 2^-s`` (exact; ``s = 32 - log2
     table_size``, 20 for 4096); ``w = W[i] + fr * (W[i + 1] - W[i])``: a subtract, a multiply, an add, each rounded.
  2. ``u = (uint64)k * dec[p]``; ``j = u >> 16``, ``ef = fp32(u & 0xFFFF) * 2^-16``; ``e = E[j] + ef * (E[j + 1] - E[j])``, and
     ``E[J]`` for ``j >= J``.
  3. ``att = fp32(min(k + 1, A)) * invA``; ``rel = 1`` for ``n < off``, else ``fp32(R - (n - off)) * invR``.
  4. ``s = (((w * e) * att) * rel) * gain``; ``y[n] = y[n] + s`` from +0, the notes in packed order.
``normalize=True`` divides by ``max |y|`` when that is positive: one fp32 division per sample (pretty_midi's ``fluidsynth``).
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np

MAX_SAMPLES = 1 << 28                    # n_samples of one call (M2M_RENDER_MAX_SAMPLES)
MAX_NOTES = 1 << 20                      # packed notes of one call, all clips together (M2M_RENDER_MAX_NOTES)
MAX_CLIPS = 65535                        # M2M_RENDER_MAX_CLIPS
MAX_RAMP = 1 << 24                       # A and R: fp32 holds every integer up to it
MIN_ON = -(1 << 30)                      # the earliest onset in samples: k = n - on stays below 2^31


def pitch_hz(p) -> np.ndarray:
    return 440.0 * 2.0 ** ((np.asarray(p, dtype=np.float64) - 69.0) / 12.0)


class Voice:
    """The tables and constants of the voice at sample rate ``fs``; see the module's docstring.  ``table_size`` is a power of two in
    256..65536 (the fraction of a phase must fit fp32's 24 bits).
    A voice that has rendered on a GPU keeps its two tables there (``_device``, by device index) for as long as it lives, and the
    voices of ``default_voice`` live as long as the process; ``copy.deepcopy`` and pickle leave those tensors behind
    (``__getstate__``), the copy uploads its own on first use."""

    def __init__(self, fs: float, table_size: int = 4096, harmonics: int = 6, tau: Tuple[float, float, float] = (3.0, 24.0, 0.2),
                 decay_steps: int = 1024, attack: float = 0.002, release: float = 0.05):
        fs = float(fs)
        if not fs > 0:
            raise ValueError(f"Voice: fs = {fs}")
        bits = int(table_size).bit_length() - 1
        if int(table_size) != 1 << bits or not 8 <= bits <= 16:
            raise ValueError(f"Voice: table_size = {table_size} is not a power of two in 256..65536")
        if not 1 <= int(harmonics) <= 64 or not 1 <= int(decay_steps) <= MAX_RAMP:
            raise ValueError(f"Voice: harmonics = {harmonics} (1..64), decay_steps = {decay_steps} (1..2^24)")
        self.fs, self.table_size, self.harmonics, self.tau, self.decay_steps = fs, int(table_size), int(harmonics), tuple(tau), int(decay_steps)
        self.shift = 32 - bits
        k = np.arange(self.table_size, dtype=np.float64)
        wave, acc = np.zeros((self.harmonics, self.table_size + 1), dtype=np.float32), np.zeros(self.table_size)
        for m in range(1, self.harmonics + 1):
            acc = acc + np.sin(2.0 * np.pi * m * k / self.table_size) / m
            wave[m - 1, :-1] = (acc / np.abs(acc).max()).astype(np.float32)
            wave[m - 1, -1] = wave[m - 1, 0]
        self.wave = wave
        f = pitch_hz(np.arange(128))
        with np.errstate(over="ignore"):
            self.table = np.minimum(self.harmonics, np.floor((fs / 2.0 - 1.0) / f)).astype(np.int64)       # 0: no table
        self.silent = (f >= fs / 2.0) | (self.table < 1)
        self.table = np.where(self.silent, 0, self.table)
        self.inc = np.where(self.silent, 0, np.floor(np.minimum(f / fs, 0.5) * 2.0 ** 32 + 0.5)).astype(np.uint32)
        self.decay = np.exp(-np.arange(self.decay_steps + 1, dtype=np.float64) / 64.0).astype(np.float32)
        tau_p = self.tau[0] * 2.0 ** (-(np.arange(128) - 21.0) / self.tau[1]) + self.tau[2]
        dec = np.floor(64.0 / (tau_p * fs) * 65536.0 + 0.5)
        if not (dec >= 0).all() or dec.max() >= 2.0 ** 32:
            raise ValueError(f"Voice: tau = {self.tau} at fs = {fs} gives decay steps outside uint32")
        self.dec = dec.astype(np.uint32)
        self.attack, self.release = max(1, int(attack * fs)), max(1, int(release * fs))
        if self.attack > MAX_RAMP or self.release > MAX_RAMP:
            raise ValueError(f"Voice: attack / release = {self.attack} / {self.release} samples, the limit is 2^24")
        self.inv_attack = np.float32(1.0) / np.float32(self.attack)
        self.inv_release = np.float32(1.0) / np.float32(self.release)
        self._device: dict = {}                              # device index -> (wave, decay) on that device

    def __getstate__(self) -> dict:
        return {**self.__dict__, "_device": {}}

    def gain(self, velocity) -> np.ndarray:
        return np.float32(0.25) * (np.asarray(velocity).astype(np.float32) / np.float32(127.0))

    def on_device(self, device):
        """(wave, decay) as CUDA tensors, uploaded once per device."""
        import torch
        got = self._device.get(device.index)
        if got is None:
            got = self._device.setdefault(device.index, (torch.from_numpy(self.wave).to(device), torch.from_numpy(self.decay).to(device)))
        return got


_default_voices: dict = {}


def default_voice(fs: float) -> Voice:
    v = _default_voices.get(float(fs))
    if v is None:
        v = _default_voices.setdefault(float(fs), Voice(fs))
    return v


class Packed(NamedTuple):
    """The notes of one clip on the sample grid, in the order they are added: int64 on / off, int64 pitch, fp32 gain, and
    ``index``, the row of the caller's array each came from."""
    on: np.ndarray
    off: np.ndarray
    pitch: np.ndarray
    gain: np.ndarray
    index: np.ndarray


def pack(notes, fs: float, n_samples: Optional[int] = None, voice: Optional[Voice] = None) -> Packed:
    """``on = floor(onset * fs + 0.5)``, ``off`` likewise (float64 -> int64).  Dropped: ``off <= on``, a silent pitch, no sample in
    ``[0, n_samples)`` (``n_samples=None``: no sample at or after 0).  The rest sorted stably by ``on``.  A negative ``on`` is legal
    down to -2^30: the note is already sounding when the clip begins."""
    voice = default_voice(fs) if voice is None else voice
    notes = np.asarray(notes, dtype=np.float64).reshape(-1, 4)
    if not np.isfinite(notes).all():
        raise ValueError("pack: a note holds NaN or infinity")
    on = np.floor(notes[:, 0] * float(fs) + 0.5).astype(np.int64)
    off = np.floor(notes[:, 1] * float(fs) + 0.5).astype(np.int64)
    pitch = notes[:, 2].astype(np.int64)
    if len(pitch) and (pitch.min() < 0 or pitch.max() > 127):
        raise ValueError(f"pack: pitches {pitch.min()}..{pitch.max()} outside 0..127")
    keep = (off > on) & ~voice.silent[pitch] & (off + voice.release > 0)
    if n_samples is not None:
        keep &= on < int(n_samples)
    if keep.any() and on[keep].min() < MIN_ON:
        raise ValueError(f"pack: an onset {on[keep].min()} samples before the clip (the limit is 2^30)")
    index = np.flatnonzero(keep)
    index = index[np.argsort(on[index], kind="stable")]
    return Packed(on[index], off[index], pitch[index], voice.gain(notes[index, 3]), index)


def _default_length(packed: Sequence[Packed], voice: Voice) -> int:
    return max([int(p.off.max()) + voice.release for p in packed if len(p.off)] + [0])


def _add_note(y: np.ndarray, v: Voice, on: int, off: int, p: int, gain: np.float32) -> None:
    lo, hi = max(on, 0), min(off + v.release, len(y))
    if hi <= lo:
        return
    f32 = np.float32
    n = np.arange(lo, hi, dtype=np.int64)
    k = n - on
    phase = (k.astype(np.uint64) * np.uint64(v.inc[p])) & np.uint64(0xFFFFFFFF)
    i = (phase >> np.uint64(v.shift)).astype(np.int64)
    fr = (phase & np.uint64((1 << v.shift) - 1)).astype(f32) * f32(2.0 ** -v.shift)
    W = v.wave[v.table[p] - 1]
    d = W[i + 1] - W[i]
    w = W[i] + fr * d
    u = k.astype(np.uint64) * np.uint64(v.dec[p])
    j = np.minimum(u >> np.uint64(16), np.uint64(v.decay_steps)).astype(np.int64)
    ef = (u & np.uint64(0xFFFF)).astype(f32) * f32(2.0 ** -16)
    j1 = np.minimum(j + 1, v.decay_steps)
    e = np.where(j >= v.decay_steps, v.decay[v.decay_steps], v.decay[j] + ef * (v.decay[j1] - v.decay[j]))
    att = np.minimum(k + 1, v.attack).astype(f32) * v.inv_attack
    rel = np.where(n < off, f32(1.0), (v.release - (n - off)).astype(f32) * v.inv_release)
    s = (((w * e) * att) * rel) * f32(gain)
    assert s.dtype == np.float32
    y[lo:hi] = y[lo:hi] + s


def _normalize(y: np.ndarray) -> np.ndarray:
    peak = np.abs(y).max(axis=-1, keepdims=True) if y.shape[-1] else np.zeros(y.shape[:-1] + (1,), np.float32)
    return np.where(peak > 0, y / np.where(peak > 0, peak, np.float32(1.0)), y).astype(np.float32)


def render_host(notes, fs: float, n_samples: Optional[int] = None, voice: Optional[Voice] = None, normalize: bool = False) -> np.ndarray:
    """THE DEFINITION (the module's docstring): float32 [n_samples]; ``n_samples=None`` is the last ``off + R``."""
    voice = default_voice(fs) if voice is None else voice
    packed = pack(notes, fs, n_samples, voice)
    if n_samples is None:
        n_samples = _default_length([packed], voice)
    y = np.zeros(int(n_samples), dtype=np.float32)
    for on, off, p, g in zip(packed.on.tolist(), packed.off.tolist(), packed.pitch.tolist(), packed.gain):
        _add_note(y, voice, on, off, p, g)
    return _normalize(y) if normalize else y


def render_batch_host(notes_batch, fs: float, n_samples: int, voice: Optional[Voice] = None, normalize: bool = False) -> np.ndarray:
    """``render_host`` per clip: float32 [B, n_samples]."""
    return np.stack([render_host(n, fs, n_samples, voice, normalize) for n in notes_batch]).reshape(len(notes_batch), int(n_samples))


# ------------------------------------------------------------------ the device
def tile_lists(packed_batch: Sequence[Packed], n_samples: int, tile: int, release: int) -> Tuple[np.ndarray, np.ndarray]:
    """Which notes touch which tile, as a CSR over ``(clip, tile)``: ``start`` int32 [B * tiles + 1] and ``entries`` int32, the
    indices into the clips' packed notes CONCATENATED, in note order inside a tile.  A note touches the tiles
    ``max(on, 0) // tile .. (min(off + release, n_samples) - 1) // tile``."""
    tiles = -(-int(n_samples) // tile)
    B = len(packed_batch)
    on = np.concatenate([p.on for p in packed_batch]) if B else np.zeros(0, np.int64)
    off = np.concatenate([p.off for p in packed_batch]) if B else np.zeros(0, np.int64)
    clip = np.repeat(np.arange(B, dtype=np.int64), [len(p.on) for p in packed_batch])
    first = np.maximum(on, 0) // tile
    last = (np.minimum(off + release, int(n_samples)) - 1) // tile
    count = last - first + 1
    assert (count >= 1).all(), "tile_lists: a packed note without a sample in the clip"
    total = int(count.sum())
    if total >= 1 << 31:
        raise ValueError(f"tile_lists: {total} (note, tile) pairs, the limit is 2^31 - 1")
    note = np.repeat(np.arange(len(on), dtype=np.int64), count)
    slot = np.repeat(clip * tiles + first - (np.cumsum(count) - count), count) + np.arange(total, dtype=np.int64)
    # by slot, note order kept inside a slot: the keys slot * 2^20 + note are distinct (at most 2^20 notes), so a plain sort does it
    assert len(on) <= MAX_NOTES
    key = np.sort((slot << 20) | note)
    start = np.zeros(B * tiles + 1, dtype=np.int64)
    np.cumsum(np.bincount(slot, minlength=B * tiles), out=start[1:])
    return start.astype(np.int32), (key & (MAX_NOTES - 1)).astype(np.int32)


def tile_size() -> int:
    from . import native
    return int(native.load().m2m_render_tile())


def _as_batch(notes) -> Tuple[list, bool]:
    """(the clips' note arrays, whether the caller gave a list of them): a list or tuple of numpy arrays is a batch."""
    if isinstance(notes, (list, tuple)) and all(isinstance(n, np.ndarray) for n in notes):
        return [np.asarray(n, dtype=np.float64).reshape(-1, 4) for n in notes], True
    return [np.asarray(notes, dtype=np.float64).reshape(-1, 4)], False


def device_lists(packed_batch: Sequence[Packed], n_samples: int, voice: Voice) -> Tuple[np.ndarray, Tuple[int, int, int]]:
    """What one launch reads, as ONE int32 buffer for one copy: the note records (six words each: on, min(off, n_samples), inc,
    dec, table row, the gain's bits - ``m2m_render_note``), the tile starts, the entries; and the three counts."""
    start, entries = tile_lists(packed_batch, n_samples, tile_size(), voice.release)
    n_notes = sum(len(p.on) for p in packed_batch)
    rec = np.zeros((n_notes, 6), dtype=np.int32)
    if n_notes:
        pitch = np.concatenate([p.pitch for p in packed_batch])
        rec[:, 0] = np.concatenate([p.on for p in packed_batch])
        rec[:, 1] = np.minimum(np.concatenate([p.off for p in packed_batch]), n_samples)  # rel = 1 for every n < n_samples either way
        rec[:, 2] = voice.inc[pitch].view(np.int32)
        rec[:, 3] = voice.dec[pitch].view(np.int32)
        rec[:, 4] = voice.table[pitch] - 1
        rec[:, 5] = np.concatenate([p.gain for p in packed_batch]).astype(np.float32).view(np.int32)
    return np.concatenate([rec.reshape(-1), start, entries]), (n_notes, len(start), len(entries))


def launch(lists, counts: Tuple[int, int, int], voice: Voice, out) -> None:
    """``m2m_render_notes_f32`` on ``lists`` (``device_lists`` as a CUDA tensor) into ``out``, fp32 [B, n_samples] with unit column
    stride, on the current stream of its device.  Copies nothing and waits for nothing."""
    import torch
    from . import native
    dev = out.device
    n_notes, n_start, n_entries = counts
    if out.dim() != 2 or out.dtype != torch.float32 or not out.is_cuda or (out.shape[1] > 1 and out.stride(1) != 1):
        raise ValueError(f"render: out is {tuple(out.shape)} {out.dtype} on {dev}, wanted CUDA fp32 [B, n_samples] with unit column stride")
    B, n_samples = int(out.shape[0]), int(out.shape[1])
    wave, decay = voice.on_device(dev)
    vs = native.RenderVoice(wave_dev=wave.data_ptr(), decay_dev=decay.data_ptr(), table_size=voice.table_size, n_tables=voice.harmonics,
                            decay_steps=voice.decay_steps, attack=voice.attack, release=voice.release, reserved=0)
    base = lists.data_ptr()
    native.check(native.load().m2m_render_notes_f32(base if n_notes else None, n_notes, base + 24 * n_notes, base + 24 * n_notes + 4 * n_start,
                                                    n_entries, C.byref(vs), out.data_ptr(), n_samples, out.stride(0) if B > 1 else n_samples, B,
                                                    native.stream_handle(dev)), "m2m_render_notes_f32")


def render(notes, fs: float, n_samples: Optional[int] = None, voice: Optional[Voice] = None, normalize: bool = False, device=None):
    """``render_host`` on the device, bit for bit, enqueued on the current stream: fp32 CUDA tensor [n_samples] for one [n, 4]
    array, [B, n_samples] for a list of them (one launch for the batch).  ``n_samples=None``: the last ``off + R`` of the batch.
    A CPU ``device`` returns the definition's result as a CPU tensor.  (Rows with a stride of their own: ``device_lists`` and
    ``launch``.)"""
    import torch
    voice = default_voice(fs) if voice is None else voice
    batch, is_batch = _as_batch(notes)
    dev = torch.device("cuda" if device is None else device)
    packed = [pack(n, fs, n_samples, voice) for n in batch]
    if n_samples is None:
        n_samples = _default_length(packed, voice)
    n_samples, B = int(n_samples), len(batch)
    if dev.type != "cuda":
        y = np.stack([render_host(n, fs, n_samples, voice, normalize) for n in batch]) if B else np.zeros((0, n_samples), np.float32)
        return torch.from_numpy(y if is_batch else y[0])
    dev = torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)
    if n_samples == 0 or B == 0:
        return torch.zeros((B, n_samples) if is_batch else (n_samples,), dtype=torch.float32, device=dev)
    n_notes = sum(len(p.on) for p in packed)
    if n_samples > MAX_SAMPLES or B > MAX_CLIPS or n_notes > MAX_NOTES:
        raise ValueError(f"render: {n_samples} samples (1..2^28), {B} clips (1..65535), {n_notes} notes (..2^20)")
    words, counts = device_lists(packed, n_samples, voice)
    with torch.cuda.device(dev):
        lists = torch.from_numpy(words).pin_memory().to(dev, non_blocking=True)
        out = torch.empty((B, n_samples), dtype=torch.float32, device=dev)
        launch(lists, counts, voice, out)
        if normalize:
            peak = out.abs().amax(dim=1, keepdim=True)
            out = torch.where(peak > 0, out / torch.where(peak > 0, peak, torch.ones_like(peak)), out)
    return out if is_batch else out[0]


# ------------------------------------------------------------------ labelled clips without a dataset
SYNTHETIC_MAX_NOTES = 90


def synthetic_notes(rng: np.random.Generator, duration: float) -> np.ndarray:
    """One clip's notes, float64 [n, 4] sorted by onset.  The draws, in this order: ``n = rng.integers(1, 91)``;
    ``onset = rng.uniform(0, duration, n)``; ``length = rng.uniform(0.05, 1.0, n)``; ``pitch = rng.integers(21, 109, n)``;
    ``velocity = rng.integers(40, 128, n)``.  ``offset = min(onset + length, duration)``."""
    n = int(rng.integers(1, SYNTHETIC_MAX_NOTES + 1))
    onset = rng.uniform(0.0, duration, n)
    length = rng.uniform(0.05, 1.0, n)
    pitch = rng.integers(21, 109, n)
    velocity = rng.integers(40, 128, n)
    notes = np.stack([onset, np.minimum(onset + length, duration), pitch.astype(np.float64), velocity.astype(np.float64)], axis=1)
    return notes[np.argsort(notes[:, 0], kind="stable")]


def synthetic_batch(rng: np.random.Generator, B: int, config, voice: Optional[Voice] = None, device=None):
    """``B`` labelled clips of ``config.dataset.segment_duration`` seconds at ``config.model.sample_rate``: ``synthetic_notes`` per
    clip, in clip order, from ``rng``; all clips rendered by ONE launch, each peak-normalised.  ``ModelInputs`` with the waveform on
    ``device`` (``None``: the GPU), ``notes_batch`` as host float64 arrays and zero ``cond_index``: batches for
    ``Music2MIDI.fit_batches`` with no dataset on the machine."""
    import torch
    from .config import load_config
    from .input import ModelInputs
    config = load_config(config)
    fs, duration = config.model.sample_rate, float(config.dataset.segment_duration)
    notes = tuple(synthetic_notes(rng, duration) for _ in range(int(B)))
    wave = render(list(notes), fs, int(fs * duration), voice, normalize=True, device=device)
    cond = torch.zeros((int(B), len(config.conditioning.keys())), dtype=torch.long, device=wave.device)
    return ModelInputs(input_waveform=wave, notes_batch=notes, cond_index=cond)
