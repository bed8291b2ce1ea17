"""Tokenising of note labels on the device: ``MidiTokenizer.__call__`` for a whole batch as one HIP kernel.

``Music2MIDI._labels`` and ``T5Transformer.forward`` turn the notes of every batch into token ids; on the host that is a Python loop
with ``np.unique`` and two masks per time step and clip.  ``MidiTokenizer`` stays the definition; here the same ids are written by
one launch of csrc/tokenize.hip (one workgroup per clip) on the current stream, exactly: ``torch.equal`` with the host's tensor.

    notes_eligible(tokenizer, notes_batch)                                                        -> bool
    tokenize(tokenizer, notes_batch, cutoff_time, device, width, labels, bucket)                   -> DeviceTokens  (.ids .lengths)
    training_labels(tokenizer, notes_batch, device, pad_token_id, bucket, stream)                  -> labels on the device, or None
    quantize(tokenizer, seconds) / row_bound(n_notes, n_time)                                      host arithmetic of the library

There is no fallback in this module: a missing library or a refused call raises ``native.NativeError``, notes the device path
cannot take raise ``ValueError``.  Callers that want the host path instead ask ``notes_eligible`` first, or go through
``training_labels``, which returns None for such a batch.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import native
from .tokenizer import PAD

MAX_NOTES = 1024                         # M2M_TOKENIZE_MAX_NOTES: per clip
MAX_TIME = 4096                          # M2M_TOKENIZE_MAX_TIME
MAX_ROWS = 65535
MAX_PITCH = 32768                        # |pitch|: far inside what float32 -> int64 converts exactly as numpy does
IGNORE = -100                            # CrossEntropyLoss's ignore_index: what the labels carry for PAD


def quantize(tokenizer, seconds: float) -> int:
    """``tokenizer._quantize(seconds)`` as the kernel computes it (host arithmetic of the library, no GPU); -1 outside its domain."""
    return int(native.load().m2m_tokenize_quantize(float(seconds), float(tokenizer.time_step), int(tokenizer.config.vocab_size.time)))


def row_bound(n_notes: int, n_time: int) -> int:
    """The longest row ``n_notes`` notes can give over ``n_time`` time ids: 1 + 2k + min(2k, T) + 2 min(k, T)."""
    return int(native.load().m2m_tokenize_row_bound(int(n_notes), int(n_time)))


class _Ineligible(ValueError):
    """Notes or a vocabulary the device path does not take."""


def _vocabulary(tokenizer) -> tuple:
    """(time_step, pitch_token_offset, time_token_offset, n_time) within the library's limits, else ``_Ineligible``."""
    try:
        step, po = float(tokenizer.time_step), int(tokenizer.pitch_token_offset)
        to, n_time = int(tokenizer.time_token_offset), int(tokenizer.config.vocab_size.time)
    except (AttributeError, KeyError, TypeError, ValueError):
        raise _Ineligible("the tokenizer does not name its vocabulary") from None
    if not (0.0 < step <= 3600.0):
        raise _Ineligible(f"a time step of {step} s is outside (0, 3600]")
    if not 1 <= n_time <= MAX_TIME:
        raise _Ineligible(f"{n_time} time ids are outside 1..{MAX_TIME}")
    if po < 5 or not po <= to <= 1 << 30:
        raise _Ineligible(f"pitch_token_offset {po} / time_token_offset {to} out of range")
    return step, po, to, n_time


def _flat_notes(notes_batch: Sequence) -> tuple:
    """(every clip's notes as one [n, 4] float64 array, their count per clip); ``_Ineligible`` when the device path cannot take them.
    The rule: every array [n, 4] or empty, n <= 1024, every value finite, onsets >= 0, |pitch| <= 32768.  All arrays are checked in
    one pass (a batch is a hundred small arrays)."""
    arrays = []
    for i, notes in enumerate(notes_batch):
        try:
            a = np.asarray(notes, dtype=np.float64)
        except (TypeError, ValueError):
            raise _Ineligible(f"clip {i}: not a numeric array") from None
        if a.size == 0:
            a = np.zeros((0, 4))
        elif a.ndim != 2 or a.shape[1] != 4:
            raise _Ineligible(f"clip {i}: shape {a.shape} is not [n, 4]")
        if len(a) > MAX_NOTES:
            raise _Ineligible(f"clip {i}: {len(a)} notes, more than {MAX_NOTES}")
        arrays.append(a)
    if len(arrays) > MAX_ROWS:
        raise _Ineligible(f"{len(arrays)} clips, more than {MAX_ROWS}")
    flat = np.concatenate(arrays) if arrays else np.zeros((0, 4))
    per_clip = np.asarray([len(a) for a in arrays], dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for why, wrong in (("a value that is not finite", ~np.isfinite(flat).all(axis=1)), ("a negative onset", flat[:, 0] < 0),
                           (f"a pitch beyond +-{MAX_PITCH}", np.abs(flat[:, 2]) > MAX_PITCH)):
            if wrong.any():
                owner = np.repeat(np.arange(len(arrays)), per_clip)
                raise _Ineligible(f"clip {int(owner[np.argmax(wrong)])}: {why}")
    return flat, per_clip


def notes_eligible(tokenizer, notes_batch) -> bool:
    """True when ``tokenize`` can take every note array of the batch with this tokenizer's vocabulary."""
    try:
        _vocabulary(tokenizer)
        _flat_notes(list(notes_batch))
    except (_Ineligible, TypeError):
        return False
    return True


def _pack(flat: np.ndarray, per_clip: np.ndarray) -> np.ndarray:
    """One float64 buffer for one upload: [3, n] onsets / offsets / pitches, then the [B + 1] int32 offsets in the words that follow."""
    n, B = len(flat), len(per_clip)
    buf = np.zeros(3 * n + (B + 2) // 2, dtype=np.float64)
    buf[:3 * n].reshape(3, n)[:] = flat[:, :3].T
    offsets = buf[3 * n:].view(np.int32)
    offsets[1:B + 1] = np.cumsum(per_clip)
    return buf


class DeviceTokens:
    """``ids`` [B, W] int64 on the device: row r holds its ``lengths[r]`` ids, then the fill; ``lengths`` [B] int32 on the device,
    the true length of every row (larger than W for a row that was cut at ``width=``), -1 for a row the kernel could not place.
    ``ready``: an event behind the kernel, for a consumer on another stream (``stream.wait_event(tokens.ready)``)."""

    def __init__(self, ids: torch.Tensor, lengths: torch.Tensor, width: int, ready: Optional[torch.cuda.Event] = None):
        self.ids, self.lengths, self.width = ids, lengths, int(width)
        self.ready = ready                   # recorded behind the kernel on the stream it ran on (None: nothing was launched)

    def check(self) -> "DeviceTokens":
        """Raise ``ValueError`` for a row that did not fit ``width`` or could not be placed (one small copy to the host)."""
        _raise_for_rows(self.lengths.cpu().numpy(), self.width)
        return self


def _raise_for_rows(lengths: np.ndarray, width: int) -> None:
    bad = np.flatnonzero(lengths < 0)
    if len(bad):
        raise ValueError(f"tokenize: clip {int(bad[0])} holds a value that cannot be placed (not finite, a negative onset): nothing was written for it")
    long = np.flatnonzero(lengths > width)
    if len(long):
        raise ValueError(f"tokenize: clip {int(long[0])} gives {int(lengths[long[0]])} ids, more than width={width}: the row was cut")


def _enqueue(packed: torch.Tensor, n: int, vocabulary: tuple, cutoff_time, fill: int, labels: bool, pad_token_id: int, ids: torch.Tensor,
             lengths: torch.Tensor) -> None:
    """The kernel on the current stream, for notes that are on the device already (``_pack``'s buffer): ids [B, cols], lengths [B]."""
    step, po, to, n_time = vocabulary
    native.check(native.load().m2m_tokenize_notes(
        packed.data_ptr(), packed.data_ptr() + 24 * n, n, int(ids.shape[0]), step, po, to, n_time, 0 if cutoff_time is None else 1,
        0.0 if cutoff_time is None else float(cutoff_time), int(fill), 1 if labels else 0, int(pad_token_id), ids.data_ptr(),
        int(ids.shape[1]), int(ids.stride(0)), lengths.data_ptr(), native.stream_handle(ids.device)), "m2m_tokenize_notes")


def tokenize(tokenizer, notes_batch, cutoff_time=None, device=None, width: Optional[int] = None, labels: bool = False, bucket: int = 1,
             pad_token_id: int = PAD) -> DeviceTokens:
    """``tokenizer(notes_batch, cutoff_time)`` on the device: one packed upload and one launch on the current stream.

    ``width=None``: the rows are written into a buffer as wide as the longest row the clips' note counts allow, the B lengths are
    copied to the host (one small copy, as at the end of ``scoring.chroma_counts``) and ``.ids`` is the view ``[:, :W]``, W the longest
    row rounded up to ``bucket`` - with ``bucket=1`` the tensor the host tokenizer returns.  ``width=int``: no copy and no wait; rows
    that did not fit are cut inside their row and raise on ``.check()``.  ``labels=True`` fills with -100 and writes -100 for every
    id equal to ``pad_token_id``: the tensor ``Music2MIDI._labels`` builds (``bucket=LABEL_BUCKET``)."""
    try:
        step, po, to, n_time = _vocabulary(tokenizer)
        flat, per_clip = _flat_notes(list(notes_batch))
    except _Ineligible as e:
        raise _Ineligible(f"tokenize: the notes are not eligible for the device path: {e}") from None
    if bucket < 1 or (width is not None and width < 1):
        raise ValueError(f"tokenize: bucket={bucket} / width={width} must be at least 1")
    if not torch.cuda.is_available():
        raise native.NativeError("tokenize: no HIP device visible; the host definition is MidiTokenizer.__call__")
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"tokenize: {device} is not a GPU")
    B = len(per_clip)
    if B == 0:
        return DeviceTokens(torch.zeros((0, 0), dtype=torch.int64, device=device), torch.zeros(0, dtype=torch.int32, device=device), 0)
    n = len(flat)
    fill = IGNORE if labels else PAD
    cols = int(width) if width is not None else -(-row_bound(int(per_clip.max()), n_time) // bucket) * bucket
    with torch.cuda.device(device):
        packed = torch.from_numpy(_pack(flat, per_clip)).to(device)
        ids = torch.empty((B, cols), dtype=torch.int64, device=device)
        lengths = torch.empty(B, dtype=torch.int32, device=device)
        _enqueue(packed, n, (step, po, to, n_time), cutoff_time, fill, labels, pad_token_id, ids, lengths)
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(device))
        if width is not None:
            return DeviceTokens(ids, lengths, cols, ready)
        host = lengths.cpu().numpy()
    _raise_for_rows(host, cols)
    W = -(-int(host.max()) // bucket) * bucket
    return DeviceTokens(ids[:, :W], lengths, W, ready)


def training_labels(tokenizer, notes_batch, device, pad_token_id: int, bucket: int, stream):
    """The labels of a teacher-forced pass on ``device`` - ``tokenizer(notes_batch)`` with PAD -> -100, the width rounded up to
    ``bucket`` with -100 - or None when the device path does not take the batch (the caller then builds them on the host).
    ``stream``: the side stream to tokenise on, so that the read-back of the lengths waits for that stream only and not for what
    the current stream still has in flight; the current stream then waits for the kernel's event before it reads the labels."""
    device = torch.device(device)
    if device.type != "cuda" or int(pad_token_id) != PAD:
        return None
    consumer = torch.cuda.current_stream(device)
    try:
        with torch.cuda.stream(stream):
            tokens = tokenize(tokenizer, notes_batch, device=device, labels=True, bucket=bucket, pad_token_id=pad_token_id)
    except _Ineligible:                                       # (the one pass over the notes is tokenize's own)
        return None
    if tokens.ready is not None:
        consumer.wait_event(tokens.ready)
        tokens.ids.record_stream(consumer)
    return tokens.ids
