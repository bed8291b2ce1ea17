"""Scoring of decoded tokens on the device: detokenise, melody, the counts of the chroma accuracy.

Everything ``Music2MIDI.evaluate_batch`` does after ``generate`` - ``MidiTokenizer.decode``, ``numpy_to_midi``,
``evaluation.evaluate_batch`` - is integer work on ids that are already in HBM.  Those host functions stay the definition; here the
same pipeline runs as two HIP kernels (csrc/score.hip) on the current stream and returns what the host returns, exactly: the same
notes, the same counts, the same float.

    detokenize(tokenizer, token_ids [R, L] cuda int64, mode, duration_per_batch)   -> DeviceNotes   (.to_numpy() == tokenizer.decode(...))
    detokenize_scored(tokenizer, token_ids, token_logprobs [R, L] cuda float32, mode, duration_per_batch, min_confidence)
                                                                                   -> DeviceNotes   (+ .note_lp, .confidence_numpy())
    chroma_counts(tokenizer, token_ids, notes_batch, mode, duration_per_batch)     -> ChromaCounts  (.correct .voiced .frames .score)
    note_counts(tokenizer, token_ids, notes_batch, ..., token_logprobs, thresholds) -> NoteCounts    (.tp .n_est .n_ref [T, K], .f1 ...)
    frame_counts(tokenizer, token_ids, notes_batch, ..., token_logprobs, thresholds) -> FrameCounts  (.tp .fn .fp .melody_* [T, K], .f1 ...)
    error_notes(tokenizer, token_ids, notes_batch, ..., melody_only, min_confidence) -> ErrorNotes  (.to_numpy(): TP / FN / FP notes)
    labels_eligible(notes_batch)                                                   -> bool

``frame_counts`` and ``error_notes`` are the frame-level piano-roll comparison of ``music2midi_amd.frame_metrics``
(csrc/frame_roll.hip): the true-positive, false-negative and false-positive cells of the two rolls, as counts per threshold and as
notes.  ``note_counts`` is the note-level matching of ``music2midi_amd.note_metrics`` (csrc/note_match.hip): one launch for every confidence
threshold of a sweep, the integers equal to the definition's.

``batched``: row i is clip i, scored against ``notes_batch[i]``; ``sequential``: the rows are the segments of one recording, scored
against ONE label array.  ``cutoff_time`` is not supported.  There is no fallback in this module: a missing library or a refused
call raises ``native.NativeError``, labels the device path cannot take raise ``ValueError`` (callers that want the host path
instead ask ``labels_eligible`` first, as ``Music2MIDI.score_batch`` does).
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from . import native

FS = 100                                 # frames per second of the metric (evaluation.extract_midi_melody's default, the only one)
MAX_TOKENS = 2048
MAX_FRAMES = 1 << 22                     # M2M_SCORE_MAX_FRAMES: 11.6 hours per timeline
MAX_VOCAB = 4096


def frame_count(end_seconds: float) -> int:
    """``len(np.arange(0, end_seconds, 1 / 100))`` as the kernels compute it (host arithmetic of the library, no GPU)."""
    return int(native.load().m2m_score_frame_count(float(end_seconds)))


def _steps_per_row(tokenizer, mode: str, duration_per_batch) -> int:
    if mode == "batched":
        return 0
    if mode == "sequential":
        if duration_per_batch is None:
            raise ValueError('duration_per_batch is required for mode="sequential"')
        return int(round(duration_per_batch / tokenizer.time_step))
    raise ValueError(f"Invalid argument mode={mode}")


def _vocab_size(tokenizer, vocab_size: Optional[int]) -> int:
    """The ids the model can emit: the argument, else the T5 vocabulary the tokenizer's config names, else the device limit."""
    if vocab_size is None:
        vocab_size = getattr(tokenizer, "model_vocab_size", None)
    return MAX_VOCAB if vocab_size is None else int(vocab_size)


class DeviceNotes:
    """The notes of every row, on the device: ``notes`` [R, L, 3] int32 (onset index, offset index, pitch), the first
    ``counts[r]`` of row r in emission order; ``counts`` [R] int32, -1 for a row that held an id outside the vocabulary.
    From ``detokenize_scored`` also ``note_lp`` [R, L, 2] float32: the onset and offset parts of the notes' log-probability
    (``music2midi_amd.confidence``), side by side with ``notes``; ``None`` otherwise."""

    def __init__(self, notes: torch.Tensor, counts: torch.Tensor, mode: str, time_step: float, default_velocity, steps_per_row: int,
                 note_lp: Optional[torch.Tensor] = None):
        self.notes, self.counts, self.mode = notes, counts, mode
        self.time_step, self.default_velocity, self.steps_per_row = time_step, default_velocity, steps_per_row
        self.note_lp = note_lp

    def to_numpy(self) -> Union[List[np.ndarray], np.ndarray]:
        """What ``tokenizer.decode(token_ids, mode, duration_per_batch)`` returns: a list of [n, 4] float64 arrays, or their
        concatenation in ``sequential`` mode."""
        counts = self.counts.cpu().numpy()
        _raise_for_bad_rows(counts)
        notes = self.notes.cpu().numpy()
        parts = []
        for r, c in enumerate(counts):
            out = np.zeros((int(c), 4), dtype=np.float64)
            out[:, :3] = notes[r, :c]
            out[:, 3] = self.default_velocity
            out[:, :2] = out[:, :2] * self.time_step
            parts.append(out)
        return parts if self.mode == "batched" else np.concatenate(parts)

    def note_lp_numpy(self) -> Union[List[np.ndarray], np.ndarray]:
        """The (onset part, offset part) float32 pairs of the notes ``to_numpy()`` returns, [n, 2] per row or concatenated."""
        if self.note_lp is None:
            raise ValueError("these notes carry no log-probabilities: they do not come from detokenize_scored")
        counts = self.counts.cpu().numpy()
        _raise_for_bad_rows(counts)
        lp = self.note_lp.cpu().numpy()
        parts = [lp[r, :c].copy() for r, c in enumerate(counts)]
        return parts if self.mode == "batched" else np.concatenate(parts)

    def confidence_numpy(self) -> Union[List[np.ndarray], np.ndarray]:
        """``exp`` in float64 of the notes' float32 total (onset part + offset part), one value per note of ``to_numpy()``, in the
        list / concatenated shape of the mode: what ``confidence.decode_with_confidence`` returns second."""
        from .confidence import confidence_of
        lp = self.note_lp_numpy()
        return [confidence_of(p) for p in lp] if self.mode == "batched" else confidence_of(lp)


def _raise_for_bad_rows(counts: np.ndarray) -> None:
    bad = np.flatnonzero(counts < 0)
    if len(bad):
        raise ValueError(f"token row {int(bad[0])} holds an id outside [0, vocab_size): nothing was decoded for it")


def detokenize(tokenizer, token_ids: torch.Tensor, mode: str = "batched", duration_per_batch: Optional[float] = None,
               vocab_size: Optional[int] = None) -> DeviceNotes:
    """``tokenizer.decode`` on the device, one workgroup per row; nothing is copied to the host until ``to_numpy()``."""
    return _detokenize(tokenizer, token_ids, mode, duration_per_batch, vocab_size, None, 0.0)


def detokenize_scored(tokenizer, token_ids: torch.Tensor, token_logprobs: torch.Tensor, mode: str = "batched",
                      duration_per_batch: Optional[float] = None, min_confidence: float = 0.0,
                      vocab_size: Optional[int] = None) -> DeviceNotes:
    """``confidence.decode_with_confidence`` on the device: ``detokenize`` with the log-probability of every id
    (``token_logprobs`` [R, L] CUDA float32, column-aligned, unit inner stride).  The notes whose float32 total is below
    ``float32(log(min_confidence))`` are dropped on the device (a NaN total is kept); ``to_numpy()`` and ``confidence_numpy()``
    give the kept notes and their confidences, ``note_lp`` the two float32 parts."""
    from .confidence import min_logprob
    floor = float(min_logprob(min_confidence))
    if not (isinstance(token_logprobs, torch.Tensor) and token_logprobs.is_cuda and token_logprobs.dim() == 2
            and token_logprobs.dtype == torch.float32):
        raise ValueError("detokenize_scored: token_logprobs must be a CUDA float32 tensor [rows, length]")
    return _detokenize(tokenizer, token_ids, mode, duration_per_batch, vocab_size, token_logprobs, floor)


def _detokenize(tokenizer, token_ids, mode, duration_per_batch, vocab_size, token_logprobs, floor: float) -> DeviceNotes:
    scored = token_logprobs is not None
    steps = _steps_per_row(tokenizer, mode, duration_per_batch)
    velocity = tokenizer.config.default_velocity
    if not velocity > 0:
        raise ValueError(f"default_velocity = {velocity}: the decoder opens a note only with a positive velocity")
    if not (isinstance(token_ids, torch.Tensor) and token_ids.is_cuda and token_ids.dim() == 2 and token_ids.dtype == torch.int64):
        raise ValueError("detokenize: token_ids must be a CUDA int64 tensor [rows, length]")
    R, L = token_ids.shape
    device = token_ids.device
    if scored:
        if tuple(token_logprobs.shape) != (R, L) or token_logprobs.device != device:
            raise ValueError(f"detokenize_scored: token_logprobs {tuple(token_logprobs.shape)} on {token_logprobs.device} for token_ids "
                             f"{(R, L)} on {device}")
        if L > 1 and token_logprobs.stride(1) != 1:
            raise ValueError("detokenize_scored: token_logprobs must have unit inner stride")
    if R == 0:
        if mode == "sequential":
            raise ValueError("need at least one row to concatenate")
        return DeviceNotes(torch.zeros((0, 1, 3), dtype=torch.int32, device=device), torch.zeros(0, dtype=torch.int32, device=device),
                           mode, tokenizer.time_step, velocity, steps,
                           torch.zeros((0, 1, 2), dtype=torch.float32, device=device) if scored else None)
    if L == 0:                                               # PAD is skipped: one column of it decodes as the empty row does
        token_ids, L = token_ids.new_zeros((R, 1)), 1
        token_logprobs = token_logprobs.new_zeros((R, 1)) if scored else None
    if token_ids.stride(1) != 1:
        token_ids = token_ids.contiguous()
    if scored and token_logprobs.stride(1) != 1:             # (one column: any stride reads the same element)
        token_logprobs = token_logprobs.contiguous()
    with torch.cuda.device(device):
        # (sizes the library will refuse are not allocated for: it answers on the arguments alone)
        fits = R <= 65535 and L <= MAX_TOKENS
        notes = torch.empty((R, L, 3) if fits else (1, 1, 3), dtype=torch.int32, device=device)
        counts = torch.empty(R if fits else 1, dtype=torch.int32, device=device)
        if not scored:
            native.check(native.load().m2m_score_detokenize(
                token_ids.data_ptr(), R, L, token_ids.stride(0), steps, int(tokenizer.pitch_token_offset), int(tokenizer.time_token_offset),
                _vocab_size(tokenizer, vocab_size), notes.data_ptr(), counts.data_ptr(), native.stream_handle(device)), "m2m_score_detokenize")
            return DeviceNotes(notes, counts, mode, tokenizer.time_step, velocity, steps)
        note_lp = torch.empty((R, L, 2) if fits else (1, 1, 2), dtype=torch.float32, device=device)
        native.check(native.load().m2m_score_detokenize_scored(
            token_ids.data_ptr(), R, L, token_ids.stride(0), steps, int(tokenizer.pitch_token_offset), int(tokenizer.time_token_offset),
            _vocab_size(tokenizer, vocab_size), token_logprobs.data_ptr(), token_logprobs.stride(0), floor, notes.data_ptr(),
            counts.data_ptr(), note_lp.data_ptr(), native.stream_handle(device)), "m2m_score_detokenize_scored")
    return DeviceNotes(notes, counts, mode, tokenizer.time_step, velocity, steps, note_lp)


# ----------------------------------------------------------------------------------------------------------------- labels
class _Ineligible(ValueError):
    pass


def _kept_labels(label_arrays: Sequence) -> tuple:
    """(the notes ``numpy_to_midi`` keeps (``end > start``) of every array as one [n, 4] float64 array, their count per array);
    ``_Ineligible`` when the device path cannot score against them.  The rule, for the kept notes: every value finite,
    ``start >= 0``, ``0 <= int(pitch) <= 127``, ``int(velocity) >= 1`` - a velocity in (0, 1) is truncated to 0 by ``numpy_to_midi``
    and sounds in no frame on the host, so it is left to the host - and an end within the frame cap.  All arrays are checked in
    one pass (a batch is a hundred small arrays)."""
    arrays = []
    for i, notes in enumerate(label_arrays):
        try:
            a = np.asarray(notes, dtype=np.float64)
        except (TypeError, ValueError):
            raise _Ineligible(f"timeline {i}: not a numeric array") from None
        if a.ndim != 2 or a.shape[1] != 4:
            raise _Ineligible(f"timeline {i}: shape {a.shape} is not [n, 4]")
        arrays.append(a)
    flat = np.concatenate(arrays) if arrays else np.zeros((0, 4))
    owner = np.repeat(np.arange(len(arrays)), [len(a) for a in arrays])
    with np.errstate(invalid="ignore"):
        keep = flat[:, 1] > flat[:, 0]
    flat, owner = flat[keep], owner[keep]
    pitch = np.trunc(flat[:, 2])
    for why, wrong in (("a value that is not finite", ~np.isfinite(flat).all(axis=1)), ("a negative start", flat[:, 0] < 0),
                       ("a pitch outside 0..127", (pitch < 0) | (pitch > 127)), ("a velocity below 1", flat[:, 3] < 1)):
        if wrong.any():
            raise _Ineligible(f"timeline {int(owner[np.argmax(wrong)])}: {why}")
    if len(flat) and frame_count(float(flat[:, 1].max())) > MAX_FRAMES:
        raise _Ineligible(f"timeline {int(owner[np.argmax(flat[:, 1])])}: an end beyond {MAX_FRAMES} frames")
    return flat, np.bincount(owner, minlength=len(arrays))


def labels_eligible(notes_batch: Sequence) -> bool:
    """True when ``chroma_counts`` can take every label array of the batch."""
    try:
        _kept_labels(notes_batch)
    except _Ineligible:
        return False
    return True


def _pack_labels(label_arrays: Sequence) -> tuple:
    """([3, N] float64 starts / ends / int(pitch) of the notes with end > start, [T + 1] int32 offsets, frames bound)."""
    try:
        flat, per_array = _kept_labels(label_arrays)
    except _Ineligible as e:
        raise ValueError(f"chroma_counts: the labels are not eligible for the device path: {e}") from None
    packed = np.ascontiguousarray(flat[:, :3].T)
    packed[2] = np.trunc(packed[2])
    offsets = np.concatenate([[0], np.cumsum(per_array)]).astype(np.int32)
    bound = frame_count(float(packed[1].max())) if packed.shape[1] else 0
    return packed, offsets, bound


class ChromaCounts:
    """int64 ``correct``, ``voiced``, ``frames`` per timeline; ``score`` = sum(correct) / sum(voiced) in float64 (0.0 without a
    voiced frame), the value of ``evaluation.evaluate_batch``; ``scores`` the same ratio per timeline."""

    def __init__(self, correct: np.ndarray, voiced: np.ndarray, frames: np.ndarray):
        self.correct, self.voiced, self.frames = correct, voiced, frames

    @property
    def score(self) -> float:
        voiced = self.voiced.sum()
        return float(self.correct.sum() / voiced) if voiced else 0.0

    @property
    def scores(self) -> np.ndarray:
        out = np.zeros(len(self.voiced), dtype=np.float64)
        np.divide(self.correct, self.voiced, out=out, where=self.voiced > 0)
        return out


def _enqueue_counts(dn: DeviceNotes, labels_dev: torch.Tensor, offsets_dev: torch.Tensor, frame_cap: int) -> torch.Tensor:
    """The counts kernel on the current stream, for labels that are on the device already: [T, 3] int32 (correct, voiced, frames)."""
    R, L = int(dn.notes.shape[0]), int(dn.notes.shape[1])
    T, n_labels = int(offsets_dev.shape[0]) - 1, int(labels_dev.shape[1])
    device = dn.notes.device
    out = torch.empty((T, 3), dtype=torch.int32, device=device)
    native.check(native.load().m2m_score_chroma_counts(
        dn.notes.data_ptr(), dn.counts.data_ptr(), R, L, 1 if dn.mode == "sequential" else 0, float(dn.time_step),
        labels_dev.data_ptr() if n_labels else None, offsets_dev.data_ptr(), n_labels, T, int(frame_cap), out.data_ptr(),
        native.stream_handle(device)), "m2m_score_chroma_counts")
    return out


def chroma_counts(tokenizer, token_ids: torch.Tensor, notes_batch, mode: str = "batched", duration_per_batch: Optional[float] = None,
                  vocab_size: Optional[int] = None, token_logprobs: Optional[torch.Tensor] = None,
                  min_confidence: float = 0.0) -> ChromaCounts:
    """The counts of ``evaluation.evaluate_batch(labels, decoded)`` for ids on the device.  ``notes_batch``: one label array per
    row (``batched``), or ONE array for the whole recording (``sequential``).  One small copy to the host at the end.
    With ``token_logprobs`` the ids are detokenised by ``detokenize_scored`` and only the notes of at least ``min_confidence`` are
    counted; a threshold without log-probabilities raises ``ValueError``."""
    labels = [notes_batch] if mode == "sequential" else list(notes_batch)
    if token_logprobs is None:
        from .confidence import min_logprob
        if min_logprob(min_confidence) != -np.inf:
            raise ValueError(f"chroma_counts: min_confidence={min_confidence} needs token_logprobs")
        dn = detokenize(tokenizer, token_ids, mode, duration_per_batch, vocab_size)
    else:
        dn = detokenize_scored(tokenizer, token_ids, token_logprobs, mode, duration_per_batch, min_confidence, vocab_size)
    R = int(dn.counts.shape[0])
    T = 1 if mode == "sequential" else R
    if len(labels) != T:
        raise ValueError(f"chroma_counts: {len(labels)} label arrays for {T} timelines")
    packed, offsets, label_frames = _pack_labels(labels)
    if R == 0:
        empty = np.zeros(0, dtype=np.int64)
        return ChromaCounts(empty, empty.copy(), empty.copy())
    # the largest time index a row can hold bounds the output's frames: the grid is sized for it and for the labels
    vocab = _vocab_size(tokenizer, vocab_size)
    top_index = (R - 1) * dn.steps_per_row + max(0, vocab - 1 - int(tokenizer.time_token_offset))
    frame_cap = max(1, label_frames, frame_count(top_index * tokenizer.time_step))
    if frame_cap > MAX_FRAMES:
        raise ValueError(f"chroma_counts: a timeline of up to {frame_cap} frames exceeds the device limit of {MAX_FRAMES}")
    device = dn.notes.device
    with torch.cuda.device(device):
        lab = torch.from_numpy(packed).to(device)
        off = torch.from_numpy(offsets).to(device)
        out = _enqueue_counts(dn, lab, off, frame_cap)
        host = torch.cat([out.reshape(-1), dn.counts]).cpu().numpy()
    _raise_for_bad_rows(host[3 * T:])
    res = host[:3 * T].reshape(T, 3).astype(np.int64)
    if (res[:, 2] < 0).any():
        raise native.NativeError(f"m2m_score_chroma_counts: a timeline is longer than its bound of {frame_cap} frames")
    return ChromaCounts(res[:, 0].copy(), res[:, 1].copy(), res[:, 2].copy())


# ----------------------------------------------------------------------------------------------------------------- note metrics
MAX_THRESHOLDS = 64                      # M2M_SCORE_MAX_THRESHOLDS


class NoteCounts:
    """int64 ``tp``, ``n_est``, ``n_ref`` of shape [T, K]: per timeline and per threshold, the size of the maximum matching, the
    decoded notes kept under the threshold and the label notes (``note_metrics.match_counts``).  ``precision``, ``recall`` and
    ``f1`` [K] float64 are micro-averaged: the integers are summed over the timelines first; ``per_timeline_f1`` is [T, K]."""

    def __init__(self, tp: np.ndarray, n_est: np.ndarray, n_ref: np.ndarray):
        self.tp, self.n_est, self.n_ref = tp, n_est, n_ref

    def _micro(self) -> np.ndarray:
        from .note_metrics import precision_recall_f1
        sums = zip(self.tp.sum(axis=0).tolist(), self.n_ref.sum(axis=0).tolist(), self.n_est.sum(axis=0).tolist())
        return np.asarray([precision_recall_f1(*s) for s in sums], dtype=np.float64).reshape(-1, 3)

    @property
    def precision(self) -> np.ndarray:
        return self._micro()[:, 0].copy()

    @property
    def recall(self) -> np.ndarray:
        return self._micro()[:, 1].copy()

    @property
    def f1(self) -> np.ndarray:
        return self._micro()[:, 2].copy()

    @property
    def per_timeline_f1(self) -> np.ndarray:
        from .note_metrics import precision_recall_f1
        out = np.zeros(self.tp.shape, dtype=np.float64)
        for i in np.ndindex(*self.tp.shape):
            out[i] = precision_recall_f1(self.tp[i], self.n_ref[i], self.n_est[i])[2]
        return out


def threshold_logprobs(thresholds, scored: bool, who: str = "note_counts") -> np.ndarray:
    """[K] float32 ``confidence.min_logprob`` of every threshold (``None``: ``[0.0]``); ``ValueError`` for an empty or too long
    sequence, a threshold that is no probability, or a positive threshold without log-probabilities."""
    from .confidence import min_logprob
    values = [0.0] if thresholds is None else [float(c) for c in thresholds]
    if not 1 <= len(values) <= MAX_THRESHOLDS:
        raise ValueError(f"{who}: {len(values)} thresholds out of range (1..{MAX_THRESHOLDS})")
    floors = np.asarray([min_logprob(c) for c in values], dtype=np.float32)
    if not scored and (floors != -np.inf).any():
        raise ValueError(f"{who}: thresholds={values} need token_logprobs")
    return floors


def _enqueue_note_counts(dn: DeviceNotes, labels_dev: torch.Tensor, offsets_dev: torch.Tensor, min_logprobs_dev: Optional[torch.Tensor],
                         onset_tolerance: float, offset_ratio: float, offset_min_tolerance: float) -> torch.Tensor:
    """The matching kernel on the current stream, for labels and thresholds that are on the device already: [T, K, 3] int32
    (tp, n_est, n_ref); K = 1 without thresholds.  ``offset_ratio`` < 0: onsets only.  The workspace is torch's."""
    R, L = int(dn.notes.shape[0]), int(dn.notes.shape[1])
    T, n_labels = int(offsets_dev.shape[0]) - 1, int(labels_dev.shape[1])
    K = 1 if min_logprobs_dev is None else int(min_logprobs_dev.shape[0])
    device = dn.notes.device
    lib = native.load()
    need = int(lib.m2m_score_note_workspace_bytes(R, L, n_labels, K))
    # (sizes the library will refuse are not allocated for: it answers on the arguments alone)
    workspace = torch.empty(max(need, 8) // 8, dtype=torch.int64, device=device)
    out = torch.empty((T, K, 3), dtype=torch.int32, device=device)
    scored = dn.note_lp is not None and min_logprobs_dev is not None
    native.check(lib.m2m_score_note_counts(
        dn.notes.data_ptr(), dn.counts.data_ptr(), dn.note_lp.data_ptr() if scored else None, R, L, 1 if dn.mode == "sequential" else 0,
        float(dn.time_step), labels_dev.data_ptr() if n_labels else None, offsets_dev.data_ptr(), n_labels, T, onset_tolerance,
        offset_ratio, offset_min_tolerance, min_logprobs_dev.data_ptr() if scored else None, K, workspace.data_ptr(), need,
        out.data_ptr(), native.stream_handle(device)), "m2m_score_note_counts")
    return out


def note_counts(tokenizer, token_ids: torch.Tensor, notes_batch, mode: str = "batched", duration_per_batch: Optional[float] = None,
                vocab_size: Optional[int] = None, token_logprobs: Optional[torch.Tensor] = None, thresholds=None,
                onset_tolerance: float = 0.05, offset_ratio: Optional[float] = 0.2, offset_min_tolerance: float = 0.05) -> NoteCounts:
    """``note_metrics.match_counts(labels, decoded notes of at least thresholds[k])`` for ids on the device, for every timeline and
    every threshold: one detokenise, one launch for all thresholds (csrc/note_match.hip), one copy of [T, K, 3] integers to the
    host.  ``notes_batch`` as in ``chroma_counts``.  ``thresholds``: confidences in [0, 1] (``None``: ``[0.0]``); positive ones need
    ``token_logprobs``.  ``offset_ratio=None`` is the onset-only metric.  The matching is exact: no cap, no host route."""
    labels = [notes_batch] if mode == "sequential" else list(notes_batch)
    floors = threshold_logprobs(thresholds, token_logprobs is not None)
    K = len(floors)
    for name, value in (("onset_tolerance", onset_tolerance), ("offset_min_tolerance", offset_min_tolerance)):
        if not 0.0 <= float(value) <= 3600.0:
            raise ValueError(f"note_counts: {name}={value} out of range [0, 3600] seconds")
    ratio = -1.0 if offset_ratio is None else float(offset_ratio)
    if offset_ratio is not None and not 0.0 <= ratio <= 1e6:
        raise ValueError(f"note_counts: offset_ratio={offset_ratio} out of range [0, 1e6] (None: onsets only)")
    if token_logprobs is None:
        dn = detokenize(tokenizer, token_ids, mode, duration_per_batch, vocab_size)
    else:
        dn = detokenize_scored(tokenizer, token_ids, token_logprobs, mode, duration_per_batch, 0.0, vocab_size)
    R = int(dn.counts.shape[0])
    T = 1 if mode == "sequential" else R
    if len(labels) != T:
        raise ValueError(f"note_counts: {len(labels)} label arrays for {T} timelines")
    try:
        packed, offsets, _ = _pack_labels(labels)
    except ValueError as e:
        raise ValueError(str(e).replace("chroma_counts", "note_counts", 1)) from None
    if R == 0:
        empty = np.zeros((0, K), dtype=np.int64)
        return NoteCounts(empty, empty.copy(), empty.copy())
    device = dn.notes.device
    Kd = K if dn.note_lp is not None else 1                  # without log-probabilities every threshold keeps every note: one column
    with torch.cuda.device(device):
        lab = torch.from_numpy(packed).to(device)
        off = torch.from_numpy(offsets).to(device)
        thr = torch.from_numpy(floors).to(device) if dn.note_lp is not None else None
        out = _enqueue_note_counts(dn, lab, off, thr, float(onset_tolerance), ratio, float(offset_min_tolerance))
        host = torch.cat([out.reshape(-1), dn.counts]).cpu().numpy()
    _raise_for_bad_rows(host[3 * T * Kd:])
    res = np.repeat(host[:3 * T * Kd].reshape(T, Kd, 3).astype(np.int64), K // Kd, axis=1)
    return NoteCounts(res[:, :, 0].copy(), res[:, :, 1].copy(), res[:, :, 2].copy())


# ----------------------------------------------------------------------------------------------------------------- frame metrics
FRAME_TILE = 1024                        # M2M_SCORE_FRAME_TILE: frames of one timeline per workgroup of csrc/frame_roll.hip


class FrameCounts:
    """int64 ``tp``, ``fn``, ``fp`` and ``melody_tp``, ``melody_fn``, ``melody_fp`` of shape [T, K]: per timeline and per threshold,
    the cells of the piano rolls at 100 frames per second that sound on both sides, in the labels only, in the output only
    (``frame_metrics.frame_counts``), on the full roll and on the 12-row melody roll; ``frames`` [T] is ``n_frames`` with every
    output note kept.  ``precision``, ``recall``, ``f1`` and their ``melody_`` forms [K] float64 are micro-averaged: the integers
    are summed over the timelines first; ``per_timeline_f1`` is [T, K]."""

    def __init__(self, tp, fn, fp, melody_tp, melody_fn, melody_fp, frames):
        self.tp, self.fn, self.fp = tp, fn, fp
        self.melody_tp, self.melody_fn, self.melody_fp = melody_tp, melody_fn, melody_fp
        self.frames = frames

    def _micro(self, prefix: str = "") -> np.ndarray:
        from .note_metrics import precision_recall_f1
        tp, fn, fp = (getattr(self, prefix + n).sum(axis=0).tolist() for n in ("tp", "fn", "fp"))
        return np.asarray([precision_recall_f1(a, a + b, a + c) for a, b, c in zip(tp, fn, fp)], dtype=np.float64).reshape(-1, 3)

    precision = property(lambda self: self._micro()[:, 0].copy())
    recall = property(lambda self: self._micro()[:, 1].copy())
    f1 = property(lambda self: self._micro()[:, 2].copy())
    melody_precision = property(lambda self: self._micro("melody_")[:, 0].copy())
    melody_recall = property(lambda self: self._micro("melody_")[:, 1].copy())
    melody_f1 = property(lambda self: self._micro("melody_")[:, 2].copy())

    @property
    def per_timeline_f1(self) -> np.ndarray:
        from .note_metrics import precision_recall_f1
        out = np.zeros(self.tp.shape, dtype=np.float64)
        for i in np.ndindex(*self.tp.shape):
            out[i] = precision_recall_f1(self.tp[i], self.tp[i] + self.fn[i], self.tp[i] + self.fp[i])[2]
        return out


def _frame_cap(tokenizer, dn: DeviceNotes, vocab_size: Optional[int], label_frames: int, who: str) -> int:
    """The bound on n_frames of any timeline the grid is sized for: the labels' and the largest time index a row can hold."""
    R = int(dn.counts.shape[0])
    top_index = (R - 1) * dn.steps_per_row + max(0, _vocab_size(tokenizer, vocab_size) - 1 - int(tokenizer.time_token_offset))
    frame_cap = max(1, label_frames, frame_count(top_index * tokenizer.time_step))
    if frame_cap > MAX_FRAMES:
        raise ValueError(f"{who}: a timeline of up to {frame_cap} frames exceeds the device limit of {MAX_FRAMES}")
    return frame_cap


def _enqueue_frame_counts(dn: DeviceNotes, labels_dev: torch.Tensor, offsets_dev: torch.Tensor, min_logprobs_dev: Optional[torch.Tensor],
                          frame_cap: int) -> torch.Tensor:
    """The counts kernel of csrc/frame_roll.hip on the current stream, for labels and thresholds that are on the device already:
    [T * K * 6 + T] int32 - (tp, fn, fp, melody tp, fn, fp) per timeline and threshold, then ``frames`` [T]; K = 1 without
    thresholds."""
    R, L = int(dn.notes.shape[0]), int(dn.notes.shape[1])
    T, n_labels = int(offsets_dev.shape[0]) - 1, int(labels_dev.shape[1])
    scored = dn.note_lp is not None and min_logprobs_dev is not None
    K = int(min_logprobs_dev.shape[0]) if scored else 1
    device = dn.notes.device
    out = torch.empty(T * K * 6 + T, dtype=torch.int32, device=device)
    native.check(native.load().m2m_score_frame_counts(
        dn.notes.data_ptr(), dn.counts.data_ptr(), dn.note_lp.data_ptr() if scored else None, R, L, 1 if dn.mode == "sequential" else 0,
        float(dn.time_step), labels_dev.data_ptr() if n_labels else None, offsets_dev.data_ptr(), n_labels, T, int(frame_cap),
        min_logprobs_dev.data_ptr() if scored else None, K, out.data_ptr(), out.data_ptr() + 4 * T * K * 6,
        native.stream_handle(device)), "m2m_score_frame_counts")
    return out


def frame_counts(tokenizer, token_ids: torch.Tensor, notes_batch, mode: str = "batched", duration_per_batch: Optional[float] = None,
                 vocab_size: Optional[int] = None, token_logprobs: Optional[torch.Tensor] = None, thresholds=None) -> FrameCounts:
    """``frame_metrics.frame_counts(labels, decoded notes of at least thresholds[k])`` for ids on the device, for every timeline and
    every threshold: one detokenise, one launch for all thresholds (csrc/frame_roll.hip), one copy of the integers to the host.
    ``notes_batch`` as in ``chroma_counts``, ``thresholds`` as in ``note_counts``."""
    labels = [notes_batch] if mode == "sequential" else list(notes_batch)
    floors = threshold_logprobs(thresholds, token_logprobs is not None, "frame_counts")
    K = len(floors)
    if token_logprobs is None:
        dn = detokenize(tokenizer, token_ids, mode, duration_per_batch, vocab_size)
    else:
        dn = detokenize_scored(tokenizer, token_ids, token_logprobs, mode, duration_per_batch, 0.0, vocab_size)
    R = int(dn.counts.shape[0])
    T = 1 if mode == "sequential" else R
    if len(labels) != T:
        raise ValueError(f"frame_counts: {len(labels)} label arrays for {T} timelines")
    try:
        packed, offsets, label_frames = _pack_labels(labels)
    except ValueError as e:
        raise ValueError(str(e).replace("chroma_counts", "frame_counts", 1)) from None
    if R == 0:
        empty = np.zeros((0, K), dtype=np.int64)
        return FrameCounts(*(empty.copy() for _ in range(6)), np.zeros(0, dtype=np.int64))
    frame_cap = _frame_cap(tokenizer, dn, vocab_size, label_frames, "frame_counts")
    device = dn.notes.device
    Kd = K if dn.note_lp is not None else 1                  # without log-probabilities every threshold keeps every note: one column
    with torch.cuda.device(device):
        lab = torch.from_numpy(packed).to(device)
        off = torch.from_numpy(offsets).to(device)
        thr = torch.from_numpy(floors).to(device) if dn.note_lp is not None else None
        out = _enqueue_frame_counts(dn, lab, off, thr, frame_cap)
        host = torch.cat([out, dn.counts]).cpu().numpy()
    n = 6 * T * Kd
    _raise_for_bad_rows(host[n + T:])
    frames = host[n:n + T].astype(np.int64)
    if (frames < 0).any():
        raise native.NativeError(f"m2m_score_frame_counts: a timeline is longer than its bound of {frame_cap} frames")
    res = np.repeat(host[:n].reshape(T, Kd, 6).astype(np.int64), K // Kd, axis=1)
    return FrameCounts(*(res[:, :, i].copy() for i in range(6)), frames)


class ErrorNotes:
    """The TP / FN / FP rolls of every timeline as notes, on the device: ``notes`` [T, 3, cap, 3] int32 (first frame, end frame,
    row) - the first ``counts[t, kind]`` of kind TP / FN / FP of timeline t, ordered by end frame, then row - and ``counts`` [T, 3]
    int32.  A row is a pitch, or a pitch class with ``melody_only``."""

    def __init__(self, notes: torch.Tensor, counts: torch.Tensor, row_counts: torch.Tensor, melody_only: bool):
        self.notes, self.counts, self.melody_only = notes, counts, melody_only
        self._row_counts = row_counts

    def to_numpy(self) -> list:
        """Per timeline ``(tp, fn, fp)``: [n, 4] float64 arrays (start, end, row, velocity 1) with ``start = first / 100`` and
        ``end = end frame / 100`` in float64 - ``frame_metrics.roll_to_notes`` of ``frame_metrics.error_rolls``."""
        T = int(self.counts.shape[0])
        host = torch.cat([self.counts.reshape(-1), self._row_counts]).cpu().numpy()
        _raise_for_bad_rows(host[3 * T:])
        counts = host[:3 * T].reshape(T, 3)
        if (counts < 0).any():
            raise native.NativeError(f"m2m_score_error_notes: timeline {int(np.argmax((counts < 0).any(axis=1)))} is beyond its bounds")
        notes = self.notes.cpu().numpy()
        out = []
        for t in range(T):
            kinds = []
            for q in range(3):
                frames = notes[t, q, :counts[t, q]]
                a = np.ones((len(frames), 4), dtype=np.float64)
                a[:, 0], a[:, 1], a[:, 2] = frames[:, 0] / FS, frames[:, 1] / FS, frames[:, 2]
                kinds.append(a)
            out.append(tuple(kinds))
        return out


def error_notes(tokenizer, token_ids: torch.Tensor, notes_batch, mode: str = "batched", duration_per_batch: Optional[float] = None,
                melody_only: bool = False, token_logprobs: Optional[torch.Tensor] = None, min_confidence: float = 0.0,
                vocab_size: Optional[int] = None) -> ErrorNotes:
    """``frame_metrics.error_rolls`` + ``roll_to_notes`` for ids on the device: where the decode of at least ``min_confidence``
    (positive: needs ``token_logprobs``) is right, misses and adds, as three note lists per timeline in the definition's order,
    extracted on the device (csrc/frame_roll.hip); the tensors stay there until ``to_numpy()``."""
    from .confidence import min_logprob
    labels = [notes_batch] if mode == "sequential" else list(notes_batch)
    floor = float(min_logprob(min_confidence))
    if token_logprobs is None:
        if floor != -np.inf:
            raise ValueError(f"error_notes: min_confidence={min_confidence} needs token_logprobs")
        dn = detokenize(tokenizer, token_ids, mode, duration_per_batch, vocab_size)
    else:
        dn = detokenize_scored(tokenizer, token_ids, token_logprobs, mode, duration_per_batch, 0.0, vocab_size)
    R, L = int(dn.notes.shape[0]), int(dn.notes.shape[1])
    T = 1 if mode == "sequential" else R
    if len(labels) != T:
        raise ValueError(f"error_notes: {len(labels)} label arrays for {T} timelines")
    try:
        packed, offsets, label_frames = _pack_labels(labels)
    except ValueError as e:
        raise ValueError(str(e).replace("chroma_counts", "error_notes", 1)) from None
    device = dn.notes.device
    if R == 0:
        return ErrorNotes(torch.zeros((0, 3, 1, 3), dtype=torch.int32, device=device), torch.zeros((0, 3), dtype=torch.int32, device=device),
                          dn.counts, bool(melody_only))
    frame_cap = _frame_cap(tokenizer, dn, vocab_size, label_frames, "error_notes")
    max_labels, n_labels = int(np.diff(offsets).max()), int(packed.shape[1])
    lib = native.load()
    sequential, melody = 1 if mode == "sequential" else 0, 1 if melody_only else 0
    cap = int(lib.m2m_score_error_notes_capacity(R, L, sequential, max_labels, melody))
    need = int(lib.m2m_score_error_notes_workspace_bytes(T, frame_cap, melody))
    with torch.cuda.device(device):
        lab = torch.from_numpy(packed).to(device)
        off = torch.from_numpy(offsets).to(device)
        # (sizes the library will refuse are not allocated for: it answers on the arguments alone)
        workspace = torch.empty(max(need, 8) // 8, dtype=torch.int64, device=device)
        notes = torch.empty((T, 3, max(cap, 1), 3), dtype=torch.int32, device=device)
        counts = torch.empty((T, 3), dtype=torch.int32, device=device)
        native.check(lib.m2m_score_error_notes(
            dn.notes.data_ptr(), dn.counts.data_ptr(), dn.note_lp.data_ptr() if dn.note_lp is not None else None, R, L, sequential,
            float(dn.time_step), lab.data_ptr() if n_labels else None, off.data_ptr(), n_labels, T, frame_cap, floor, melody, max_labels,
            workspace.data_ptr(), need, notes.data_ptr(), counts.data_ptr(), native.stream_handle(device)), "m2m_score_error_notes")
    return ErrorNotes(notes, counts, dn.counts, bool(melody_only))


# ----------------------------------------------------------------------------------------------------------------- consensus
MAX_CANDIDATES = 16                      # M2M_CONSENSUS_MAX_CANDIDATES


class PairwiseCounts:
    """int64 numpy ``tp`` [B, K, K] and ``n`` [B, K] of ``consensus.pairwise_counts`` for every clip: ``tp[b, i, j]`` is the size of
    the maximum matching with candidate j as the reference and candidate i as the estimate, ``tp[b, i, i] = n[b, i]`` the kept
    notes of candidate i."""

    def __init__(self, tp: np.ndarray, n: np.ndarray):
        self.tp, self.n = tp, n


def _consensus_tolerances(who: str, onset_tolerance, offset_ratio, offset_min_tolerance) -> tuple:
    for name, value in (("onset_tolerance", onset_tolerance), ("offset_min_tolerance", offset_min_tolerance)):
        if not 0.0 <= float(value) <= 3600.0:
            raise ValueError(f"{who}: {name}={value} out of range [0, 3600] seconds")
    ratio = -1.0 if offset_ratio is None else float(offset_ratio)
    if offset_ratio is not None and not 0.0 <= ratio <= 1e6:
        raise ValueError(f"{who}: offset_ratio={offset_ratio} out of range [0, 1e6] (None: onsets only)")
    return float(onset_tolerance), ratio, float(offset_min_tolerance)


def _consensus_rows(who: str, token_ids, K) -> tuple:
    """(K, clips) for ids [B * K, L]; ``ValueError`` for a K outside 2..16, ids that are no 2-D int64 tensor or rows that are not
    whole clips."""
    from .consensus import check_candidates
    K = check_candidates(K, who)
    if not (isinstance(token_ids, torch.Tensor) and token_ids.dim() == 2 and token_ids.dtype == torch.int64):
        raise ValueError(f"{who}: token_ids must be an int64 tensor [clips * candidates, length]")
    R = int(token_ids.shape[0])
    if R % K != 0:
        raise ValueError(f"{who}: {R} rows are not whole clips of {K} candidates")
    return K, R // K


def _enqueue_pairwise(dn: DeviceNotes, K: int, onset_tolerance: float, offset_ratio: float, offset_min_tolerance: float) -> tuple:
    """The pairwise kernel of csrc/consensus.hip on the current stream: (tp [B, K, K], n [B, K]) int32 on the device.
    ``offset_ratio`` < 0: onsets only.  The workspace is torch's."""
    R, L = int(dn.notes.shape[0]), int(dn.notes.shape[1])
    device = dn.notes.device
    lib = native.load()
    need = int(lib.m2m_consensus_workspace_bytes(R, L, K))
    # (sizes the library will refuse are not allocated for: it answers on the arguments alone)
    workspace = torch.empty(max(need, 8) // 8, dtype=torch.int64, device=device)
    B = R // K
    tp = torch.empty((B, K, K), dtype=torch.int32, device=device)
    n = torch.empty((B, K), dtype=torch.int32, device=device)
    native.check(lib.m2m_consensus_pairwise_counts(
        dn.notes.data_ptr(), dn.counts.data_ptr(), R, L, K, float(dn.time_step), onset_tolerance, offset_ratio, offset_min_tolerance,
        workspace.data_ptr(), need, tp.data_ptr(), n.data_ptr(), native.stream_handle(device)), "m2m_consensus_pairwise_counts")
    return tp, n


def _enqueue_select(tp: torch.Tensor, n: torch.Tensor) -> tuple:
    """The select kernel on the current stream: (chosen [B] int32, utility [B, K] float64) on the device."""
    B, K = int(n.shape[0]), int(n.shape[1])
    device = tp.device
    chosen = torch.empty(B, dtype=torch.int32, device=device)
    utility = torch.empty((B, K), dtype=torch.float64, device=device)
    native.check(native.load().m2m_consensus_select(tp.data_ptr(), n.data_ptr(), B, K, chosen.data_ptr(), utility.data_ptr(),
                                                    native.stream_handle(device)), "m2m_consensus_select")
    return chosen, utility


def _consensus_tensors(who: str, tokenizer, token_ids, K, vocab_size, onset_tolerance, offset_ratio, offset_min_tolerance,
                       choose: bool) -> tuple:
    """The one path both public calls and ``generate_consensus`` take: (tp [B, K, K] int32, n [B, K] int32, counts [B * K] int32,
    chosen [B] int32, utility [B, K] float64) on the device of the ids, the last two ``None`` unless ``choose``.  Ids on a GPU go
    through the detokenise and the kernels on the current stream and nothing is copied to the host; ids on the host take the
    definition."""
    K, B = _consensus_rows(who, token_ids, K)
    onset, ratio, floor = _consensus_tolerances(who, onset_tolerance, offset_ratio, offset_min_tolerance)
    device = token_ids.device
    if B == 0:
        tp, n = torch.zeros((0, K, K), dtype=torch.int32, device=device), torch.zeros((0, K), dtype=torch.int32, device=device)
        counts, chosen = torch.zeros(0, dtype=torch.int32, device=device), torch.zeros(0, dtype=torch.int32, device=device)
        return tp, n, counts, chosen if choose else None, torch.zeros((0, K), dtype=torch.float64, device=device) if choose else None
    if not token_ids.is_cuda:
        from .consensus import pairwise_counts, select
        decoded = tokenizer.decode(token_ids, mode="batched")
        pairs = [pairwise_counts(decoded[b * K:(b + 1) * K], onset_tolerance, offset_ratio, offset_min_tolerance) for b in range(B)]
        tp = torch.from_numpy(np.stack([p[0] for p in pairs]).astype(np.int32))
        n = torch.from_numpy(np.stack([p[1] for p in pairs]).astype(np.int32))
        counts = torch.zeros(B * K, dtype=torch.int32)
        if not choose:
            return tp, n, counts, None, None
        picks = [select(*p) for p in pairs]
        return tp, n, counts, torch.tensor([p[0] for p in picks], dtype=torch.int32), torch.from_numpy(np.stack([p[1] for p in picks]))
    dn = detokenize(tokenizer, token_ids, "batched", None, vocab_size)
    with torch.cuda.device(device):
        tp, n = _enqueue_pairwise(dn, K, onset, ratio, floor)
        chosen, utility = _enqueue_select(tp, n) if choose else (None, None)
    return tp, n, dn.counts, chosen, utility


def pairwise_note_counts(tokenizer, token_ids: torch.Tensor, K: int, vocab_size: Optional[int] = None, onset_tolerance: float = 0.05,
                         offset_ratio: Optional[float] = 0.2, offset_min_tolerance: float = 0.05) -> PairwiseCounts:
    """``consensus.pairwise_counts`` of the K candidate rows of every clip for ids [B * K, L] on the device (rows b * K .. b * K + K - 1
    are clip b's, HF's ``repeat_interleave`` order): one detokenise in batched mode, one launch (csrc/consensus.hip), one copy of the
    integers to the host.  A row with an id outside the vocabulary raises ``ValueError`` as ``note_counts`` does.  Ids on the host
    take the definition."""
    tp, n, counts, _, _ = _consensus_tensors("pairwise_note_counts", tokenizer, token_ids, K, vocab_size, onset_tolerance, offset_ratio,
                                             offset_min_tolerance, choose=False)
    B, K = int(n.shape[0]), int(n.shape[1])
    host = torch.cat([tp.reshape(-1), n.reshape(-1), counts]).cpu().numpy()
    _raise_for_bad_rows(host[B * K * K + B * K:])
    return PairwiseCounts(host[:B * K * K].reshape(B, K, K).astype(np.int64), host[B * K * K:B * K * K + B * K].reshape(B, K).astype(np.int64))


def consensus_choice(tokenizer, token_ids: torch.Tensor, K: int, vocab_size: Optional[int] = None, onset_tolerance: float = 0.05,
                     offset_ratio: Optional[float] = 0.2, offset_min_tolerance: float = 0.05) -> tuple:
    """(chosen [B] int32 tensor, utility [B, K] float64 tensor) on the device of the ids: ``consensus.select`` of every clip's K
    candidate rows - the detokenise and both kernels of csrc/consensus.hip on the current stream, nothing copied to the host.  A clip
    that holds a row with an id outside the vocabulary gets ``chosen = -1`` and utilities 0.  Ids on the host take the definition."""
    return _consensus_tensors("consensus_choice", tokenizer, token_ids, K, vocab_size, onset_tolerance, offset_ratio,
                              offset_min_tolerance, choose=True)[3:]

