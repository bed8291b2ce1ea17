"""Melody chroma accuracy (ref: music2midi/evaluation.py:10-75) without
librosa / mir_eval / numba / pretty_midi.

Pipeline restated: piano roll at 100 frames/s -> highest sounding pitch per
frame -> ``mir_eval.melody.raw_chroma_accuracy`` between target and output.

One deliberate difference, documented rather than imitated:
for a frame in which nothing sounds the reference indexes ``onset_pitches[-1]``
of an EMPTY array inside ``numba.njit`` (no bounds check) after storing NaN into
an int array (ref evaluation.py:15-18) — undefined values.  Here such a frame is
*unvoiced* (frequency 0), which is what the metric's voicing logic expects.
"""
from __future__ import annotations

from typing import Iterable, Tuple

import numpy as np


def _notes_of(midi) -> np.ndarray:
    if isinstance(midi, np.ndarray):
        return midi.reshape(-1, 4)
    rows = [[n.start, n.end, n.pitch, n.velocity] for inst in midi.instruments for n in inst.notes]
    return np.asarray(rows, dtype=np.float64).reshape(-1, 4)


def _end_time(notes: np.ndarray) -> float:
    return float(notes[:, 1].max()) if len(notes) else 0.0


def piano_roll(notes: np.ndarray, n_frames: int, fs: int = 100) -> np.ndarray:
    """[128, n_frames] velocity sums; a note sounds in frames [int(start*fs), int(end*fs)).
    The last frame stays zero, as pretty_midi's ``get_piano_roll(times=...)`` leaves it."""
    roll = np.zeros((128, n_frames))
    for start, end, pitch, vel in notes:
        a, b = int(start * fs), int(end * fs)
        roll[int(pitch), a:min(b, n_frames - 1)] += vel
    return roll


def highest_pitches(roll: np.ndarray) -> np.ndarray:
    """Highest sounding pitch per frame, -1 where the frame is silent."""
    active = roll > 0
    idx = 127 - np.argmax(active[::-1], axis=0)
    return np.where(active.any(axis=0), idx, -1).astype(np.int64)


def extract_midi_melody(target, output, fs: int = 100) -> Tuple[np.ndarray, np.ndarray]:
    tn, on = _notes_of(target), _notes_of(output)
    end_time = max(_end_time(tn), _end_time(on))
    n_frames = len(np.arange(0, end_time, 1 / fs))
    return highest_pitches(piano_roll(tn, n_frames, fs)), highest_pitches(piano_roll(on, n_frames, fs))


def _cents(pitch: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    voiced = pitch >= 0
    hz = np.where(voiced, 440.0 * 2.0 ** ((pitch - 69) / 12.0), 0.0)
    cent = np.zeros_like(hz)
    cent[voiced] = 1200.0 * np.log2(hz[voiced] / 10.0)   # mir_eval.melody.hz2cents base 10 Hz
    return voiced, cent


def melody_chroma_accuracy(ref_pitch: np.ndarray, est_pitch: np.ndarray, cent_tolerance: float = 50.0) -> float:
    assert ref_pitch.shape == est_pitch.shape
    ref_v, ref_c = _cents(ref_pitch)
    est_v, est_c = _cents(est_pitch)
    if ref_v.size == 0 or ref_v.sum() == 0:
        return 0.0
    nonzero = np.logical_and(est_c != 0, ref_c != 0)
    if nonzero.sum() == 0:
        return 0.0
    diff = np.abs(ref_c - est_c)[nonzero]
    octave = 1200.0 * np.floor(diff / 1200.0 + 0.5)
    correct = np.abs(diff - octave) < cent_tolerance
    return float(np.sum(ref_v[nonzero] * correct) / np.sum(ref_v))


def evaluate_batch(targets: Iterable, outputs: Iterable) -> float:
    pairs = [extract_midi_melody(t, o) for t, o in zip(targets, outputs)]
    if not pairs:
        return 0.0
    ts, os_ = zip(*pairs)
    return melody_chroma_accuracy(np.concatenate(ts), np.concatenate(os_))


def evaluate_tokens(tokenizer, token_ids, notes_batch, mode: str = "batched", duration_per_batch=None, token_logprobs=None,
                    min_confidence: float = 0.0) -> float:
    """``evaluate_batch(numpy_to_midi(labels), numpy_to_midi(tokenizer.decode(token_ids, mode, duration_per_batch)))`` for token ids
    that are on the GPU, computed there (``music2midi_amd.scoring``, csrc/score.hip): the same float, not a close one - for integer
    pitches the 50-cent octave-folded test is "the pitches differ by a multiple of 12", so the score is a ratio of two frame counts.
    ``notes_batch``: one label array per row, or ONE array in ``sequential`` mode.  ``ValueError`` for labels the device path does
    not take (``scoring.labels_eligible``).  With ``token_logprobs`` (the log-probability of every id, column-aligned) only the
    decoded notes of at least ``min_confidence`` are scored (``music2midi_amd.confidence``)."""
    from .scoring import chroma_counts
    if token_logprobs is None and not min_confidence > 0:
        return chroma_counts(tokenizer, token_ids, notes_batch, mode, duration_per_batch).score
    return chroma_counts(tokenizer, token_ids, notes_batch, mode, duration_per_batch, token_logprobs=token_logprobs,
                         min_confidence=min_confidence).score


def note_scores(tp, n_est, n_ref) -> dict:
    """The dict the note-level scorers return, from [T, K] (or [K]) integers: ``tp``, ``n_est``, ``n_ref`` [K] int64 summed over the
    timelines, and ``precision``, ``recall``, ``f1`` [K] float64 of those sums (``note_metrics.precision_recall_f1``)."""
    from .note_metrics import precision_recall_f1
    tp, n_est, n_ref = (np.asarray(a, dtype=np.int64).reshape(-1, np.shape(a)[-1]).sum(axis=0) for a in (tp, n_est, n_ref))
    prf = np.asarray([precision_recall_f1(*s) for s in zip(tp.tolist(), n_ref.tolist(), n_est.tolist())], dtype=np.float64).reshape(-1, 3)
    return {"precision": prf[:, 0].copy(), "recall": prf[:, 1].copy(), "f1": prf[:, 2].copy(), "tp": tp, "n_est": n_est, "n_ref": n_ref}


def note_scores_tokens(tokenizer, token_ids, notes_batch, mode: str = "batched", duration_per_batch=None, token_logprobs=None,
                       thresholds=None, offset_ratio=0.2, onset_tolerance: float = 0.05, offset_min_tolerance: float = 0.05) -> dict:
    """Note-level precision, recall and F1 (``music2midi_amd.note_metrics``: mir_eval.transcription's matching) of token ids that are
    on the GPU against their label notes, for every confidence threshold of ``thresholds`` (``None``: ``[0.0]``), computed there
    (``scoring.note_counts``, csrc/note_match.hip): ``{"precision", "recall", "f1"}`` [K] float64, micro-averaged over the
    timelines, and ``{"tp", "n_est", "n_ref"}`` [K] int64, the sums they are ratios of.  ``offset_ratio=None`` matches onsets only.
    Positive thresholds need ``token_logprobs``; ``ValueError`` for labels the device path does not take."""
    from .scoring import note_counts
    c = note_counts(tokenizer, token_ids, notes_batch, mode, duration_per_batch, token_logprobs=token_logprobs, thresholds=thresholds,
                    onset_tolerance=onset_tolerance, offset_ratio=offset_ratio, offset_min_tolerance=offset_min_tolerance)
    return note_scores(c.tp, c.n_est, c.n_ref)


def note_scores_host(tokenizer, token_ids, notes_batch, mode: str = "batched", duration_per_batch=None, token_logprobs=None,
                     thresholds=None, offset_ratio=0.2, onset_tolerance: float = 0.05, offset_min_tolerance: float = 0.05) -> dict:
    """``note_scores_tokens`` by the definition alone, for ids anywhere and any labels: ``confidence.decode_with_confidence`` per
    threshold (``tokenizer.decode`` without log-probabilities), then ``note_metrics.match_counts`` per timeline."""
    from .note_metrics import match_counts
    from .scoring import threshold_logprobs
    threshold_logprobs(thresholds, token_logprobs is not None, "note_scores_host")
    values = [0.0] if thresholds is None else [float(c) for c in thresholds]
    labels = [notes_batch] if mode == "sequential" else list(notes_batch)
    counts = np.zeros((len(labels), len(values), 3), dtype=np.int64)
    for k, c in enumerate(values):
        if token_logprobs is None:
            decoded = tokenizer.decode(token_ids, mode=mode, duration_per_batch=duration_per_batch)
        else:
            from .confidence import decode_with_confidence
            decoded, _ = decode_with_confidence(tokenizer, token_ids, token_logprobs, mode, duration_per_batch, c)
        decoded = [decoded] if mode == "sequential" else list(decoded)
        if len(decoded) != len(labels):
            raise ValueError(f"note_scores_host: {len(labels)} label arrays for {len(decoded)} timelines")
        for t, (want, got) in enumerate(zip(labels, decoded)):
            tp, n_ref, n_est = match_counts(want, got, onset_tolerance, offset_ratio, offset_min_tolerance)
            counts[t, k] = (tp, n_est, n_ref)
    return note_scores(counts[:, :, 0], counts[:, :, 1], counts[:, :, 2])


_FRAME_KEYS = ("tp", "fn", "fp")


def frame_scores(tp, fn, fp, melody_tp=None, melody_fn=None, melody_fp=None) -> dict:
    """The dict the frame-level scorers return, from [T, K] (or [K]) integers: ``tp``, ``fn``, ``fp`` [K] int64 summed over the
    timelines and ``precision``, ``recall``, ``f1`` [K] float64 of those sums
    (``note_metrics.precision_recall_f1(tp, tp + fn, tp + fp)``); with the melody roll's integers the same keys again with a
    ``melody_`` prefix."""
    from .note_metrics import precision_recall_f1
    out = {}
    for prefix, triple in (("", (tp, fn, fp)), ("melody_", (melody_tp, melody_fn, melody_fp))):
        if triple[0] is None:
            continue
        a, b, c = (np.asarray(x, dtype=np.int64).reshape(-1, np.shape(x)[-1]).sum(axis=0) for x in triple)
        prf = np.asarray([precision_recall_f1(i, i + j, i + k) for i, j, k in zip(a.tolist(), b.tolist(), c.tolist())],
                         dtype=np.float64).reshape(-1, 3)
        out.update({prefix + "precision": prf[:, 0].copy(), prefix + "recall": prf[:, 1].copy(), prefix + "f1": prf[:, 2].copy(),
                    prefix + "tp": a, prefix + "fn": b, prefix + "fp": c})
    return out


def frame_scores_tokens(tokenizer, token_ids, notes_batch, mode: str = "batched", duration_per_batch=None, token_logprobs=None,
                        thresholds=None) -> dict:
    """Frame-level precision, recall and F1 (``music2midi_amd.frame_metrics``: the piano rolls at 100 frames per second of
    ref plot_midi.py's ``evaluate_midi_result``) of token ids that are on the GPU against their label notes, for every confidence
    threshold of ``thresholds`` (``None``: ``[0.0]``), computed there (``scoring.frame_counts``, csrc/frame_roll.hip):
    ``{"precision", "recall", "f1"}`` [K] float64, micro-averaged over the timelines, ``{"tp", "fn", "fp"}`` [K] int64, and the same
    six with a ``melody_`` prefix for the 12-row melody roll.  Positive thresholds need ``token_logprobs``; ``ValueError`` for labels
    the device path does not take."""
    from .scoring import frame_counts
    c = frame_counts(tokenizer, token_ids, notes_batch, mode, duration_per_batch, token_logprobs=token_logprobs, thresholds=thresholds)
    return frame_scores(c.tp, c.fn, c.fp, c.melody_tp, c.melody_fn, c.melody_fp)


def frame_scores_host(tokenizer, token_ids, notes_batch, mode: str = "batched", duration_per_batch=None, token_logprobs=None,
                      thresholds=None) -> dict:
    """``frame_scores_tokens`` by the definition alone, for ids anywhere and any labels: ``confidence.decode_with_confidence`` per
    threshold (``tokenizer.decode`` without log-probabilities), then ``frame_metrics.frame_counts`` per timeline."""
    from .frame_metrics import frame_counts
    from .scoring import threshold_logprobs
    threshold_logprobs(thresholds, token_logprobs is not None, "frame_scores_host")
    values = [0.0] if thresholds is None else [float(c) for c in thresholds]
    labels = [notes_batch] if mode == "sequential" else list(notes_batch)
    counts = np.zeros((len(labels), len(values), 6), dtype=np.int64)
    for k, c in enumerate(values):
        if token_logprobs is None:
            decoded = tokenizer.decode(token_ids, mode=mode, duration_per_batch=duration_per_batch)
        else:
            from .confidence import decode_with_confidence
            decoded, _ = decode_with_confidence(tokenizer, token_ids, token_logprobs, mode, duration_per_batch, c)
        decoded = [decoded] if mode == "sequential" else list(decoded)
        if len(decoded) != len(labels):
            raise ValueError(f"frame_scores_host: {len(labels)} label arrays for {len(decoded)} timelines")
        for t, (want, got) in enumerate(zip(labels, decoded)):
            counts[t, k] = frame_counts(want, got)
    return frame_scores(*(counts[:, :, i] for i in range(6)))


def evaluate_midi_result(target, predict, melody_only: bool = False):
    """ref plot_midi.py:102-135: the MIDI object with the instruments TP, FN, FP (``frame_metrics.evaluate_midi_result``)."""
    from .frame_metrics import evaluate_midi_result as definition
    return definition(target, predict, melody_only)
