"""Frame-level piano-roll scores and the TP / FN / FP error roll: the definition, on the host, in numpy.

``evaluate_midi_result``, ``piano_roll_to_instrument`` and ``extract_melody_from_piano_roll`` of the reference
(ref: music2midi/plot_midi.py:19-135) restated for this project's note arrays ([n, 4] float64: start, end, pitch, velocity) without
pretty_midi, numba or bokeh.  It is a restatement with line references, like ``evaluation.py``: the reference's file cannot be run
where this project is built (its imports are absent), so nothing here is a recorded run of it.  The bokeh figures are out of scope.

Everything stands on ``evaluation.piano_roll``, ``evaluation.highest_pitches`` and the ``n_frames`` rule of
``evaluation.extract_midi_melody``: ``n_frames = len(np.arange(0, max(end of both), 1 / 100))``, a note sounds in
``[int(start * 100), int(end * 100))`` cut at ``n_frames - 1``, the last frame stays silent.  A note with ``end <= start`` does not
exist (``numpy_to_midi`` drops it); pitch and velocity are ``int(...)`` of the array's, as ``numpy_to_midi`` stores them.

    sounding(notes, n_frames)                     -> bool [128, n_frames]
    melody_roll(roll)                             -> bool [12, n_frames]       (ref plot_midi.py:74-99)
    error_rolls(ref, est, melody_only=False)      -> (tp, fn, fp) bool rolls   (ref plot_midi.py:113-126)
    roll_to_notes(roll)                           -> [n, 4] float64            (ref plot_midi.py:19-70)
    frame_counts(ref, est)                        -> (tp, fn, fp, melody_tp, melody_fn, melody_fp) ints
    evaluate_midi_result(target, predict, melody_only=False) -> MIDI object with the instruments TP, FN, FP

Precision, recall and F1 of the counts are ``note_metrics.precision_recall_f1(tp, tp + fn, tp + fp)``.  The device form is
``scoring.frame_counts`` / ``scoring.error_notes`` (csrc/frame_roll.hip); it equals this module.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

from .evaluation import _end_time, _notes_of, highest_pitches, piano_roll

FS = 100
KINDS = ("TP", "FN", "FP")


def _kept(notes) -> np.ndarray:
    """[n, 4] float64 of a MIDI object or a note array: the notes with end > start, pitch and velocity truncated to integers."""
    a = np.array(_notes_of(notes if hasattr(notes, "instruments") else np.asarray(notes, dtype=np.float64)), dtype=np.float64)
    with np.errstate(invalid="ignore"):
        a = a[a[:, 1] > a[:, 0]]
    a[:, 2:] = np.trunc(a[:, 2:])
    return a


def n_frames_of(ref_notes, est_notes) -> int:
    """``len(np.arange(0, end, 1 / 100))`` for the later end of both sides (ref plot_midi.py:114-117); 0 with both sides empty."""
    end_time = max(_end_time(_kept(ref_notes)), _end_time(_kept(est_notes)))
    return len(np.arange(0, end_time, 1 / FS))


def sounding(notes, n_frames: int) -> np.ndarray:
    """bool [128, n_frames]: the cells in which a note sounds."""
    return piano_roll(_kept(notes), n_frames, FS) != 0


def melody_roll(roll: np.ndarray) -> np.ndarray:
    """bool [12, n_frames]: in every frame where anything sounds, the row ``highest pitch % 12``."""
    top = highest_pitches(np.asarray(roll, dtype=np.float64))
    out = np.zeros((12, roll.shape[1]), dtype=bool)
    frames = np.flatnonzero(top >= 0)
    out[top[frames] % 12, frames] = True
    return out


def error_rolls(ref_notes, est_notes, melody_only: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(tp, fn, fp) = (ref & est, ref & ~est, ~ref & est) of the two rolls, [128, n_frames] or, ``melody_only``, [12, n_frames]."""
    n_frames = n_frames_of(ref_notes, est_notes)
    ref, est = sounding(ref_notes, n_frames), sounding(est_notes, n_frames)
    if melody_only:
        ref, est = melody_roll(ref), melody_roll(est)
    return ref & est, ref & ~est, ~ref & est


def roll_to_notes(roll: np.ndarray) -> np.ndarray:
    """[n, 4] float64 (start, end, pitch, velocity 1) of a boolean roll: every maximal run of ``True`` in a row is one note,
    ``start = first_frame / 100``, ``end = (last_frame + 1) / 100``.  Order: ascending end frame, then ascending pitch - the
    reference appends a note at its falling edge while walking ``np.nonzero(diff.T)``."""
    roll = np.asarray(roll, dtype=bool)
    padded = np.pad(roll, [(0, 0), (1, 1)], "constant")
    changes = np.nonzero(np.diff(padded).T)                  # np.diff of booleans is XOR: (frame, row) of every edge, frame-major
    on_frame = np.zeros(roll.shape[0], dtype=np.int64)
    notes = []
    for frame, row in zip(*changes):
        if padded[row, frame + 1]:
            on_frame[row] = frame
        else:
            notes.append((on_frame[row] / FS, frame / FS, float(row), 1.0))
    return np.asarray(notes, dtype=np.float64).reshape(-1, 4)


def frame_counts(ref_notes, est_notes) -> Tuple[int, int, int, int, int, int]:
    """(tp, fn, fp) of the full roll, then (tp, fn, fp) of the melody roll: the set cells of ``error_rolls``."""
    full = error_rolls(ref_notes, est_notes)
    melody = error_rolls(ref_notes, est_notes, melody_only=True)
    return tuple(int(r.sum()) for r in full + melody)


def error_midi(tp_notes, fn_notes, fp_notes):
    """The three-instrument MIDI object (TP, FN, FP; programs 0, 1, 2) of three [n, 4] note arrays: a real ``PrettyMIDI`` when
    pretty_midi is installed, else ``utils.SimpleMIDI``."""
    from . import utils
    if utils._pm is not None:
        midi = utils._pm.PrettyMIDI()
        make_inst, make_note = utils._pm.Instrument, lambda s, e, p, v: utils._pm.Note(velocity=int(v), pitch=int(p), start=s, end=e)
    else:
        midi = utils.SimpleMIDI()
        make_inst, make_note = utils.SimpleInstrument, utils.SimpleNote
    for program, (name, notes) in enumerate(zip(KINDS, (tp_notes, fn_notes, fp_notes))):
        inst = make_inst(program=program, name=name)
        inst.notes = [make_note(float(s), float(e), int(p), int(v)) for s, e, p, v in np.asarray(notes, dtype=np.float64).reshape(-1, 4)]
        midi.instruments.append(inst)
    return midi


def evaluate_midi_result(target, predict, melody_only: bool = False):
    """ref plot_midi.py:102-135: the MIDI object with the instruments TP, FN and FP (programs 0, 1, 2) of ``target`` against
    ``predict``, MIDI objects or note arrays.  ``melody_only``: on the 12-row melody roll, the pitches are pitch classes."""
    return error_midi(*(roll_to_notes(r) for r in error_rolls(target, predict, melody_only)))
