"""Note-level precision, recall and F1: the definition, on the host, in numpy + scipy.

``mir_eval.transcription.match_notes`` / ``precision_recall_f1_overlap`` restated for this project's note arrays ([n, 4] float64:
start, end, pitch, velocity) without mir_eval or pretty_midi:

    match_counts(ref_notes, est_notes, onset_tolerance=0.05, offset_ratio=0.2 | None, offset_min_tolerance=0.05) -> (tp, n_ref, n_est)
    precision_recall_f1(tp, n_ref, n_est)                                                                        -> (p, r, f)

Both sides keep only the notes with ``end > start``, as ``numpy_to_midi`` does; the pitch is ``int(pitch)``.  A reference note and an
estimated note hit when

    onset   np.around(np.abs(ref_on - est_on), 6) <= onset_tolerance        (mir_eval's 6-decimal rounding, non-strict)
    pitch   the integer pitches are equal                                   (mir_eval's 50 cents, on MIDI pitches)
    offset  np.around(np.abs(ref_off - est_off), 6) <= max(offset_ratio * (ref_off - ref_on), offset_min_tolerance)
            - only with ``offset_ratio`` not ``None``; ``None`` is the onset-only metric

and ``tp`` is the size of a maximum matching of the hit graph (``scipy.sparse.csgraph.maximum_bipartite_matching``).  The size is
unique, so the three integers compare with ``==``.  mir_eval's average overlap ratio depends on WHICH maximum matching is found
and is deliberately not provided.  A micro-average over timelines sums the three integers first.

The device form is ``scoring.note_counts`` (csrc/note_match.hip, ``m2m_score_note_counts``); it equals this module.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np


def _kept(notes) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(onsets, offsets, int pitches) of the notes with end > start."""
    a = np.asarray(notes, dtype=np.float64).reshape(-1, 4)
    with np.errstate(invalid="ignore"):
        a = a[a[:, 1] > a[:, 0]]
    return a[:, 0], a[:, 1], np.asarray([int(p) for p in a[:, 2].tolist()], dtype=np.int64)


def hit_matrix(ref_notes, est_notes, onset_tolerance: float = 0.05, offset_ratio: Optional[float] = 0.2,
               offset_min_tolerance: float = 0.05) -> np.ndarray:
    """[n_ref, n_est] bool: the hit graph of the kept notes."""
    ref_on, ref_off, ref_pitch = _kept(ref_notes)
    est_on, est_off, est_pitch = _kept(est_notes)
    hits = np.around(np.abs(ref_on[:, None] - est_on[None, :]), 6) <= onset_tolerance
    hits &= ref_pitch[:, None] == est_pitch[None, :]
    if offset_ratio is not None:
        tolerance = np.maximum(offset_ratio * (ref_off - ref_on), offset_min_tolerance)
        hits &= np.around(np.abs(ref_off[:, None] - est_off[None, :]), 6) <= tolerance[:, None]
    return hits


def match_counts(ref_notes, est_notes, onset_tolerance: float = 0.05, offset_ratio: Optional[float] = 0.2,
                 offset_min_tolerance: float = 0.05) -> Tuple[int, int, int]:
    """(tp, n_ref, n_est): the size of a maximum matching of the hit graph and the kept notes of both sides."""
    hits = hit_matrix(ref_notes, est_notes, onset_tolerance, offset_ratio, offset_min_tolerance)
    n_ref, n_est = hits.shape
    if n_ref == 0 or n_est == 0 or not hits.any():
        return 0, int(n_ref), int(n_est)
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import maximum_bipartite_matching
    matched = maximum_bipartite_matching(csr_matrix(hits), perm_type="column")
    return int((matched >= 0).sum()), int(n_ref), int(n_est)


def precision_recall_f1(tp, n_ref, n_est) -> Tuple[float, float, float]:
    """``p = tp / n_est``, ``r = tp / n_ref``, ``f = 2 p r / (p + r)`` in float64; (0, 0, 0) when either side is empty and
    ``f = 0.0`` when ``p + r == 0``."""
    tp, n_ref, n_est = int(tp), int(n_ref), int(n_est)
    if n_ref == 0 or n_est == 0:
        return 0.0, 0.0, 0.0
    p, r = tp / n_est, tp / n_ref
    return p, r, (2 * p * r / (p + r) if p + r != 0 else 0.0)
