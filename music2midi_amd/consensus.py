"""Consensus (minimum-Bayes-risk) selection among K transcriptions of one clip: the definition, on the host, in numpy.

A candidate is a note array [n, 4] as ``tokenizer.decode(..., mode="batched")`` returns it.  Every candidate is scored against
every other one with the note-level metric of ``music2midi_amd.note_metrics`` and the one the others agree with most is chosen:

    pairwise_counts(candidates, onset_tolerance=0.05, offset_ratio=0.2 | None, offset_min_tolerance=0.05) -> (tp [K, K], n [K]) int64
    agreement(tp, n_est, n_ref)          -> float      1.0 for two silent candidates, else 2 * tp / (n_est + n_ref)
    expected_agreement(tp, n)            -> u [K]      the mean agreement of candidate i with the K - 1 others
    select(tp, n)                        -> (index, u) the first maximum of u: candidate 0 is the greedy row, so ties go to greedy

``tp[i, j]`` takes candidate j as the reference and candidate i as the estimate; with offsets it is not symmetric, because the
offset tolerance comes from the reference note's duration.  ``tp[i, i] = n[i]`` is set, not computed.  K is 2..16.

The device form is ``scoring.pairwise_note_counts`` / ``scoring.consensus_choice`` (csrc/consensus.hip); it equals this module,
integer for integer and bit for bit.  Whether the chosen candidate is a better transcription than the greedy one on a trained model
has not been measured.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

from .note_metrics import _kept, match_counts

MAX_CANDIDATES = 16                      # M2M_CONSENSUS_MAX_CANDIDATES


def check_candidates(K, who: str = "consensus") -> int:
    """K as an int; ``ValueError`` unless 2 <= K <= 16."""
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 2 <= int(K) <= MAX_CANDIDATES:
        raise ValueError(f"{who}: {K} candidates out of range (2..{MAX_CANDIDATES})")
    return int(K)


def pairwise_counts(candidates: Sequence, onset_tolerance: float = 0.05, offset_ratio: Optional[float] = 0.2,
                    offset_min_tolerance: float = 0.05) -> Tuple[np.ndarray, np.ndarray]:
    """(tp [K, K] int64, n [K] int64): ``tp[i, j] = match_counts(ref=candidates[j], est=candidates[i])[0]`` for i != j, ``n[i]`` the
    kept notes (``end > start``) of candidate i, ``tp[i, i] = n[i]``."""
    K = check_candidates(len(candidates), "pairwise_counts")
    n = np.asarray([len(_kept(c)[0]) for c in candidates], dtype=np.int64)
    tp = np.zeros((K, K), dtype=np.int64)
    for i in range(K):
        for j in range(K):
            if i == j:
                tp[i, i] = n[i]
            else:
                tp[i, j] = match_counts(candidates[j], candidates[i], onset_tolerance, offset_ratio, offset_min_tolerance)[0]
    return tp, n


def agreement(tp, n_est, n_ref) -> float:
    """The F1 of two note lists from the three integers, in float64: ``2 * tp / (n_est + n_ref)``; 1.0 when both are empty - two
    silent candidates agree (``note_metrics.precision_recall_f1`` returns 0 there and is deliberately not used)."""
    tp, n_est, n_ref = int(tp), int(n_est), int(n_ref)
    if n_est + n_ref == 0:
        return 1.0
    return 2 * tp / (n_est + n_ref)


def expected_agreement(tp, n) -> np.ndarray:
    """u [K] float64: ``u[i] = (sum over j != i of agreement(tp[i, j], n[i], n[j])) / (K - 1)``, the sum in float64, left to right
    in increasing j."""
    tp, n = np.asarray(tp, dtype=np.int64), np.asarray(n, dtype=np.int64)
    K = check_candidates(len(n), "expected_agreement")
    if tp.shape != (K, K):
        raise ValueError(f"expected_agreement: tp of shape {tp.shape} for {K} candidates")
    u = np.zeros(K, dtype=np.float64)
    for i in range(K):
        total = 0.0
        for j in range(K):
            if j != i:
                total = total + agreement(tp[i, j], n[i], n[j])
        u[i] = total / (K - 1)
    return u


def select(tp, n) -> Tuple[int, np.ndarray]:
    """(index of the first maximum of ``expected_agreement(tp, n)``, that array)."""
    u = expected_agreement(tp, n)
    return int(np.argmax(u)), u
