"""Per-note confidence from the log-probabilities of the tokens that made a note: the definition, on the host, in numpy.

``generate(..., return_dict_in_generate=True, output_logprobs=True)`` returns the log-probability of every token it selected.  A
note is made by six of them - the time, ONSET and pitch tokens of its onset and the time, OFFSET and pitch tokens of the event that
closes it - and its confidence is the product of their probabilities, computed as one float32 sum of logarithms in a fixed order:

    on    = (lp[time_col]  + lp[mode_col])  + lp[pitch_col]          time_col:  the latest time token
    off   = (lp[time_col'] + lp[mode_col']) + lp[pitch_col']         mode_col:  the latest ONSET (OFFSET) token since then
    total = on + off                                                 pitch_col: the note's (the event's) own pitch token
    confidence = exp(float64(total))

``note_columns`` is the state machine of ``MidiTokenizer._decode_tokens`` restated so that every note remembers those six columns;
the tokenizer itself stays the definition of the notes and is not touched.  One OFFSET pitch token closes every open earlier note of
its pitch: all of them get the same offset part.  Notes that are never closed are dropped, PAD / BOS are skipped, EOS ends the walk.

The device form is ``scoring.detokenize_scored`` (csrc/score.hip, ``m2m_score_detokenize_scored``); it equals this module bit for
bit, NaN payloads included.
"""
from __future__ import annotations

import math
from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from .tokenizer import BOS, EOS, OFFSET, ONSET, PAD


def _row(values, dtype) -> np.ndarray:
    if isinstance(values, torch.Tensor):
        values = values.detach().cpu().numpy()
    return np.asarray(values, dtype=dtype).reshape(-1)


def note_columns(tokenizer, tokens, start_idx: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """(notes_idx [n, 3] int64: onset index, offset index, pitch; cols [n, 6] int64: the columns of the onset's time, ONSET and
    pitch tokens and of the closing event's time, OFFSET and pitch tokens) of the closed notes of one row, in emission order."""
    time_offset, pitch_offset = int(tokenizer.time_token_offset), int(tokenizer.pitch_token_offset)
    velocity = tokenizer.config.default_velocity
    notes: List[list] = []                                   # [onset index, offset index or -1, pitch]
    cols: List[list] = []
    time_idx, mode, pitch = -1, -1, -1
    time_col, mode_col, pitch_col = -1, -1, -1
    for col, token in enumerate(_row(tokens, np.int64).tolist()):
        if token == EOS:
            break
        if token == BOS or token == PAD:
            continue
        if token == ONSET:
            mode, mode_col = 1, col
        elif token == OFFSET:
            mode, mode_col = 0, col
        if token >= time_offset:
            time_idx, mode, pitch = start_idx + token - time_offset, -1, -1
            time_col = col
        elif token >= pitch_offset:
            pitch, pitch_col = token - pitch_offset, col
        if time_idx == -1 or mode == -1 or pitch == -1:
            continue
        if mode * velocity:
            notes.append([time_idx, -1, pitch])
            cols.append([time_col, mode_col, pitch_col, -1, -1, -1])
        else:
            for note, c in zip(notes, cols):
                if note[2] == pitch and note[1] == -1 and note[0] < time_idx:
                    note[1] = time_idx
                    c[3:] = [time_col, mode_col, pitch_col]
        pitch = -1
    notes_idx = np.asarray(notes, dtype=np.int64).reshape(-1, 3)
    columns = np.asarray(cols, dtype=np.int64).reshape(-1, 6)
    closed = notes_idx[:, 1] != -1
    return notes_idx[closed], columns[closed]


def note_logprobs(tokenizer, tokens, token_logprobs, start_idx: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """(notes_idx [n, 3] int64, lp [n, 2] float32: the onset part and the offset part) of the closed notes of one row.
    ``token_logprobs[i]`` is the log-probability of ``tokens[i]``.  Every addition is a rounded float32 addition, in the order
    ``(time + mode) + pitch``; the note's total is ``float32(lp[:, 0] + lp[:, 1])``."""
    tokens = _row(tokens, np.int64)
    lp = _row(token_logprobs, np.float32)
    if lp.shape != tokens.shape:
        raise ValueError(f"note_logprobs: {lp.shape[0]} log-probabilities for {tokens.shape[0]} tokens")
    notes_idx, c = note_columns(tokenizer, tokens, start_idx)
    out = np.zeros((len(notes_idx), 2), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        out[:, 0] = (lp[c[:, 0]] + lp[c[:, 1]]) + lp[c[:, 2]]
        out[:, 1] = (lp[c[:, 3]] + lp[c[:, 4]]) + lp[c[:, 5]]
    return notes_idx, out


def min_logprob(min_confidence: float) -> np.float32:
    """The threshold the filter compares a note's float32 total with: ``float32(log(min_confidence))``, ``-inf`` for
    ``min_confidence <= 0``.  ``ValueError`` for a threshold above 1 or NaN."""
    c = float(min_confidence)
    if math.isnan(c) or c > 1.0:
        raise ValueError(f"min_confidence has to be a probability (at most 1; 0 or below keeps every note), but is {min_confidence!r}")
    return np.float32(-np.inf) if c <= 0.0 else np.float32(np.log(c))


def total_logprob(lp: np.ndarray) -> np.ndarray:
    """float32 ``on + off`` of [n, 2] parts."""
    lp = np.asarray(lp, dtype=np.float32).reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        return lp[:, 0] + lp[:, 1]


def confidence_of(lp: np.ndarray) -> np.ndarray:
    """float64 ``exp`` of the float32 total of [n, 2] parts."""
    with np.errstate(over="ignore"):
        return np.exp(total_logprob(lp).astype(np.float64))


def keep_mask(lp: np.ndarray, min_confidence: float) -> np.ndarray:
    """The filter: a note is dropped iff ``total < min_logprob(min_confidence)`` is true in float32."""
    with np.errstate(invalid="ignore"):
        return ~(total_logprob(lp) < min_logprob(min_confidence))


def decode_with_confidence(tokenizer, tokens_batch, logprobs_batch, mode: str = "batched", duration_per_batch: Optional[float] = None,
                           min_confidence: float = 0.0) -> Tuple[Union[List[np.ndarray], np.ndarray], Union[List[np.ndarray], np.ndarray]]:
    """``tokenizer.decode(tokens_batch, mode, duration_per_batch)`` with a confidence per note: ``(notes, confidence)`` - a list of
    [n_i, 4] float64 arrays and a list of [n_i] float64 arrays, or their concatenations in ``sequential`` mode.
    ``confidence = np.exp(total.astype(np.float64))`` of the float32 ``total`` of ``note_logprobs``.

    The filter: a note is dropped iff ``total < min_logprob`` is TRUE in float32, where ``min_logprob =
    np.float32(np.log(min_confidence))``, or ``-inf`` for ``min_confidence <= 0``.  So a note whose total is NaN is kept under
    every threshold (the comparison is false), a note whose total is ``-inf`` is dropped by any positive threshold, and a note
    whose total equals the threshold is kept.  ``min_confidence > 1`` or NaN raises ``ValueError``.  With ``min_confidence=0`` the
    notes are exactly ``tokenizer.decode(...)``, whatever the log-probabilities."""
    if mode == "batched":
        steps = 0
    elif mode == "sequential":
        if duration_per_batch is None:
            raise ValueError('duration_per_batch is required for mode="sequential"')
        steps = round(duration_per_batch / tokenizer.time_step)
    else:
        raise ValueError(f"Invalid argument mode={mode}")
    floor = min_logprob(min_confidence)
    tokens_batch, logprobs_batch = list(tokens_batch), list(logprobs_batch)
    if len(tokens_batch) != len(logprobs_batch):
        raise ValueError(f"decode_with_confidence: {len(logprobs_batch)} log-probability rows for {len(tokens_batch)} token rows")
    notes_parts, conf_parts = [], []
    for i, (tokens, lps) in enumerate(zip(tokens_batch, logprobs_batch)):
        notes_idx, lp = note_logprobs(tokenizer, tokens, lps, i * steps)
        total = total_logprob(lp)
        with np.errstate(invalid="ignore"):
            keep = ~(total < floor)
        notes = np.zeros((int(keep.sum()), 4), dtype=np.float64)
        notes[:, :3] = notes_idx[keep]
        notes[:, 3] = tokenizer.config.default_velocity
        notes[:, :2] = notes[:, :2] * tokenizer.time_step
        notes_parts.append(notes)
        with np.errstate(over="ignore"):
            conf_parts.append(np.exp(total[keep].astype(np.float64)))
    if mode == "batched":
        return notes_parts, conf_parts
    return np.concatenate(notes_parts), np.concatenate(conf_parts)


def confidence_velocities(confidence: np.ndarray) -> np.ndarray:
    """MIDI velocities from confidences: ``max(1, min(127, int(round(127 * c))))`` per note (a NaN confidence gives 1)."""
    out = np.empty(len(confidence), dtype=np.float64)
    for i, c in enumerate(np.asarray(confidence, dtype=np.float64).tolist()):
        v = 127.0 * c
        out[i] = 1 if math.isnan(v) else max(1, min(127, int(round(min(v, 1e9)))))
    return out
