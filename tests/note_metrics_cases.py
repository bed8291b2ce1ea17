"""Inputs the CPU and GPU tests of the note-level metrics share: the crafted cases with their stated counts, and id rows that decode
to a given list of notes.  Decoded times lie on the tokenizer's 50 ms grid (index * 0.05), label times are plain float64."""
import copy

import numpy as np

from music2midi_amd.config import DEFAULT_CONFIG, load_config
from music2midi_amd.tokenizer import EOS, OFFSET, ONSET, PAD, MidiTokenizer

TOK = MidiTokenizer(load_config(copy.deepcopy(DEFAULT_CONFIG)))
STEP = TOK.time_step
assert STEP == 0.05


def ref(*notes):
    """[n, 4] float64 label notes from (start, end, pitch) triples, velocity 80."""
    return np.asarray([[s, e, p, 80.0] for s, e, p in notes], dtype=np.float64).reshape(-1, 4)


def est_seconds(idx_notes):
    """[n, 4] float64: (onset index, offset index, pitch) triples as ``tokenizer.decode`` returns them."""
    out = np.zeros((len(idx_notes), 4), dtype=np.float64)
    for i, (on, off, pitch) in enumerate(idx_notes):
        out[i] = (on, off, pitch, TOK.config.default_velocity)
    out[:, :2] = out[:, :2] * STEP
    return out


def id_row(idx_notes, first_index=0):
    """Token ids that decode to exactly these notes, in this order: one closed group of six ids per note (time, ONSET, pitch, time,
    OFFSET, pitch).  The time may go backwards between groups, so notes of one pitch may overlap; an OFFSET closes only notes that are
    still open, and every earlier note is closed already.  ``first_index`` is subtracted from the time indices (sequential rows)."""
    row = []
    for on, off, pitch in idx_notes:
        assert 0 <= on - first_index < off - first_index < TOK.model_vocab_size - TOK.time_token_offset and 0 <= pitch < 128
        row += [TOK.time_token_offset + on - first_index, ONSET, TOK.pitch_token_offset + pitch,
                TOK.time_token_offset + off - first_index, OFFSET, TOK.pitch_token_offset + pitch]
    return row + [EOS]


def id_rows(notes_per_row, width, steps_per_row=0):
    ids = np.full((len(notes_per_row), width), PAD, dtype=np.int64)
    for r, notes in enumerate(notes_per_row):
        row = id_row(notes, r * steps_per_row)
        assert len(row) <= width, (len(row), width)
        ids[r, :len(row)] = row
    return ids


# name -> (label notes, decoded notes as index triples, (tp, n_ref, n_est) with offset_ratio=0.2, the same with offset_ratio=None)
CRAFTED = {
    # A hits X and Y, B hits X only: first-fit gives A <- X and leaves B alone; the maximum matching is A <- Y, B <- X
    "augmenting path": (ref((1.00, 2.00, 60), (1.04, 1.80, 60)), [(20, 37, 60), (21, 42, 60)], (2, 2, 2), (2, 2, 2)),
    # abs(1.0 - 21 * 0.05) = 0.050000000000000044: a hit only after the rounding to 6 decimals
    "onset on the rounded tolerance": (ref((1.0, 1.5, 60)), [(21, 30, 60)], (1, 1, 1), (1, 1, 1)),
    "onset one step beyond": (ref((1.0, 1.5, 60)), [(22, 30, 60)], (0, 1, 1), (0, 1, 1)),
    # a 0.1 s note: 0.2 * duration = 0.02 is below the 0.05 floor, so an offset 0.05 off still hits and one 0.10 off does not
    "offset floor hit": (ref((1.0, 1.1, 60)), [(20, 23, 60)], (1, 1, 1), (1, 1, 1)),
    "offset floor miss": (ref((1.0, 1.1, 60)), [(20, 24, 60)], (0, 1, 1), (1, 1, 1)),
    # a 1 s note: the tolerance is 0.2 * duration = 0.2
    "offset ratio hit": (ref((1.0, 2.0, 60)), [(20, 44, 60)], (1, 1, 1), (1, 1, 1)),
    "offset ratio miss": (ref((1.0, 2.0, 60)), [(20, 45, 60)], (0, 1, 1), (1, 1, 1)),
    "one semitone off": (ref((1.0, 1.5, 60)), [(20, 30, 61)], (0, 1, 1), (0, 1, 1)),
    "two identical decoded notes": (ref((1.0, 1.5, 60)), [(20, 30, 60), (20, 30, 60)], (1, 1, 2), (1, 1, 2)),
    "labels with end <= start": (ref((1.0, 1.5, 60), (2.0, 2.0, 60), (3.0, 2.5, 62)), [(20, 30, 60), (40, 50, 60), (50, 60, 62)],
                                 (1, 1, 3), (1, 1, 3)),
    "nothing decoded": (ref((1.0, 1.5, 60), (2.0, 2.5, 64)), [], (0, 2, 0), (0, 2, 0)),
    "no labels": (ref(), [(20, 30, 60)], (0, 0, 1), (0, 0, 1)),
    "nothing at all": (ref(), [], (0, 0, 0), (0, 0, 0)),
}


def random_case(rng, max_notes=15, pitches=(60, 61, 62), span=2.5):
    """(label notes off the grid, decoded index triples): the labels quantised, jittered by -2..+2 steps at both ends, some dropped,
    some inserted."""
    n = int(rng.integers(0, max_notes + 1))
    start = rng.uniform(0.0, span, n)
    dur = rng.uniform(0.03, 0.9, n)
    labels = np.stack([start, start + dur, rng.choice(pitches, n).astype(np.float64), np.full(n, 80.0)], axis=1).reshape(-1, 4)
    decoded = []
    for s, e, pitch, _ in labels:
        if rng.random() < 0.2:
            continue
        on = max(0, int(round(s / STEP)) + int(rng.integers(-2, 3)))
        off = max(on + 1, int(round(e / STEP)) + int(rng.integers(-2, 3)))
        decoded.append((on, off, int(pitch)))
    for _ in range(int(rng.integers(0, 4))):
        on = int(rng.integers(0, int(span / STEP)))
        decoded.append((on, on + int(rng.integers(1, 12)), int(rng.choice(pitches))))
    order = rng.permutation(len(decoded))
    return labels, [decoded[i] for i in order]


def tokenised(notes_per_row, width):
    """ids [R, width] int64 of ``MidiTokenizer.__call__`` on the index triples of every row, cut or PAD-filled to ``width``: the
    compact form (shared time tokens; an OFFSET closes every open note of its pitch, a cut row leaves notes open), so what a row
    decodes to is whatever ``tokenizer.decode`` says, not necessarily the triples."""
    ids = TOK([est_seconds(n) for n in notes_per_row]).numpy()
    out = np.full((len(notes_per_row), width), PAD, dtype=np.int64)
    w = min(width, ids.shape[1])
    out[:, :w] = ids[:, :w]
    return out
