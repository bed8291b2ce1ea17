"""Inputs the CPU and GPU tests of the consensus selection share: a seeded generator of one hidden label per clip and K candidates
made from it independently, as ``note_metrics_cases.random_case`` makes its decoded side - the label quantised to the 50 ms grid,
jittered by -2..+2 steps at both ends, every note dropped with probability 0.2, 0..3 notes inserted, the order shuffled."""
import numpy as np

import note_metrics_cases as nc

STEP = nc.STEP
PITCHES = (60, 61, 62, 64, 67)
SPAN = 2.5


def hidden_label(rng, min_notes=1, max_notes=15):
    """[n, 4] float64 label notes off the grid, 1..15 of them."""
    n = int(rng.integers(min_notes, max_notes + 1))
    start = rng.uniform(0.0, SPAN, n)
    dur = rng.uniform(0.03, 0.9, n)
    return np.stack([start, start + dur, rng.choice(PITCHES, n).astype(np.float64), np.full(n, 80.0)], axis=1).reshape(-1, 4)


def candidate(rng, label):
    """Index triples (onset, offset, pitch) of one noisy transcription of ``label``."""
    decoded = []
    for s, e, pitch, _ in label:
        if rng.random() < 0.2:
            continue
        on = max(0, int(round(s / STEP)) + int(rng.integers(-2, 3)))
        off = max(on + 1, int(round(e / STEP)) + int(rng.integers(-2, 3)))
        decoded.append((on, off, int(pitch)))
    for _ in range(int(rng.integers(0, 4))):
        on = int(rng.integers(0, int(SPAN / STEP)))
        decoded.append((on, on + int(rng.integers(1, 12)), int(rng.choice(PITCHES))))
    order = rng.permutation(len(decoded))
    return [decoded[i] for i in order]


def clip(rng, K):
    """(label [n, 4], K candidates as index triples)."""
    label = hidden_label(rng)
    return label, [candidate(rng, label) for _ in range(K)]


def clips(seed, B, K):
    """B clips of K candidates: (labels, candidates[b][k]) from one seeded generator."""
    rng = np.random.default_rng(seed)
    made = [clip(rng, K) for _ in range(B)]
    return [m[0] for m in made], [m[1] for m in made]
