"""Inputs the CPU and GPU tests of the frame-level metrics share: crafted cases with their six counts and their three note lists
written out by hand, and generators of random cases.  Decoded times lie on the tokenizer's 50 ms grid (index * 0.05 s = 5 frames per
step), label times are plain float64; the id rows come from ``note_metrics_cases``."""
import numpy as np

from note_metrics_cases import STEP, TOK, est_seconds, id_rows, random_case, ref, tokenised  # noqa: F401

# name -> (label notes, decoded notes as index triples,
#          (tp, fn, fp of the full roll, tp, fn, fp of the melody roll),
#          (TP, FN, FP notes of the full roll as (start, end, pitch) lists, in the order of roll_to_notes))
# n_frames is ceil(latest end / 0.01) and the last frame is silent: a note that reaches the latest end loses its last frame.
CRAFTED = {
    # frames 100..199, the last one cut
    "one note against itself": (ref((1.0, 2.0, 60)), [(20, 40, 60)], (99, 0, 0, 99, 0, 0), ([(1.0, 1.99, 60)], [], [])),
    # labels 0..49, decoded 100..149 less the cut one
    "disjoint notes": (ref((0.0, 0.5, 60)), [(20, 30, 64)], (0, 50, 49, 0, 50, 49), ([], [(0.0, 0.5, 60)], [(1.0, 1.49, 64)])),
    # labels 100..199, decoded 150..249 less the cut one
    "half overlap": (ref((1.0, 2.0, 60)), [(30, 50, 60)], (50, 50, 49, 50, 50, 49),
                     ([(1.5, 2.0, 60)], [(1.0, 1.5, 60)], [(2.0, 2.49, 60)])),
    # two label notes of one pitch that touch are one run of 100 frames
    "label notes that touch": (ref((1.0, 1.5, 60), (1.5, 2.0, 60)), [(50, 60, 72)], (0, 100, 49, 0, 100, 49),
                               ([], [(1.0, 2.0, 60)], [(2.5, 2.99, 72)])),
    # two that overlap are a union of 150 frames, not 200 cells
    "label notes that overlap": (ref((1.0, 2.0, 60), (1.5, 2.5, 60)), [(20, 60, 60)], (150, 0, 49, 150, 0, 49),
                                 ([(1.0, 2.5, 60)], [], [(2.5, 2.99, 60)])),
    # the note reaches the last frame and loses it; the output side is empty
    "cut at the last frame, nothing decoded": (ref((0.0, 1.0, 60)), [], (0, 99, 0, 0, 99, 0), ([], [(0.0, 0.99, 60)], [])),
    # int(1.001 * 100) == int(1.009 * 100) == 100: the note sounds in no frame, but its end makes n_frames 101
    "a note of zero frames": (ref((1.001, 1.009, 60), (0.0, 0.5, 62)), [(0, 10, 62)], (50, 0, 0, 50, 0, 0), ([(0.0, 0.5, 62)], [], [])),
    "nothing at all": (ref(), [], (0, 0, 0, 0, 0, 0), ([], [], [])),
    "no labels": (ref(), [(20, 30, 60)], (0, 0, 49, 0, 0, 49), ([], [], [(1.0, 1.49, 60)])),
    # both ends of the pitch range; the melody is pitch 127, class 7; equal end frames come out in pitch order
    "pitches 0 and 127": (ref((0.0, 1.0, 0), (0.0, 1.0, 127)), [(0, 20, 0), (0, 30, 127)], (200, 0, 49, 100, 0, 49),
                          ([(0.0, 1.0, 0), (0.0, 1.0, 127)], [], [(1.0, 1.49, 127)])),
    # an octave off: wrong twice on the full roll, right on the melody roll
    "octave error": (ref((1.0, 2.0, 60)), [(20, 40, 72)], (0, 99, 99, 99, 0, 0), ([], [(1.0, 1.99, 60)], [(1.0, 1.99, 72)])),
    # the label melody is class 0, class 7 in frames 50..99, class 0 again; the decoded melody is class 0 throughout
    "melody top changes mid-note": (ref((0.0, 2.0, 60), (0.5, 1.0, 67)), [(0, 40, 60)], (199, 50, 0, 149, 50, 50),
                                    ([(0.0, 1.99, 60)], [(0.5, 1.0, 67)], [])),
    # roll_to_notes' order: the run that ends first, then equal end frames by pitch
    "equal end frames": (ref((0.0, 1.0, 64), (0.5, 1.0, 60), (0.2, 0.6, 72)), [], (0, 188, 0, 0, 99, 0),
                         ([], [(0.2, 0.6, 72), (0.5, 0.99, 60), (0.0, 0.99, 64)], [])),
}

# the melody-roll notes (start, end, pitch class) of two of the cases above
CRAFTED_MELODY = {
    "melody top changes mid-note": ([(0.0, 0.5, 0), (1.0, 1.99, 0)], [(0.5, 1.0, 7)], [(0.5, 1.0, 0)]),
    "octave error": ([(1.0, 1.99, 0)], [], []),
    "equal end frames": ([], [(0.0, 0.2, 4), (0.2, 0.6, 0), (0.6, 0.99, 4)], []),
}


def note_list(triples):
    """[n, 4] float64 (start, end, pitch, velocity 1) of (start, end, pitch) triples: the shape of ``roll_to_notes``."""
    return np.asarray([[s, e, p, 1.0] for s, e, p in triples], dtype=np.float64).reshape(-1, 4)


def random_pair(rng, max_notes=12, span=2.5):
    """(label notes off the grid, decoded index triples) over two octaves with octave errors mixed in, so that the melody roll
    differs from the full roll."""
    labels, decoded = random_case(rng, max_notes=max_notes, pitches=(48, 55, 60, 61, 62, 67, 72), span=span)
    decoded = [(on, off, p + 12 if rng.random() < 0.15 else p) for on, off, p in decoded]
    return labels, decoded


def labels_ending_at(rng, n_frames, n_notes=6):
    """Label notes whose latest end gives exactly ``n_frames`` frames (n_frames >= 1): the last note ends at n_frames / 100 s and
    starts a few frames before the end."""
    end = n_frames / 100
    assert len(np.arange(0, end, 1 / 100)) == n_frames
    starts = rng.uniform(0.0, max(end - 0.005, 0.0), n_notes)
    ends = np.minimum(starts + rng.uniform(0.02, 3.0, n_notes), end)
    pitches = rng.choice((48, 60, 64, 72), n_notes).astype(np.float64)
    notes = np.stack([starts, ends, pitches, np.full(n_notes, 80.0)], axis=1)
    return np.concatenate([notes, [[max(0.0, end - 0.035), end, 64.0, 80.0]]])
