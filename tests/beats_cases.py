"""Seeded clips with planted beats, shared by test_beats_cpu.py and test_beats_gpu.py.

A case: beats at ``bpm`` whose period drifts sinusoidally by up to ``drift`` (one cycle of the sine per clip, a seeded phase), the
first beat 0.1 to 0.5 s into the clip.  Notes sit on 90 % of the beats and on 30 % of the off-beat eighths, each onset moved by 10 ms
of Gaussian jitter and carrying 1 to 3 notes of pitches 48..84 that last 0.8 beats.  The recording is their rendering
(``render.render_host``, 22050 Hz, peak-normalised); the notes themselves are what the notes path tracks.

Conditions, not measurements: the F-measure of the tracked beats against the planted ones at a window of 70 ms (mir_eval's window; a
one-to-one matching, no trimming of the first seconds) is at least 0.90, and |P - 3000 / bpm| <= max(1 frame, 5 %).

Next to each case stands what the definition alone (``track_host`` / ``track_notes_host``, numpy) gave when the case was chosen, under
the constants of music2midi_amd/beats.py as they are: F on the audio path, F on the notes path, the period of both.  Cases were
admitted at F >= 0.95 on both paths.
"""
import functools

import numpy as np

from music2midi_amd import align, render

F_CAP = 0.90
WINDOW = 0.070

# (seed, bpm, drift, seconds)                                  F audio, F notes, P audio / notes of the definition
CASES = (
    (14, 96.0, 0.00, 12.0),                                    # 1.000  1.000  31 / 31
    (12, 120.0, 0.02, 20.0),                                   # 0.975  0.975  25 / 25
    (3, 108.0, 0.03, 30.0),                                    # 1.000  1.000  28 / 28
    (4, 100.0, 0.01, 16.0),                                    # 0.981  0.981  30 / 30
    (13, 112.0, 0.02, 24.0),                                   # 0.978  0.989  27 / 27
    (6, 104.0, 0.03, 14.0),                                    # 0.980  1.000  28 / 29
)
# Seeds that were tried and fall below the bar on the audio path, where the chain locks onto the off-beats: (2, 120.0, 0.02, 20.0)
# 0.456 and (5, 112.0, 0.02, 24.0) 0.831; (1, 96.0, 0.0, 12.0) gave 0.895 on the notes path.
# The documented limit, nothing is asserted about it: 72 BPM lies below the range the half-octave prior keeps at its own metrical
# level.  The definition gave P = 42 (71 BPM, F 1.000) on THIS seed's audio - one success that proves nothing about the tempo - and
# P = 21 (143 BPM, F 0.667) on its notes.
LIMIT_CASE = (7, 72.0, 0.0, 20.0)


@functools.lru_cache(maxsize=None)
def case(seed: int, bpm: float, drift: float, seconds: float):
    """dict(audio fp32 at 22050 Hz, notes [n, 4], beats float64 [k], bpm, frames)."""
    rng = np.random.default_rng(seed)
    phase = rng.uniform(0, 2 * np.pi)
    t, beats = rng.uniform(0.1, 0.5), []
    while t < seconds - 0.3:
        beats.append(t)
        t += 60.0 / bpm * (1.0 + drift * np.sin(2 * np.pi * t / seconds + phase))
    beats = np.array(beats)
    rows = []
    for k, b in enumerate(beats):
        step = (beats[k + 1] - b) if k + 1 < len(beats) else (b - beats[k - 1])
        for at, chance in ((b, 0.9), (b + step / 2, 0.3)):
            if rng.random() >= chance:
                continue
            onset = max(0.0, at + rng.normal(0.0, 0.010))
            for pitch in rng.choice(np.arange(48, 85), rng.integers(1, 4), replace=False):
                rows.append([onset, min(onset + 0.8 * step, seconds - 0.05), float(pitch), 80.0])
    notes = np.array(rows, dtype=np.float64)
    notes = notes[np.argsort(notes[:, 0], kind="stable")]
    notes = notes[notes[:, 1] > notes[:, 0]]
    audio = render.render_host(notes, align.FS, int(seconds * align.FS), normalize=True)
    return dict(audio=audio, notes=notes, beats=beats, bpm=bpm, frames=align.num_frames(len(audio)))


def f_measure(found, truth, window: float = WINDOW) -> float:
    """2 hits / (found + truth): a found beat and a planted one within ``window`` of each other match, each at most once (both lists
    ascend, so the greedy walk finds a largest matching)."""
    found, truth = np.asarray(found, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    if len(found) == 0 or len(truth) == 0:
        return 0.0
    i = j = hits = 0
    while i < len(found) and j < len(truth):
        if abs(found[i] - truth[j]) <= window:
            hits, i, j = hits + 1, i + 1, j + 1
        elif found[i] < truth[j]:
            i += 1
        else:
            j += 1
    return 2.0 * hits / (len(found) + len(truth))


def period_ok(period: int, bpm: float) -> bool:
    want = 3000.0 / bpm
    return abs(period - want) <= max(1.0, 0.05 * want)
