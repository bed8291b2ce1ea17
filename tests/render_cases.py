"""Inputs shared by test_render_cpu.py and test_render_gpu.py: the random polyphonic clip, and the direct call of the C entry."""
import ctypes as C

import numpy as np

from music2midi_amd import native, render

POLY_FS, POLY_SAMPLES = 48000, 144000


def random_notes(seed: int, n: int, seconds: float) -> np.ndarray:
    """``n`` notes over ``seconds``: uniform onsets, 0.05..1 s long, pitches 21..108, velocities 1..127, in draw order (unsorted)."""
    rng = np.random.default_rng(seed)
    onset = rng.uniform(0.0, seconds, n)
    return np.stack([onset, onset + rng.uniform(0.05, 1.0, n), rng.integers(21, 109, n).astype(np.float64),
                     rng.integers(1, 128, n).astype(np.float64)], axis=1)


def poly_batch() -> list:
    """B = 3: 300 random notes over 3 s (51 sounding at once on average between 0.5 and 2.5 s), an empty clip, 120 other notes."""
    return [random_notes(11, 300, 3.0), np.zeros((0, 4)), random_notes(12, 120, 3.0)]


def voice_struct(voice: render.Voice, wave_ptr, decay_ptr, **change) -> native.RenderVoice:
    fields = dict(wave_dev=wave_ptr, decay_dev=decay_ptr, table_size=voice.table_size, n_tables=voice.harmonics,
                  decay_steps=voice.decay_steps, attack=voice.attack, release=voice.release, reserved=0)
    fields.update(change)
    return native.RenderVoice(**fields)


def records(packed_batch, voice: render.Voice, n_samples: int) -> np.ndarray:
    """The packed notes of a batch as the kernel's six-word records, int32 [n, 6], written through the ctypes struct."""
    rows = [(on, min(off, n_samples), int(voice.inc[p]), int(voice.dec[p]), int(voice.table[p]) - 1, float(g))
            for pk in packed_batch for on, off, p, g in zip(pk.on.tolist(), pk.off.tolist(), pk.pitch.tolist(), pk.gain)]
    arr = (native.RenderNote * max(1, len(rows)))(*rows)
    return np.frombuffer(arr, dtype=np.int32).reshape(-1, 6)[:len(rows)].copy()
