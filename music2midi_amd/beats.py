"""Beat tracking: tempo and beat times of a recording or of a note array, defined in numpy and run on the device (csrc/beats.hip).

This is the PROJECT'S OWN tracker in the family of Ellis (2007) - an onset envelope, a tempo from an autocorrelation, a dynamic
program - not librosa's and not madmom's: ONE period per clip, whole frames, no downbeats, no time signature.  It has been validated
on rendered, planted clips only (tests/beats_cases.py); **nobody has measured its accuracy on real recordings.**  **A tempo drift
beyond about 3 % makes the one global period slip (at 5 % it does), and tempi outside roughly 85 to 170 BPM fold to another metrical
level: on audio a 72 BPM clip came out as 143 BPM and a 150 BPM clip as 75.**

    tempo_prior(centre_bpm=120, octaves=0.5) -> int32 [101]          the tables: every transcendental number enters as data that
    penalty_table(tightness=100) -> int32 [101, 201]                 numpy builds and the kernel is passed
    onset_envelope_host(L) -> int32 [frames]                         THE DEFINITION of m2m_beat_envelope; L from align.band_log_energies_host
    note_envelope(notes, frames=None) -> int32 [frames]              the envelope of a note array (host, in both paths)
    novelty(e) -> int64 [frames]
    track_envelope_host(e, period=None) -> (P, score int64 [101], beat frames int32)      THE DEFINITION of m2m_beat_track
    track_host(audio, sr=None), track_notes_host(notes, frames=None) -> BeatResult        the whole path on the host
    onset_envelope(L), track_envelopes(envs, period=None, device=None)                     the two kernels on given inputs
    track(audio, sr=None, device=None), track_batch(audios, ...), track_notes(notes_list, ...)
    aligned_beats, beat_metrics, filter_metrics, passes_filter       the dataset filter of ref: data/compute_metrics.py, generate_split.py
    quantize(notes, beat_times, subdivisions=4)                      notes snapped to the beat grid

Analysis grid: ``align``'s - 22050 Hz, 50 frames per second, a clip has 1..32768 frames.  LAG_MIN = 15, LAG_MAX = 100 (200..30 BPM),
H = 12.  Only the log band energies are floating point; from the envelope on everything is an integer.

Envelope of audio.  M[t] = max_p L[t, p] and d[3] = float32(ln 20) as in ``align``.  e[0] = 0; e[t] = 0 for a silent frame
(M[t] <= -6.0f); otherwise the sum over the bands with L[t, p] >= M[t] - d[3] of min(255, trunc(max(L[t, p] - L[t-1, p], 0) * 16.0f)) -
one fp32 subtraction, one exact scaling by a power of two, one truncation per band (the minimum is taken in fp32, before the
truncation: the same number for every finite rise).  e <= 88 * 255 = 22440.
Envelope of notes.  Frame floor(onset * 50 + 0.5) in float64, onsets outside [0, frames) dropped, e = min(64 * count, 22440);
``frames`` defaults to 1 + floor(50 * last offset).
Novelty.  o[t] = max(0, 25 e[t] - sum_{|k| <= 12} e[t + k]), e zero outside the clip; o <= 24 * 22440 = 538560 < 2^20.
Tempo.  a[k] = (sum_{t >= k} o[t] o[t - k]) // (F - k) for k = 15..min(200, F - 1), int64 (the sum stays below 2^55), 0 for a lag
beyond F - 1; score[l] = (a[l] + a[2 l] // 2) * prior[l] for l = 15..100; P = the first maximum of score, ``default_period`` (25) when
that maximum is 0.  prior[l] = rint(4096 exp(-0.5 (log2(l / (3000 / centre_bpm)) / octaves)^2)), 0 below 15.
Penalty.  s = (sum of o) // max(1, #{o > 0}); pen[tau] = (table[P][tau] * s) >> 8, table[P][tau] = rint(256 tightness ln(tau / P)^2).
Dynamic program.  lo = (P + 1) // 2, hi = 2 P; C[t] = o[t], back[t] = -1 for t < lo; otherwise C[t] = o[t] + max over
tau = lo..min(hi, t) of (C[t - tau] - pen[tau]) in int64, ties to the smallest tau, back[t] = t - tau.  The last beat is the first
maximum of C over [max(0, F - P), F); the beats are the chain of ``back`` from there, ascending.  A clip whose novelty is all zero has
no beats.  A period can be forced per clip.
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import align

FS, RATE, N_BANDS, MAX_FRAMES = align.FS, align.RATE, align.N_BANDS, align.MAX_FRAMES
LAG_MIN, LAG_MAX, H = 15, 100, 12
LAG_TOP = 2 * LAG_MAX                       # the largest lag of the autocorrelation
ENV_MAX = N_BANDS * 255                     # 22440
NOTE_WEIGHT = 64
DEFAULT_PERIOD = 25                         # 120 BPM
MIN_SAMPLES = align.N_FFT // 2 + 1          # 1025: what the reflected first frame needs


class BeatResult(NamedTuple):
    beat_times: np.ndarray                  # float64 [n] seconds
    beat_frames: np.ndarray                 # int32 [n], frames of 20 ms
    period: int                             # frames per beat
    bpm: float                              # 3000 / period
    score: np.ndarray                       # int64 [101]: the tempo score of every period; 0 below 15


# ------------------------------------------------------------------ the tables
def tempo_prior(centre_bpm: float = 120.0, octaves: float = 0.5) -> np.ndarray:
    """int32 [101]: rint(4096 * exp(-0.5 * (log2(l / centre) / octaves)^2)) with centre = 3000 / centre_bpm frames; 0 below LAG_MIN."""
    lag = np.arange(LAG_MAX + 1, dtype=np.float64)
    prior = np.zeros(LAG_MAX + 1, dtype=np.int32)
    centre = 60.0 * RATE / float(centre_bpm)
    prior[LAG_MIN:] = np.rint(4096.0 * np.exp(-0.5 * (np.log2(lag[LAG_MIN:] / centre) / float(octaves)) ** 2)).astype(np.int32)
    return prior


def penalty_table(tightness: float = 100.0) -> np.ndarray:
    """int32 [101, 201]: rint(256 * tightness * ln(tau / P)^2) for P = 15..100 and tau = 1..200, 0 elsewhere.  At the default its
    largest entry is 542914 (P = 100, tau = 1); the tracker reads tau = lo..hi only, where it is at most 12300 (ln 2 squared)."""
    table = np.zeros((LAG_MAX + 1, LAG_TOP + 1), dtype=np.int32)
    P, tau = np.arange(LAG_MIN, LAG_MAX + 1, dtype=np.float64)[:, None], np.arange(1, LAG_TOP + 1, dtype=np.float64)[None, :]
    table[LAG_MIN:, 1:] = np.rint(256.0 * float(tightness) * np.log(tau / P) ** 2).astype(np.int32)
    return table


_tables: dict = {}


def _default_tables() -> Tuple[np.ndarray, np.ndarray]:
    if not _tables:
        _tables["prior"], _tables["penalty"] = tempo_prior(), penalty_table()
    return _tables["prior"], _tables["penalty"]


def _check_tables(prior, table) -> Tuple[np.ndarray, np.ndarray]:
    dp, dt = _default_tables()
    prior = dp if prior is None else np.ascontiguousarray(prior, dtype=np.int32)
    table = dt if table is None else np.ascontiguousarray(table, dtype=np.int32)
    if prior.shape != (LAG_MAX + 1,) or table.shape != (LAG_MAX + 1, LAG_TOP + 1) or prior.min() < 0 or table.min() < 0:
        raise ValueError("beats: the prior is int32 [101] and the penalty table int32 [101, 201], neither negative")
    return prior, table


def _check_period(period) -> int:
    p = 0 if period is None else int(period)
    if p != 0 and not LAG_MIN <= p <= LAG_MAX:
        raise ValueError(f"beats: a forced period of {p} frames, the tracker takes {LAG_MIN}..{LAG_MAX}")
    return p


# ------------------------------------------------------------------ the envelopes
def onset_envelope_host(L) -> np.ndarray:
    """THE DEFINITION (the module's docstring): int32 [frames] of L fp32 [frames, 88]."""
    L = np.asarray(L, dtype=np.float32).reshape(-1, N_BANDS)
    frames = L.shape[0]
    e = np.zeros(frames, dtype=np.int32)
    if frames < 2:
        return e
    M = L.max(axis=1)
    thr = M - align.D_THRESH[3]
    with np.errstate(over="ignore"):
        rise = L[1:] - L[:-1]
        assert rise.dtype == np.float32 and thr.dtype == np.float32
        step = np.minimum(np.maximum(rise, np.float32(0)) * np.float32(16.0), np.float32(255.0)).astype(np.int32)
    keep = (L[1:] >= thr[1:, None]) & ~(M[1:] <= align.SILENT)[:, None]
    e[1:] = (step * keep).sum(axis=1)
    return e


def note_envelope(notes, frames: Optional[int] = None) -> np.ndarray:
    """int32 [frames]: min(64 * (onsets in the frame), 22440)."""
    notes = np.asarray(notes, dtype=np.float64).reshape(-1, 4)
    if frames is None:
        frames = 1 + int(np.floor(RATE * float(notes[:, 1].max()))) if len(notes) else 1
    frames = int(frames)
    if frames < 1:
        raise ValueError(f"note_envelope: {frames} frames")
    at = np.floor(notes[:, 0] * RATE + 0.5)
    at = at[(at >= 0) & (at < frames)].astype(np.int64)
    return np.minimum(NOTE_WEIGHT * np.bincount(at, minlength=frames), ENV_MAX).astype(np.int32)


def _check_envelope(e, most: Optional[int] = None) -> np.ndarray:
    e = np.ascontiguousarray(e, dtype=np.int32).reshape(-1)
    if len(e) < 1 or (most is not None and len(e) > most):
        raise ValueError(f"beats: an envelope of {len(e)} frames, the device takes 1..{MAX_FRAMES} and the definition 1 or more")
    if e.min() < 0 or e.max() > ENV_MAX:
        raise ValueError(f"beats: envelope values outside 0..{ENV_MAX}")
    return e


def novelty(e) -> np.ndarray:
    e = np.asarray(e, dtype=np.int64).reshape(-1)
    csum = np.concatenate([[0], np.cumsum(np.pad(e, H))])
    local = csum[2 * H + 1:] - csum[:-(2 * H + 1)]
    return np.maximum(0, (2 * H + 1) * e - local)


# ------------------------------------------------------------------ the tracker
def tempo_score(o, prior=None) -> np.ndarray:
    """int64 [101]: (a[l] + a[2 l] // 2) * prior[l]."""
    prior, _ = _check_tables(prior, None)
    o = np.asarray(o, dtype=np.int64)
    F = len(o)
    a = np.zeros(LAG_TOP + 1, dtype=np.int64)
    for k in range(LAG_MIN, min(LAG_TOP, F - 1) + 1):
        a[k] = int(np.dot(o[k:], o[:F - k])) // (F - k)
    lag = np.arange(LAG_MIN, LAG_MAX + 1)
    score = np.zeros(LAG_MAX + 1, dtype=np.int64)
    score[LAG_MIN:] = (a[lag] + a[2 * lag] // 2) * prior[LAG_MIN:].astype(np.int64)
    return score


def track_envelope_host(e, period=None, prior=None, table=None, default_period: int = DEFAULT_PERIOD):
    """THE DEFINITION (the module's docstring): (P, score int64 [101], beat frames int32) of an envelope int32 [frames]."""
    e = _check_envelope(e)
    prior, table = _check_tables(prior, table)
    forced = _check_period(period)
    if not LAG_MIN <= int(default_period) <= LAG_MAX:
        raise ValueError(f"beats: default_period = {default_period} outside {LAG_MIN}..{LAG_MAX}")
    F = len(e)
    o = novelty(e)
    score = tempo_score(o, prior)
    if forced:
        P = forced
    else:
        P = LAG_MIN + int(np.argmax(score[LAG_MIN:]))
        if score[P] <= 0:
            P = int(default_period)
    if not o.any():
        return P, score, np.zeros(0, dtype=np.int32)
    s = int(o.sum()) // max(1, int(np.count_nonzero(o)))
    lo, hi = (P + 1) // 2, 2 * P
    tau = np.arange(lo, hi + 1)
    pen = (table[P, lo:hi + 1].astype(np.int64) * s) >> 8
    Cs = np.zeros(F, dtype=np.int64)
    back = np.full(F, -1, dtype=np.int64)
    Cs[:lo] = o[:lo]
    floor = np.iinfo(np.int64).min
    for t0 in range(lo, F, lo):                                                  # the frames of a block do not depend on one another
        t = np.arange(t0, min(t0 + lo, F))
        src = t[:, None] - tau[None, :]
        cand = np.where(src >= 0, Cs[np.maximum(src, 0)] - pen[None, :], floor)
        pick = np.argmax(cand, axis=1)                                           # the first maximum: the smallest tau
        Cs[t] = o[t] + cand[np.arange(len(t)), pick]
        back[t] = t - tau[pick]
    start = max(0, F - P)
    t = start + int(np.argmax(Cs[start:]))
    chain = []
    while t >= 0:
        chain.append(t)
        t = int(back[t])
    return P, score, np.array(chain[::-1], dtype=np.int32)


def _result(P: int, score, frames) -> BeatResult:
    frames = np.asarray(frames, dtype=np.int32)
    return BeatResult(frames.astype(np.float64) / RATE, frames, int(P), 60.0 * RATE / int(P), np.asarray(score, dtype=np.int64))


def track_host(audio, sr: Optional[float] = None, period=None) -> BeatResult:
    """The whole audio path in numpy: resample to 22050 Hz where ``sr`` differs, peak-normalise, ``band_log_energies_host``,
    ``onset_envelope_host``, ``track_envelope_host``.  The definition has no upper limit on the frames (its sums stay inside int64
    up to 2^23 of them)."""
    y = align._as_audio_host(audio, sr)
    with np.errstate(invalid="ignore", over="ignore"):
        L = align.band_log_energies_host(y)
    L = np.where(np.isfinite(L), L, np.float32(np.log(np.float32(1e-6)))).astype(np.float32)     # audio that is not finite: silent frames
    return _result(*track_envelope_host(onset_envelope_host(L), period))


def track_notes_host(notes, frames: Optional[int] = None, period=None) -> BeatResult:
    """The notes path in numpy: ``note_envelope``, ``track_envelope_host``."""
    return _result(*track_envelope_host(note_envelope(notes, frames), period))


# ------------------------------------------------------------------ the device
def onset_envelope(L, device=None):
    """``onset_envelope_host`` on the device, integer for integer: L fp32 [frames, 88] (numpy or tensor), or a list of them (one launch
    for the batch) -> CUDA int32 [frames], or a list of them."""
    import torch
    dev = align._cuda(device)
    batch = list(L) if isinstance(L, (list, tuple)) else [L]
    parts = [torch.as_tensor(x, dtype=torch.float32).reshape(-1, N_BANDS) for x in batch]
    frames = [int(p.shape[0]) for p in parts]
    if min(frames) < 1:
        raise ValueError("onset_envelope: a clip without frames")
    with torch.cuda.device(dev):
        env = _envelope_device(torch.cat([p.to(dev) for p in parts]).contiguous(), frames, dev)
    offs = align._offsets(frames)
    out = [env[offs[k]:offs[k + 1]] for k in range(len(frames))]
    return out if isinstance(L, (list, tuple)) else out[0]


def _envelope_device(L, frames: Sequence[int], dev):
    """``m2m_beat_envelope`` on L fp32 [sum frames, 88] (CUDA, contiguous): int32 [sum frames], one launch."""
    import torch
    from . import native
    total = int(sum(frames))
    assert L.is_cuda and L.dtype == torch.float32 and L.is_contiguous() and tuple(L.shape) == (total, N_BANDS)
    offs = torch.from_numpy(align._offsets(frames)).to(dev)
    env = torch.empty(total, dtype=torch.int32, device=dev)
    native.check(native.load().m2m_beat_envelope(L.data_ptr(), offs.data_ptr(), len(frames), int(max(frames)), total, env.data_ptr(),
                                                 native.stream_handle(dev)), "m2m_beat_envelope")
    return env


_device_tables: dict = {}


def _tables_device(prior, table, dev):
    import torch
    if prior is None and table is None:
        got = _device_tables.get(dev.index)
        if got is None:
            p, t = _default_tables()
            got = _device_tables.setdefault(dev.index, (torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev)))
        return got
    p, t = _check_tables(prior, table)
    return torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev)


def _track_device(env, frames: Sequence[int], periods: Sequence[int], dev, prior=None, table=None, default_period: int = DEFAULT_PERIOD):
    """``m2m_beat_track`` over the clips of env int32 [sum frames] (CUDA): (periods, scores, beat frames per clip) as host arrays - one
    launch, one wait."""
    import torch
    from . import native
    lib = native.load()
    n = len(frames)
    fr = np.ascontiguousarray(frames, dtype=np.int32)
    need = int(lib.m2m_beat_track_workspace_bytes(fr.ctypes.data_as(C.c_void_p), n))
    if need < 0:
        native.check(need, "m2m_beat_track_workspace_bytes")
    room = fr.astype(np.int64) // 8 + 2
    clips = np.zeros((n, 4), dtype=np.int32)
    clips[:, 0], clips[:, 1], clips[:, 2], clips[:, 3] = align._offsets(frames)[:-1], fr, periods, np.cumsum(room) - room
    cap = int(room.sum())
    prior_dev, table_dev = _tables_device(prior, table, dev)
    with torch.cuda.device(dev):
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        period_out = torch.empty(n, dtype=torch.int32, device=dev)
        score_out = torch.empty((n, LAG_MAX + 1), dtype=torch.int64, device=dev)
        beats_out = torch.empty(cap, dtype=torch.int32, device=dev)
        n_out = torch.empty(n, dtype=torch.int32, device=dev)
        native.check(lib.m2m_beat_track(env.data_ptr(), int(env.shape[0]), clips.ctypes.data_as(C.c_void_p), n, prior_dev.data_ptr(),
                                        table_dev.data_ptr(), int(default_period), ws.data_ptr(), need, period_out.data_ptr(),
                                        score_out.data_ptr(), beats_out.data_ptr(), cap, n_out.data_ptr(), native.stream_handle(dev)),
                     "m2m_beat_track")
        P, score, beats, counts = period_out.cpu().numpy(), score_out.cpu().numpy(), beats_out.cpu().numpy(), n_out.cpu().numpy()   # waits: `clips` is read by then
    return P, score, [beats[clips[k, 3]:clips[k, 3] + counts[k]].copy() for k in range(n)]


def track_envelopes(envs, period=None, device=None, prior=None, table=None, default_period: int = DEFAULT_PERIOD):
    """``track_envelope_host`` on the device, integer for integer: an envelope int32 [frames] (numpy or tensor) -> (P, score, beat
    frames), or a list of envelopes (and of periods; ``None`` or 0: estimate) -> a list of such triples by ONE launch."""
    import torch
    dev = align._cuda(device)
    is_batch = isinstance(envs, (list, tuple))
    batch = list(envs) if is_batch else [envs]
    periods = list(period) if isinstance(period, (list, tuple)) else [period] * len(batch)
    if len(periods) != len(batch):
        raise ValueError(f"track_envelopes: {len(batch)} envelopes and {len(periods)} periods")
    periods = [_check_period(p) for p in periods]
    if not LAG_MIN <= int(default_period) <= LAG_MAX:
        raise ValueError(f"beats: default_period = {default_period} outside {LAG_MIN}..{LAG_MAX}")
    parts = []
    for x in batch:
        if torch.is_tensor(x) and x.is_cuda:
            x = x.reshape(-1)
            if not 1 <= int(x.shape[0]) <= MAX_FRAMES:
                raise ValueError(f"beats: an envelope of {int(x.shape[0])} frames, the tracker takes 1..{MAX_FRAMES}")
            parts.append(x.to(dev, torch.int32))                                # a kernel's own output: its range is the kernel's
        else:
            parts.append(torch.from_numpy(_check_envelope(x.cpu().numpy() if torch.is_tensor(x) else x, MAX_FRAMES)).to(dev))
    frames = [int(p.shape[0]) for p in parts]
    with torch.cuda.device(dev):
        P, score, beats = _track_device(torch.cat(parts).contiguous(), frames, periods, dev, prior, table, default_period)
    out = [(int(P[k]), score[k].copy(), beats[k]) for k in range(len(frames))]
    return out if is_batch else out[0]


def track_batch(audios: Sequence, sr=None, device=None) -> List[BeatResult]:
    """``track_host`` for a batch of recordings with the work on the GPU, one launch per stage for the whole batch: resample (where
    ``sr`` differs from 22050; one rate or one per recording), peak-normalise, ``align``'s band energies, the envelope, the tracker.
    The band energies differ from numpy's in their last bits, so a few envelope values - and with them a beat - may differ from the
    definition's; every stage after them is exact.  A recording the device path does not take - audio that is not finite, fewer than
    1025 samples, more than 32768 frames - goes through the definition."""
    import torch
    from . import ingest
    dev = align._cuda(device)
    B = len(audios)
    rates = list(sr) if isinstance(sr, (list, tuple)) else [sr] * B
    results: List[Optional[BeatResult]] = [None] * B
    with torch.cuda.device(dev):
        ys, taken = [], []
        for k in range(B):
            y = torch.as_tensor(audios[k], dtype=torch.float32).reshape(-1).to(dev)
            if rates[k] is not None and float(rates[k]) != FS:
                y = ingest.resample_device(y.contiguous(), rates[k], FS)
            n = int(y.shape[0])
            if n < MIN_SAMPLES or align.num_frames(n) > MAX_FRAMES or not bool(torch.isfinite(y).all()):
                results[k] = track_host(y.cpu().numpy())
                continue
            peak = y.abs().max()
            ys.append(torch.where(peak > 0, y / torch.where(peak > 0, peak, torch.ones_like(peak)), y))
            taken.append(k)
        if taken:
            L, frames = align._band_log_energies_device(ys, dev)
            env = _envelope_device(L, frames, dev)
            P, score, beats = _track_device(env, frames, [0] * len(frames), dev)
            for i, k in enumerate(taken):
                results[k] = _result(P[i], score[i].copy(), beats[i])
    return results


def track(audio, sr: Optional[float] = None, device=None) -> BeatResult:
    """``track_batch`` of one recording."""
    return track_batch([audio], sr, device)[0]


def track_notes(notes_list, frames=None, device=None):
    """``track_notes_host`` for a list of note arrays (or one array [n, 4]: one result) by ONE launch of the tracker; the envelopes
    are made on the host.  ``frames``: one count, one per array, or ``None``.  Notes of more than 32768 frames go through the
    definition."""
    single = not isinstance(notes_list, (list, tuple))
    batch = [notes_list] if single else list(notes_list)
    counts = list(frames) if isinstance(frames, (list, tuple)) else [frames] * len(batch)
    envs = [note_envelope(n, f) for n, f in zip(batch, counts)]
    out: List[Optional[BeatResult]] = [_result(*track_envelope_host(e)) if len(e) > MAX_FRAMES else None for e in envs]
    taken = [k for k in range(len(envs)) if out[k] is None]
    if taken:
        for k, r in zip(taken, track_envelopes([envs[k] for k in taken], device=device)):
            out[k] = _result(*r)
    return out[0] if single else out


# ------------------------------------------------------------------ the dataset filter
def aligned_beats(cover_notes, warp_path, device=None) -> np.ndarray:
    """The cover's beats on the recording's clock: its beats on its own clock (``track_notes`` when a GPU is there, the definition
    otherwise), then ``np.interp(beats, wp[1], wp[0])`` - ref: data/align_audio_midi.py:300-301, with the tracker in the place of
    ``PrettyMIDI.get_beats``: our labels are note arrays without a tempo map."""
    import torch
    wp = np.asarray(warp_path, dtype=np.float64).reshape(2, -1)
    result = track_notes(cover_notes, device=device) if torch.cuda.is_available() else track_notes_host(cover_notes)
    return np.interp(result.beat_times, wp[1], wp[0])


def _rms(arr: np.ndarray) -> float:
    return np.sqrt(np.mean(arr ** 2))


def beat_metrics(beat_times, duration: float, notes) -> dict:
    """``max_beat_fluctuation`` and ``max_note_density`` of ref: data/compute_metrics.py:38-54, restated line for line in float64.
    It is a restatement with line references that was NEVER RUN AGAINST THE ORIGINAL: that file imports omegaconf and pretty_midi,
    which the image this project is built on does not have.

    The duration is appended to the beats (ref :38); a beat less than 0.1 s after its predecessor is dropped, the first compared with
    -1 (:40); the beats are ``array_split`` into 10 parts (:41-42); the fluctuation is the largest rms of the second difference over
    the parts longer than 2 (:43-45).  The notes are split with ``searchsorted`` at the first beat of every part longer than 1
    (:47-50), the durations are those parts' spans (:51), and the density is the largest ``len(piece) / duration`` over
    ``zip(pieces, durations)`` (:52-54).  The reference's zip pairs piece 0 - the notes BEFORE the first part's first beat - with the
    first part's duration, piece 1 with the second part's, and never reaches the last piece; that is kept as it is.  When no part is
    long enough ``np.max`` of an empty list raises ``ValueError`` there, and so does this."""
    beat_times = np.append(np.asarray(beat_times, dtype=np.float64).reshape(-1), float(duration))
    notes = np.asarray(notes, dtype=np.float64).reshape(-1, 4)
    beat_times = beat_times[np.diff(beat_times, prepend=-1) > 0.1]
    beat_times_split = np.array_split(beat_times, 10)
    fluctuation = [_rms(np.diff(np.diff(x))) for x in beat_times_split if len(x) > 2]
    if not fluctuation:
        raise ValueError("beat_metrics: no tenth of the beats holds more than two of them")
    max_beat_fluctuation = np.max(fluctuation)
    notes_split_indices = np.searchsorted(notes[:, 0], [x[0] for x in beat_times_split if len(x) > 1])
    notes_split = np.array_split(notes, notes_split_indices)
    duration_split = [x[-1] - x[0] for x in beat_times_split if len(x) > 1]
    max_note_density = np.max([len(piece) / dur for (piece, dur) in zip(notes_split, duration_split)])
    return {"max_beat_fluctuation": float(max_beat_fluctuation), "max_note_density": float(max_note_density)}


def filter_metrics(align_result, cover_notes, duration: float, device=None) -> dict:
    """The four values ``config.dataset.filter_threshold`` bounds: ``align_result.metrics`` (wp_std, time_diff_ratio) and
    ``beat_metrics`` of the cover's aligned beats, the recording's duration and the aligned notes.  ``beat_metrics`` may raise
    ``ValueError`` (too few beats); ``passes_filter`` of such a pair is False - see ``filter_pair``."""
    beats = aligned_beats(cover_notes, align_result.warp_path, device)
    return dict(align_result.metrics, **beat_metrics(beats, duration, align_result.notes))


def passes_filter(metrics, config=None) -> bool:
    """The four strict ``<`` comparisons of ref: data/generate_split.py:29-34 against ``config.dataset.filter_threshold``.
    ``metrics``: the dict of ``filter_metrics``; ``None`` (a ``ValueError`` of ``beat_metrics``) or a missing or NaN value fails.
    The reference also asks for ``opt_chroma_shift == 0``: that belongs to the caller."""
    from .config import default_config
    threshold = (default_config() if config is None else config).dataset.filter_threshold
    if metrics is None:
        return False
    return all(name in metrics and bool(float(metrics[name]) < float(threshold[name]))
               for name in ("wp_std", "max_beat_fluctuation", "max_note_density", "time_diff_ratio"))


def filter_pair(align_result, cover_notes, duration: float, config=None, device=None) -> Tuple[Optional[dict], bool]:
    """(metrics or None, passes): ``filter_metrics`` then ``passes_filter``; a ``ValueError`` from ``beat_metrics`` fails the filter."""
    try:
        metrics = filter_metrics(align_result, cover_notes, duration, device)
    except ValueError:
        return None, False
    return metrics, passes_filter(metrics, config)


# ------------------------------------------------------------------ the beat grid
def grid_positions(times, beat_times) -> np.ndarray:
    """Seconds -> beats (float64): beat k lies at position k, linear between beats, the first and the last interval continued
    outside them."""
    beat_times = _check_beat_times(beat_times)
    times = np.asarray(times, dtype=np.float64)
    k = np.clip(np.searchsorted(beat_times, times, side="right") - 1, 0, len(beat_times) - 2)
    return k + (times - beat_times[k]) / (beat_times[k + 1] - beat_times[k])


def grid_times(positions, beat_times) -> np.ndarray:
    """The inverse of ``grid_positions``."""
    beat_times = _check_beat_times(beat_times)
    positions = np.asarray(positions, dtype=np.float64)
    k = np.clip(np.floor(positions).astype(np.int64), 0, len(beat_times) - 2)
    return beat_times[k] + (positions - k) * (beat_times[k + 1] - beat_times[k])


def _check_beat_times(beat_times) -> np.ndarray:
    beat_times = np.asarray(beat_times, dtype=np.float64).reshape(-1)
    if len(beat_times) < 2 or not (np.diff(beat_times) > 0).all() or not np.isfinite(beat_times).all():
        raise ValueError("beats: a grid needs two or more finite, strictly increasing beat times")
    return beat_times


def quantize(notes, beat_times, subdivisions: int = 4) -> np.ndarray:
    """Notes [n, 4] with onsets and offsets moved to the nearest grid point - ``subdivisions`` per beat, linear between beats (halves
    round up) - and every offset at least one grid step after its onset.  A grid point before time 0 is moved up to the first that
    is not.  float64, host only."""
    if int(subdivisions) < 1:
        raise ValueError(f"quantize: {subdivisions} subdivisions")
    n = int(subdivisions)
    notes = np.asarray(notes, dtype=np.float64).reshape(-1, 4).copy()
    first = np.ceil(grid_positions(0.0, beat_times) * n - 1e-9)                 # the first grid point at or after time 0
    on = np.maximum(np.floor(grid_positions(notes[:, 0], beat_times) * n + 0.5), first)
    off = np.maximum(np.floor(grid_positions(notes[:, 1], beat_times) * n + 0.5), on + 1)
    notes[:, 0], notes[:, 1] = grid_times(on / n, beat_times), grid_times(off / n, beat_times)
    return notes
