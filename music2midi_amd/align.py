"""Note labels -> a recording's clock: integer chroma / onset features and DTW, defined in numpy and run on the device (csrc/align.hip).

Stands in for ref: data/align_audio_midi.py (render the MIDI cover, chroma and onset features of both signals, the key shift, DTW,
note times moved onto the recording's clock) and for the two values of ref: data/compute_metrics.py that need nothing but the
alignment.  This is the PROJECT'S OWN aligner, not synctoolbox's: one resolution (plus a 5 Hz shift search), no tuning estimation,
a simplified onset feature.  It has been validated on rendered, time-warped notes only (tests/align_cases.py); nobody has measured
its alignment quality on real recordings.  Dense random clusters (6 notes per second and up) saturate chroma and can fail.

    pitch_filterbank(fs, n_fft) -> float32 [n_fft/2+1, 88]           one triangle per MIDI pitch 21..108
    band_log_energies_host(y) -> float32 [frames, 88]                log(max(|STFT|^2 @ fb, 1e-6)): the ONLY floating-point stage
    features_host(L) -> (chroma, onset) uint8 [frames, 12]           THE DEFINITION of m2m_align_features
    coarse(chroma, W=21, D=10) -> int32 [ceil(frames/D), 12]         centred box sums at 5 Hz
    cost(u, v), cost_matrix(A, B) -> int32                           256 - isqrt(65536 (u.v)^2 // ((u.u)(v.v)))
    dtw_host(C) -> (total, path int32 [2, L])                        THE DEFINITION of m2m_align_dtw
    dtw_features_host(fa, fb, shift=0, coarse=False)                 dtw_host of the cost matrix of two feature sets
    optimal_shift_host(chroma_a, chroma_b) -> (s, totals[12])        opt_chroma_shift in the reference's sense
    strictly_monotonic(path), apply_warp(notes, wp), warp_metrics(wp, duration, notes)
    align_notes_host(audio, notes, sr=None) -> AlignResult           the whole path on the host
    align_features(L), dtw(fa, fb, shift=0, coarse=False)            the two kernels on given inputs
    align_notes(audio, notes, sr=None, device=None), align_batch(audios, notes_list, sr=None, device=None)

Analysis: fs 22050 ("to follow sync toolbox", the reference says), rate = dataset.dtw_feature_rate = 50, hop = 441, n_fft 2048, the
project's periodic Hann window, centred frames with reflected edges, frames = 1 + T // hop.

Features of a frame t from L [frames, 88] (finite), d = float32(ln 2.5, ln 5, ln 10, ln 20); every step is ONE fp32 subtraction and a
comparison.  M[t] = max_p L[t, p]; the frame is silent when M[t] <= -6.0f and all its features are 0.
  q[t, p] = #{k : L[t, p] >= M[t] - d[k]} (0..4);  chroma[t, c] = sum of q over the pitches of class c (at most 32).
  on[t, p] = t >= 2 and L[t, p] - L[t-2, p] >= float32(ln 4) and L[t, p] >= M[t] - d[3] and t not silent;
  first = on[t] and not on[t-1];  o[t, c] = sum of first over the pitches of class c;  onset[t, c] = max_{tau=0..3} (4 - tau) o[t - tau, c].

Cost.  S = 256; cost(u, v) = S - isqrt((S S (u.v)^2) // ((u.u)(v.v))) in 64-bit integers, S when either vector is zero.  The quotient
is at most 65536 (Cauchy-Schwarz).  The largest intermediate value is 65536 (12 672^2)^2 = 1.93e18 of the 9.22e18 an int64 holds
(coarse chroma is at most 21 * 32 = 672 per class).  A full-resolution cell costs cost(chroma) + cost(onset), a coarse one cost(chroma).

DTW.  D[-1, -1] = 0, every other border cell +inf; D[i, j] = min(D[i-1, j-1] + 4 C, D[i-1, j] + 3 C, D[i, j-1] + 3 C) (synctoolbox's step
weights 2, 1.5, 1.5, doubled); a tie takes the diagonal, then (i-1, j), then (i, j-1).  The path runs from (0, 0) to (N-1, M-1).
Sides of up to 32768 frames (10.9 min): the total is at most 65536 * 4 * 512 = 2^27.
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import melbank, render

FS = 22050
RATE = 50                                 # dataset.dtw_feature_rate
HOP = FS // RATE                          # 441
N_FFT = 2048
N_BANDS = 88                              # MIDI 21..108
LOW_PITCH = 21
S = 256
MAX_FRAMES = 32768                        # a side of one DTW problem on the device (M2M_ALIGN_MAX_FRAMES)
COARSE_W, COARSE_D = 21, 10
SILENT = np.float32(-6.0)
D_THRESH = np.array([np.log(2.5), np.log(5.0), np.log(10.0), np.log(20.0)], dtype=np.float64).astype(np.float32)
ONSET_RISE = np.float32(np.log(4.0))
PITCH_CLASS = (LOW_PITCH + np.arange(N_BANDS)) % 12
_INF = np.int64(1) << np.int64(40)


class AlignResult(NamedTuple):
    notes: np.ndarray                     # float64 [n, 4] on the recording's clock, transposed by semitones(opt_chroma_shift)
    warp_path: np.ndarray                 # float64 [2, K] seconds: [0] the recording's clock, [1] the notes'; strictly increasing
    opt_chroma_shift: int                 # 0..11
    total_cost: int                       # the full-resolution DTW total
    metrics: dict                         # wp_std, time_diff_ratio


def semitones(s: int) -> int:
    return int(s) if int(s) <= 6 else int(s) - 12


# ------------------------------------------------------------------ the floating-point stage
def pitch_filterbank(fs: float = FS, n_fft: int = N_FFT) -> np.ndarray:
    """float32 [n_fft/2+1, 88]: band p (MIDI 21 + column) is 1 at its own frequency and 0 at the two neighbouring semitones'."""
    f = np.arange(n_fft // 2 + 1, dtype=np.float64) * (float(fs) / n_fft)
    centre = render.pitch_hz(np.arange(LOW_PITCH - 1, LOW_PITCH + N_BANDS + 1))
    lo, mid, hi = centre[:-2], centre[1:-1], centre[2:]
    up = (f[:, None] - lo[None, :]) / (mid - lo)[None, :]
    down = (hi[None, :] - f[:, None]) / (hi - mid)[None, :]
    return np.maximum(0.0, np.minimum(up, down)).astype(np.float32)


def num_frames(n_samples: int) -> int:
    return 1 + int(n_samples) // HOP


def _check_audio(y: np.ndarray) -> np.ndarray:
    y = np.asarray(y, dtype=np.float32).reshape(-1)
    if len(y) < N_FFT // 2 + 1:
        raise ValueError(f"align: {len(y)} samples, the reflected first frame needs at least {N_FFT // 2 + 1}")
    return y


def band_log_energies_host(y, chunk: int = 2048) -> np.ndarray:
    """float32 [frames, 88] of a signal at 22050 Hz: the log-mel frontend's definition with ``pitch_filterbank``."""
    y = _check_audio(y)
    window, fb = melbank.hann_window(N_FFT), pitch_filterbank()
    padded = np.pad(y, N_FFT // 2, mode="reflect")
    frames = num_frames(len(y))
    out = np.empty((frames, N_BANDS), dtype=np.float32)
    for t0 in range(0, frames, chunk):
        t = np.arange(t0, min(t0 + chunk, frames))
        x = padded[t[:, None] * HOP + np.arange(N_FFT)[None, :]] * window[None, :]
        spec = np.fft.rfft(x, axis=1)
        power = (spec.real ** 2 + spec.imag ** 2).astype(np.float32)
        out[t] = np.log(np.maximum(power @ fb, np.float32(1e-6)))
    return out


# ------------------------------------------------------------------ the integer stages
def _class_sum(x: np.ndarray) -> np.ndarray:
    """[frames, 88] -> [frames, 12], summed over the pitches of each class."""
    out = np.zeros((x.shape[0], 12), dtype=np.int32)
    for c in range(12):
        out[:, c] = x[:, PITCH_CLASS == c].sum(axis=1)
    return out


def features_host(L) -> Tuple[np.ndarray, np.ndarray]:
    """THE DEFINITION (the module's docstring): (chroma, onset), both uint8 [frames, 12]."""
    L = np.asarray(L, dtype=np.float32).reshape(-1, N_BANDS)
    frames = L.shape[0]
    M = L.max(axis=1) if frames else np.zeros(0, np.float32)
    loud = ~(M <= SILENT)
    thr = M[:, None] - D_THRESH[None, :]                                       # fp32 [frames, 4]
    assert thr.dtype == np.float32
    q = (L[:, :, None] >= thr[:, None, :]).sum(axis=2).astype(np.int32) * loud[:, None]
    chroma = _class_sum(q)
    on = np.zeros((frames, N_BANDS), dtype=bool)
    if frames > 2:
        rise = L[2:] - L[:-2]
        assert rise.dtype == np.float32
        on[2:] = (rise >= ONSET_RISE) & (L[2:] >= thr[2:, 3:4]) & loud[2:, None]
    first = on.copy()
    first[1:] &= ~on[:-1]
    o = _class_sum(first.astype(np.int32))
    onset = np.zeros((frames, 12), dtype=np.int32)
    for tau in range(4):
        onset[tau:] = np.maximum(onset[tau:], (4 - tau) * o[:frames - tau])
    return chroma.astype(np.uint8), onset.astype(np.uint8)


def coarse_frames(frames: int, D: int = COARSE_D) -> int:
    return -(-int(frames) // D)


def coarse(chroma, W: int = COARSE_W, D: int = COARSE_D) -> np.ndarray:
    """int32 [ceil(frames / D), 12]: the sum of the W frames centred on every D-th frame, zeros outside the clip."""
    chroma = np.asarray(chroma).reshape(-1, 12).astype(np.int32)
    half = W // 2
    csum = np.concatenate([np.zeros((1, 12), np.int32), np.cumsum(np.pad(chroma, ((half, half), (0, 0))), axis=0, dtype=np.int32)])
    centre = np.arange(coarse_frames(len(chroma), D)) * D
    return (csum[centre + W] - csum[centre]).astype(np.int32)


def _isqrt(q: np.ndarray) -> np.ndarray:
    r = np.floor(np.sqrt(q.astype(np.float64))).astype(np.int64)
    r = np.where(r * r > q, r - 1, r)
    return np.where((r + 1) * (r + 1) <= q, r + 1, r)


def cost_matrix(A, B) -> np.ndarray:
    """int32 [N, M]: ``cost`` of every row of A [N, 12] against every row of B [M, 12].  Largest intermediate value:
    65536 * (12 * 672^2)^2 = 1.93e18 < 2^63 = 9.22e18."""
    A, B = np.asarray(A).reshape(-1, 12).astype(np.int64), np.asarray(B).reshape(-1, 12).astype(np.int64)
    dot = A @ B.T
    den = (A * A).sum(axis=1)[:, None] * (B * B).sum(axis=1)[None, :]
    q = (S * S * dot * dot) // np.where(den > 0, den, 1)
    return np.where(den > 0, S - _isqrt(q), S).astype(np.int32)


def cost(u, v) -> int:
    return int(cost_matrix(np.asarray(u).reshape(1, 12), np.asarray(v).reshape(1, 12))[0, 0])


def feature_cost_host(fa, fb, shift: int = 0, coarse: bool = False, rows: Optional[slice] = None) -> np.ndarray:
    """The cost matrix of two feature sets - coarse: int32 [n, 12] chroma; else (chroma, onset) uint8 pairs - with side b rolled by
    ``shift`` classes (``np.roll(b, shift, axis=1)``).  ``rows`` restricts side a."""
    rows = slice(None) if rows is None else rows
    if coarse:
        return cost_matrix(np.asarray(fa)[rows], np.roll(np.asarray(fb), shift, axis=1))
    return (cost_matrix(np.asarray(fa[0])[rows], np.roll(np.asarray(fb[0]), shift, axis=1)) +
            cost_matrix(np.asarray(fa[1])[rows], np.roll(np.asarray(fb[1]), shift, axis=1)))


def dtw_host(Cm) -> Tuple[int, np.ndarray]:
    """THE DEFINITION (the module's docstring): (total, path int32 [2, L]) of a cost matrix [N, M], anti-diagonal by anti-diagonal."""
    Cm = np.asarray(Cm)
    N, M = Cm.shape
    if N < 1 or M < 1:
        raise ValueError(f"dtw_host: a {N} x {M} cost matrix")
    direction = np.zeros((N, M), dtype=np.uint8)
    # position i + 1 of a diagonal's array holds row i; position 0 is row -1
    prev2 = np.full(N + 1, _INF, dtype=np.int64)
    prev2[0] = 0                                                               # D[-1, -1]
    prev1 = np.full(N + 1, _INF, dtype=np.int64)
    total = 0
    for k in range(N + M - 1):
        i = np.arange(max(0, k - M + 1), min(k, N - 1) + 1)
        c = Cm[i, k - i].astype(np.int64)
        best = prev2[i] + 4 * c                                                # D[i-1, j-1]
        up = prev1[i] + 3 * c                                                  # D[i-1, j]
        left = prev1[i + 1] + 3 * c                                            # D[i, j-1]
        d = np.zeros(len(i), dtype=np.uint8)
        take = up < best
        best, d = np.where(take, up, best), np.where(take, np.uint8(1), d)
        take = left < best
        best, d = np.where(take, left, best), np.where(take, np.uint8(2), d)
        direction[i, k - i] = d
        cur = np.full(N + 1, _INF, dtype=np.int64)
        cur[i + 1] = best
        prev2, prev1 = prev1, cur
        total = int(best[-1])
    i, j, path = N - 1, M - 1, []
    while True:
        path.append((i, j))
        if i == 0 and j == 0:
            break
        d = int(direction[i, j])
        i, j = (i - 1, j - 1) if d == 0 else ((i - 1, j) if d == 1 else (i, j - 1))
    return total, np.array(path[::-1], dtype=np.int32).T.reshape(2, -1)


def dtw_features_host(fa, fb, shift: int = 0, coarse: bool = False) -> Tuple[int, np.ndarray]:
    n, m = len(fa if coarse else fa[0]), len(fb if coarse else fb[0])
    Cm = np.empty((n, m), dtype=np.uint16)                                     # at most 512; in row blocks: the int64 temporaries are large
    for r0 in range(0, n, 512):
        Cm[r0:r0 + 512] = feature_cost_host(fa, fb, shift, coarse, slice(r0, r0 + 512))
    return dtw_host(Cm)


def optimal_shift_host(chroma_a, chroma_b) -> Tuple[int, List[int]]:
    """(s, the 12 totals): the s in 0..11 whose ``dtw(cost(coarse(a), roll(coarse(b), s, axis=1)))`` total is smallest, ties to the
    smallest s."""
    ca, cb = coarse(chroma_a), coarse(chroma_b)
    totals = [dtw_features_host(ca, cb, s, True)[0] for s in range(12)]
    return int(np.argmin(totals)), totals


def strictly_monotonic(path) -> np.ndarray:
    """The first point, then every point at which BOTH coordinates exceed the last kept point's."""
    path = np.asarray(path).reshape(2, -1)
    keep, li, lj = [0], int(path[0, 0]), int(path[1, 0])
    for k in range(1, path.shape[1]):
        if path[0, k] > li and path[1, k] > lj:
            keep.append(k)
            li, lj = int(path[0, k]), int(path[1, k])
    return path[:, keep]


def apply_warp(notes, wp) -> np.ndarray:
    """Notes [n, 4] from the clock of ``wp[1]`` to that of ``wp[0]`` (seconds, increasing): the notes whose start and end lie inside
    ``[wp[1][0], wp[1][-1]]`` are kept, both times interpolated in float64, negative times clamped to 0, and a note whose end is not
    after its start dropped."""
    notes = np.asarray(notes, dtype=np.float64).reshape(-1, 4)
    wp = np.asarray(wp, dtype=np.float64).reshape(2, -1)
    keep = (notes[:, 0] >= wp[1, 0]) & (notes[:, 1] <= wp[1, -1])
    out = notes[keep].copy()
    out[:, 0] = np.maximum(np.interp(out[:, 0], wp[1], wp[0]), 0.0)
    out[:, 1] = np.maximum(np.interp(out[:, 1], wp[1], wp[0]), 0.0)
    return out[out[:, 1] > out[:, 0]]


def warp_metrics(wp, duration: float, notes) -> dict:
    """``wp_std`` and ``time_diff_ratio`` of ref: data/compute_metrics.py, the two that need nothing but the alignment;
    ``config.dataset.filter_threshold`` bounds both.  ``notes`` are the notes as they came in."""
    wp = np.asarray(wp, dtype=np.float64).reshape(2, -1)
    notes = np.asarray(notes, dtype=np.float64).reshape(-1, 4)
    end = float(notes[:, 1].max()) if len(notes) else 0.0
    return {"wp_std": float(np.std(wp[0] - wp[1])), "time_diff_ratio": abs(float(duration) - end) / float(duration)}


def transpose(notes, s: int) -> np.ndarray:
    """Notes moved by ``semitones(s)``; those that leave 0..127 are dropped."""
    notes = np.asarray(notes, dtype=np.float64).reshape(-1, 4).copy()
    notes[:, 2] += semitones(s)
    return notes[(notes[:, 2] >= 0) & (notes[:, 2] <= 127)]


def notes_length(notes) -> int:
    """Samples of the notes' rendering: the last ``off + release``, at least one analysis window."""
    voice = render.default_voice(FS)
    return max(render._default_length([render.pack(notes, FS, None, voice)], voice), N_FFT)


def _finish(notes, n_audio: int, shift: int, total: int, path: np.ndarray) -> AlignResult:
    wp = strictly_monotonic(path).astype(np.float64) / RATE
    return AlignResult(apply_warp(transpose(notes, shift), wp), wp, int(shift), int(total), warp_metrics(wp, n_audio / FS, notes))


def _as_audio_host(audio, sr) -> np.ndarray:
    from . import audio as audio_mod
    y = np.asarray(audio.detach().cpu().numpy() if hasattr(audio, "detach") else audio, dtype=np.float32).reshape(-1)
    if sr is not None and float(sr) != FS:
        y = audio_mod.resample(y, sr, FS).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):                          # audio that is not finite stays what it is
        return render._normalize(_check_audio(y))


def align_notes_host(audio, notes, sr: Optional[float] = None) -> AlignResult:
    """The whole path in numpy: render the notes (``render_host``, peak-normalised, 22050 Hz), peak-normalise the audio, features of
    both, the shift search, the full-resolution DTW with the notes' features rolled by the shift, ``strictly_monotonic``, seconds,
    ``apply_warp`` on the transposed notes.  ``sr``: the audio's rate when it is not 22050."""
    notes = np.asarray(notes, dtype=np.float64).reshape(-1, 4)
    y = _as_audio_host(audio, sr)
    z = render.render_host(notes, FS, notes_length(notes), normalize=True)
    fa, fb = features_host(band_log_energies_host(y)), features_host(band_log_energies_host(z))
    shift, _ = optimal_shift_host(fa[0], fb[0])
    total, path = dtw_features_host(fa, fb, shift, False)
    return _finish(notes, len(y), shift, total, path)


# ------------------------------------------------------------------ the device
_FE_HOP = 2 * HOP                          # the frontend reads sample pairs and takes even hops only: see _band_log_energies_device
_FE_LEAD = 2 * _FE_HOP - N_FFT // 2        # 740: frontend frame 2 + j begins at sample 882 j + 740 of its row
_frontends: dict = {}


class _Frontend:
    """An ``m2m_frontend`` of hop 882 with the pitch filterbank, for one device, for as long as the process lives."""

    def __init__(self):
        from . import native
        window, fb = np.ascontiguousarray(melbank.hann_window(N_FFT)), np.ascontiguousarray(pitch_filterbank())
        desc = native.FrontendDesc(N_FFT, _FE_HOP, N_FFT // 2 + 1, N_BANDS, window.ctypes.data_as(C.c_void_p), fb.ctypes.data_as(C.c_void_p))
        self.handle = C.c_void_p()
        native.check(native.load().m2m_frontend_create(C.byref(desc), C.byref(self.handle)), "m2m_frontend_create")


def _frontend(dev) -> _Frontend:
    fe = _frontends.get(dev.index)
    if fe is None:
        fe = _frontends.setdefault(dev.index, _Frontend())
    return fe


def _band_log_energies_device(signals: Sequence, dev):
    """The log band energies of K CUDA fp32 signals by ONE ``m2m_logmel_f32`` launch: (L fp32 [sum frames, 88], frames per signal).
    The frontend kernel takes even hops only, and 441 is odd; so every signal is laid out twice, reflected edges included, once
    for its even frames and once, 441 samples on, for its odd ones, and transformed at hop 882.  A row begins with 740 (299) zeros
    so that frontend frame 2 + j is frame 2 j (2 j + 1) of the signal and frames 0 and 1, which reflect the row's own edge, are
    thrown away; a row is long enough that no frame that is kept reflects at its end."""
    import torch
    import torch.nn.functional as F
    from . import native
    frames = [num_frames(int(y.shape[0])) for y in signals]
    half = max(-(-f // 2) for f in frames)
    Tz = _FE_HOP * (half + 1) + N_FFT // 2 + _FE_HOP
    rows = torch.zeros((2 * len(signals), Tz), dtype=torch.float32, device=dev)
    for k, y in enumerate(signals):
        padded = F.pad(y.reshape(1, 1, -1), (N_FFT // 2, N_FFT // 2), mode="reflect").reshape(-1)
        for odd in (0, 1):
            lead = _FE_LEAD - odd * HOP
            n = min(int(padded.shape[0]), Tz - lead)
            rows[2 * k + odd, lead:lead + n] = padded[:n]
    fe_frames = 1 + Tz // _FE_HOP
    out = torch.empty((2 * len(signals), fe_frames, N_BANDS), dtype=torch.float32, device=dev)
    native.check(native.load().m2m_logmel_f32(_frontend(dev).handle, rows.data_ptr(), 2 * len(signals), Tz, out.data_ptr(), out.stride(0), 0,
                                              native.stream_handle(dev)), "m2m_logmel_f32")
    L = torch.empty((sum(frames), N_BANDS), dtype=torch.float32, device=dev)
    at = 0
    for k, f in enumerate(frames):
        L[at:at + f:2] = out[2 * k, 2:2 + -(-f // 2)]
        L[at + 1:at + f:2] = out[2 * k + 1, 2:2 + f // 2]
        at += f
    return L, frames


def _cuda(device):
    import torch
    from . import native
    native.require_gpu()
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise ValueError(f"align: the device path runs on a GPU, not on {dev}")
    return torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)


def _offsets(counts: Sequence[int]) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.int64))]).astype(np.int32)


def _features_device(L, frames: Sequence[int], dev):
    """``m2m_align_features`` on L fp32 [sum frames, 88] (CUDA, contiguous): (chroma, onset) uint8 [sum frames, 12], one launch."""
    import torch
    from . import native
    total = int(sum(frames))
    assert L.is_cuda and L.dtype == torch.float32 and L.is_contiguous() and tuple(L.shape) == (total, N_BANDS)
    offs = torch.from_numpy(_offsets(frames)).to(dev)
    chroma = torch.empty((total, 12), dtype=torch.uint8, device=dev)
    onset = torch.empty((total, 12), dtype=torch.uint8, device=dev)
    native.check(native.load().m2m_align_features(L.data_ptr(), offs.data_ptr(), len(frames), int(max(frames)), total, chroma.data_ptr(),
                                                  onset.data_ptr(), native.stream_handle(dev)), "m2m_align_features")
    return chroma, onset


def align_features(L, device=None):
    """``features_host`` on the device, bit for bit: L fp32 [frames, 88] (numpy or tensor), or a list of them (one launch for the
    batch) -> (chroma, onset) CUDA uint8 [frames, 12], or a list of such pairs."""
    import torch
    dev = _cuda(device)
    batch = list(L) if isinstance(L, (list, tuple)) else [L]
    parts = [torch.as_tensor(x, dtype=torch.float32).reshape(-1, N_BANDS) for x in batch]
    frames = [int(p.shape[0]) for p in parts]
    if min(frames) < 1:
        raise ValueError("align_features: a clip without frames")
    with torch.cuda.device(dev):
        chroma, onset = _features_device(torch.cat([p.to(dev) for p in parts]).contiguous(), frames, dev)
    offs = _offsets(frames)
    pairs = [(chroma[offs[k]:offs[k + 1]], onset[offs[k]:offs[k + 1]]) for k in range(len(frames))]
    return pairs if isinstance(L, (list, tuple)) else pairs[0]


def _coarse_device(chroma, frames: Sequence[int], dev):
    """``coarse`` of every clip of chroma uint8 [sum frames, 12] by one launch: (int32 [sum coarse frames, 12], coarse frames)."""
    import torch
    from . import native
    cf = [coarse_frames(f) for f in frames]
    offs = torch.from_numpy(np.concatenate([_offsets(frames), _offsets(cf)])).to(dev)
    out = torch.empty((int(sum(cf)), 12), dtype=torch.int32, device=dev)
    native.check(native.load().m2m_align_coarse(chroma.data_ptr(), offs.data_ptr(), offs.data_ptr() + 4 * (len(frames) + 1), len(frames),
                                                int(max(cf)), int(sum(frames)), int(sum(cf)), COARSE_W, COARSE_D, out.data_ptr(),
                                                native.stream_handle(dev)), "m2m_align_coarse")
    return out, cf


def strip_width() -> int:
    """Columns of a DTW strip: the workgroup's threads (``m2m_align_dtw_strip``)."""
    from . import native
    return int(native.load().m2m_align_dtw_strip())


def _dtw_device(a, b, problems: np.ndarray, coarse_flag: bool, dev):
    """``m2m_align_dtw`` over ``problems`` int32 [P, 6] (a_offset, n, b_offset, m, shift, path_offset); ``a`` / ``b`` are one int32
    [frames, 12] tensor each (coarse) or (chroma, onset) uint8 pairs.  Returns (totals, lengths, paths) as host arrays: one wait."""
    import torch
    from . import native
    lib = native.load()
    problems = np.ascontiguousarray(problems, dtype=np.int32).reshape(-1, 6)
    P = len(problems)
    rows, cols = np.ascontiguousarray(problems[:, 1]), np.ascontiguousarray(problems[:, 3])
    need = int(lib.m2m_align_dtw_workspace_bytes(rows.ctypes.data_as(C.c_void_p), cols.ctypes.data_as(C.c_void_p), P))
    if need < 0:
        native.check(need, "m2m_align_dtw_workspace_bytes")
    cap = int(problems[-1, 5] + problems[-1, 1] + problems[-1, 3] - 1)
    a0, a1 = (a, a) if coarse_flag else a
    b0, b1 = (b, b) if coarse_flag else b
    with torch.cuda.device(dev):
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        totals = torch.empty(P, dtype=torch.int32, device=dev)
        lengths = torch.empty(P, dtype=torch.int32, device=dev)
        paths = torch.empty((2, cap), dtype=torch.int32, device=dev)
        native.check(lib.m2m_align_dtw(a0.data_ptr(), a1.data_ptr(), int(a0.shape[0]), b0.data_ptr(), b1.data_ptr(), int(b0.shape[0]),
                                       1 if coarse_flag else 0, problems.ctypes.data_as(C.c_void_p), P, ws.data_ptr(), need, totals.data_ptr(),
                                       paths.data_ptr(), cap, lengths.data_ptr(), native.stream_handle(dev)), "m2m_align_dtw")
        out = totals.cpu().numpy(), lengths.cpu().numpy(), paths.cpu().numpy()      # waits: `problems` is read by then
    return out


def _problem_table(ns: Sequence[int], ms: Sequence[int], a_offs, b_offs, shifts) -> np.ndarray:
    tab = np.zeros((len(ns), 6), dtype=np.int64)
    tab[:, 0], tab[:, 1], tab[:, 2], tab[:, 3], tab[:, 4] = a_offs, ns, b_offs, ms, shifts
    room = tab[:, 1] + tab[:, 3] - 1
    tab[:, 5] = np.cumsum(room) - room
    if tab[-1, 5] + room[-1] >= 1 << 31:
        raise ValueError("align: the paths of one call exceed 2^31 points")
    return tab.astype(np.int32)


def _split_paths(tab: np.ndarray, totals, lengths, paths) -> List[Tuple[int, np.ndarray]]:
    return [(int(totals[p]), paths[:, tab[p, 5]:tab[p, 5] + lengths[p]].copy()) for p in range(len(tab))]


def dtw(features_a, features_b, shift=0, coarse: bool = False, device=None):
    """``dtw_features_host`` on the device, bit for bit: (total, path int32 [2, L]).  Features are int32 [n, 12] (``coarse=True``) or
    (chroma, onset) uint8 pairs, numpy or tensors.  Lists of features (and of shifts) are a batch: one launch, a list of results."""
    import torch
    dev = _cuda(device)
    is_batch = isinstance(features_a, list)
    fa, fb = (features_a, features_b) if is_batch else ([features_a], [features_b])
    shifts = list(shift) if isinstance(shift, (list, tuple)) else [int(shift)] * len(fa)
    dtype = torch.int32 if coarse else torch.uint8

    def side(fs):
        parts = [[torch.as_tensor(x).reshape(-1, 12) for x in ((f,) if coarse else tuple(f))] for f in fs]
        cat = [torch.cat([p[k].to(dev, dtype) for p in parts]).contiguous() for k in range(len(parts[0]))]
        return (cat[0] if coarse else tuple(cat)), [int(p[0].shape[0]) for p in parts]
    with torch.cuda.device(dev):
        a, ns = side(fa)
        b, ms = side(fb)
        if min(ns + ms) < 1 or max(ns + ms) > MAX_FRAMES:
            raise ValueError(f"dtw: sides of {min(ns + ms)}..{max(ns + ms)} frames, the device takes 1..{MAX_FRAMES}")
        tab = _problem_table(ns, ms, _offsets(ns)[:-1], _offsets(ms)[:-1], shifts)
        out = _split_paths(tab, *_dtw_device(a, b, tab, coarse, dev))
    return out if is_batch else out[0]


def align_batch(audios: Sequence, notes_list: Sequence, sr=None, device=None) -> List[AlignResult]:
    """``align_notes_host`` for a batch of (recording, notes) pairs with the work on the GPU, one launch per stage for the whole
    batch: resample (where ``sr`` differs from 22050; one rate or one per pair), render, band energies, features, the 12 B coarse
    problems of the shift search, the B full-resolution problems; the paths come to the host, which applies them to the notes.  The
    band energies differ from numpy's in their last bits, so a few quantised features - and with them the path - may differ from
    the definition's; every stage after them is exact.  A pair the device does not take - a side of more than 32768 frames, audio
    that is not finite, no notes - goes through the definition."""
    import torch
    from . import ingest
    dev = _cuda(device)
    B = len(audios)
    if len(notes_list) != B:
        raise ValueError(f"align_batch: {B} recordings and {len(notes_list)} note arrays")
    rates = list(sr) if isinstance(sr, (list, tuple)) else [sr] * B
    notes_list = [np.asarray(n, dtype=np.float64).reshape(-1, 4) for n in notes_list]
    results: List[Optional[AlignResult]] = [None] * B
    with torch.cuda.device(dev):
        ys, lengths, taken = [], [], []
        for k in range(B):
            y = torch.as_tensor(audios[k], dtype=torch.float32).reshape(-1).to(dev)
            if rates[k] is not None and float(rates[k]) != FS:
                y = ingest.resample_device(y.contiguous(), rates[k], FS)
            if int(y.shape[0]) < N_FFT // 2 + 1:
                raise ValueError(f"align: {int(y.shape[0])} samples, the reflected first frame needs at least {N_FFT // 2 + 1}")
            n_notes = notes_length(notes_list[k]) if len(notes_list[k]) and np.isfinite(notes_list[k]).all() else 0
            ok = (n_notes > 0 and num_frames(int(y.shape[0])) <= MAX_FRAMES and num_frames(n_notes) <= MAX_FRAMES and
                  bool(torch.isfinite(y).all()))
            if not ok:
                results[k] = align_notes_host(y.cpu().numpy(), notes_list[k])
                continue
            peak = y.abs().max()
            ys.append(torch.where(peak > 0, y / torch.where(peak > 0, peak, torch.ones_like(peak)), y))
            lengths.append(n_notes)
            taken.append(k)
        if not taken:
            return results
        K = len(taken)
        rendered = render.render([notes_list[k] for k in taken], FS, max(lengths), normalize=True, device=dev)
        signals = ys + [rendered[i, :lengths[i]] for i in range(K)]
        L, frames = _band_log_energies_device(signals, dev)
        chroma, onset = _features_device(L, frames, dev)
        coarse_all, cf = _coarse_device(chroma, frames, dev)
        f_off, c_off = _offsets(frames), _offsets(cf)
        # the shift search: 12 problems per pair, one launch
        idx = np.repeat(np.arange(K), 12)
        tab = _problem_table(np.asarray(cf)[idx], np.asarray(cf)[K + idx], c_off[idx], c_off[K + idx], np.tile(np.arange(12), K))
        totals, _, _ = _dtw_device(coarse_all, coarse_all, tab, True, dev)
        shifts = totals.reshape(K, 12).argmin(axis=1)                          # the first minimum: ties to the smallest s
        idx = np.arange(K)
        tab = _problem_table(np.asarray(frames)[idx], np.asarray(frames)[K + idx], f_off[idx], f_off[K + idx], shifts)
        full = _split_paths(tab, *_dtw_device((chroma, onset), (chroma, onset), tab, False, dev))
        for i, k in enumerate(taken):
            results[k] = _finish(notes_list[k], int(ys[i].shape[0]), int(shifts[i]), full[i][0], full[i][1])
    return results


def align_notes(audio, notes, sr: Optional[float] = None, device=None) -> AlignResult:
    """``align_batch`` of one pair."""
    return align_batch([audio], [notes], sr, device)[0]
