"""Audio ingest on the device: WAVE sample bytes -> mono fp32 -> the model's sample rate, zero-padded to whole segments.

``audio.load_audio`` (without librosa) reads the file, averages the channels and resamples with scipy's polyphase filter on the
host; for a four-minute 44.1 kHz recording that is longer than the transcription that follows.  Those host functions stay the
definition; here the same steps run as two HIP kernels (csrc/ingest.hip) on the current stream and give the same samples, exactly:

    load_audio_device(path, sr, device=None, offset=0.0, duration=None, pad_to=None)  -> cuda fp32 [n]   (== audio.load_audio(path, sr))
    resample_device(y, orig_sr, target_sr)                                            -> cuda fp32 [n]   (== audio.resample(y, ...))
    decode_pcm_device(body, n_frames, channels, kind)                                 -> cuda fp32 [n]   (== read_wav(...)[0].mean(axis=1))
    eligible(path, sr=None)                                                           -> bool

The RIFF header is parsed on the host (``audio.wav_layout``, shared with ``read_wav``) and only the body of the ``data`` chunk -
with ``offset`` / ``duration``, only that slice of it - is uploaded.  The resampling filter is designed here as the installed scipy
designs it inside ``resample_poly`` and cached per ratio and device; the kernel designs none.  This is the scipy definition, not
librosa's soxr: with librosa installed, ``audio.load_audio`` and this module differ.  Equality holds for finite samples (scipy's
zero-padded filter turns an infinity next to the filter's support into NaN; the kernel does not visit those taps).

There is no fallback in this module: a missing library or a refused call raises ``native.NativeError``, a file the device path
cannot take raises ``ValueError`` (callers that want the host path instead ask ``eligible`` first, as ``Music2MIDI`` does).
"""
from __future__ import annotations

import mmap
import threading
from fractions import Fraction
from math import gcd
from typing import Optional, Tuple

import numpy as np
import torch

from . import native
from .audio import wav_layout, wav_sample_format

MAX_FRAMES = 1 << 28                     # M2M_INGEST_MAX_FRAMES
MAX_CHANNELS = 7                         # M2M_INGEST_MAX_CHANNELS: from 8 up numpy's mean sums pairwise
MAX_RATIO = 1000                         # M2M_INGEST_MAX_RATIO
MAX_OUT = 1 << 30                        # M2M_INGEST_MAX_OUT
FORMATS = {"u8": (0, 1), "s16": (1, 2), "s24": (2, 3), "s32": (3, 4), "f32": (4, 4), "f64": (5, 8)}   # kind -> (M2M_PCM_*, bytes)

_filters: dict = {}
_filters_lock = threading.Lock()


def resampled_length(n_in: int, up: int, down: int) -> int:
    """``len(resample_poly(x, up, down))`` for ``len(x) == n_in`` (host arithmetic of the library, no GPU)."""
    n = int(native.load().m2m_ingest_resampled_length(int(n_in), int(up), int(down)))
    if n < 0:
        raise ValueError(f"resampled_length: n_in = {n_in}, up / down = {up} / {down} out of range")
    return n


def ratio(orig_sr: float, target_sr: float) -> Tuple[int, int]:
    """(up, down) as ``audio.resample`` picks them; ``ValueError`` when the device path does not take them (outside 1..1000)."""
    frac = Fraction(float(target_sr) / float(orig_sr)).limit_denominator(1000)
    up, down = frac.numerator, frac.denominator
    g = gcd(up, down)
    if g:
        up, down = up // g, down // g
    if not (1 <= up <= MAX_RATIO and 1 <= down <= MAX_RATIO):
        raise ValueError(f"resampling {orig_sr} -> {target_sr} Hz needs up / down = {up} / {down}, outside 1..{MAX_RATIO}")
    return up, down


def design_filter(up: int, down: int) -> np.ndarray:
    """The fp32 filter ``resample_poly(x, up, down)`` builds for fp32 ``x``, in its order of operations: ``firwin`` in float64,
    cast to fp32, times ``up`` in fp32.  [2 half + 1], half = 10 max(up, down)."""
    from scipy.signal import firwin
    max_rate = max(up, down)
    half_len = 10 * max_rate
    h = firwin(2 * half_len + 1, 1. / max_rate, window=("kaiser", 5.0)).astype(np.float32)
    h *= up
    return h


def phase_major(h: np.ndarray, up: int) -> np.ndarray:
    """[up, J]: row p holds h[p], h[p + up], ... reversed (the order of ascending input index), zero where the filter has ended."""
    taps = (len(h) - 1) // up + 1
    padded = np.zeros(taps * up, dtype=np.float32)
    padded[:len(h)] = h
    return np.ascontiguousarray(padded.reshape(taps, up).T[:, ::-1])


def _filter_on(device: torch.device, up: int, down: int) -> torch.Tensor:
    key = (up, down, device.index)
    with _filters_lock:
        hp = _filters.get(key)
    if hp is None:
        hp = torch.from_numpy(phase_major(design_filter(up, down), up)).to(device)
        assert hp.shape[1] == native.load().m2m_ingest_phase_taps(up, down)
        with _filters_lock:
            hp = _filters.setdefault(key, hp)
    return hp


def _cuda_device(device) -> torch.device:
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise ValueError(f"the device ingest runs on a GPU, not on {device}")
    return torch.device("cuda", torch.cuda.current_device() if device.index is None else device.index)


def _resample(y: torch.Tensor, up: int, down: int, capacity: int) -> torch.Tensor:
    """``capacity`` samples: resample_poly(y, up, down), then zeros.  Enqueued on the current stream of y's device."""
    n_in = int(y.shape[0])
    device = y.device
    if capacity > MAX_OUT:
        raise ValueError(f"the resampled signal of {capacity} samples exceeds the device limit of {MAX_OUT}")
    with torch.cuda.device(device):
        hp = None if up == down else _filter_on(device, up, down)
        out = torch.empty(capacity, dtype=torch.float32, device=device)
        native.check(native.load().m2m_ingest_resample_f32(
            y.data_ptr(), n_in, up, down, None if hp is None else hp.data_ptr(), 10 * max(up, down), out.data_ptr(), capacity,
            native.stream_handle(device)), "m2m_ingest_resample_f32")
    return out


def _padded(n: int, pad_to: Optional[int]) -> int:
    if pad_to is None:
        return n
    if int(pad_to) < 1:
        raise ValueError(f"pad_to = {pad_to} must be a positive number of samples")
    return -(-n // int(pad_to)) * int(pad_to)


def resample_device(y: torch.Tensor, orig_sr: float, target_sr: float, pad_to: Optional[int] = None) -> torch.Tensor:
    """``audio.resample(y, orig_sr, target_sr)`` for a CUDA fp32 [n] tensor: the same samples, bit for bit.  With ``pad_to = k`` the
    result is zero-padded to the next multiple of k samples by the same kernel.  Equal rates return ``y`` itself, as the host does."""
    if not (isinstance(y, torch.Tensor) and y.is_cuda and y.dim() == 1 and y.dtype == torch.float32):
        raise ValueError("resample_device: y must be a CUDA float32 tensor [n]")
    n_in = int(y.shape[0])
    if orig_sr == target_sr:
        up = down = 1
    else:
        up, down = ratio(orig_sr, target_sr)
    if n_in > MAX_FRAMES:
        raise ValueError(f"resample_device: {n_in} samples exceed the device limit of {MAX_FRAMES}")
    n_out = resampled_length(n_in, up, down)
    capacity = _padded(n_out, pad_to)
    if n_in == 0 or (up == down and capacity == n_in):
        return y if capacity == n_in else y.new_zeros(capacity)
    return _resample(y.contiguous(), up, down, capacity)


def decode_pcm_device(body: torch.Tensor, n_frames: int, channels: int, kind: str) -> torch.Tensor:
    """``read_wav(...)[0].mean(axis=1)`` for the interleaved sample bytes of a ``data`` chunk: ``body`` is a CUDA uint8 tensor of at
    least ``n_frames * channels * width`` bytes (any alignment), ``kind`` one of ``u8 s16 s24 s32 f32 f64``."""
    if kind not in FORMATS:
        raise ValueError(f"decode_pcm_device: unknown sample format {kind!r}")
    code, width = FORMATS[kind]
    if not (isinstance(body, torch.Tensor) and body.is_cuda and body.dim() == 1 and body.dtype == torch.uint8 and body.is_contiguous()):
        raise ValueError("decode_pcm_device: body must be a contiguous CUDA uint8 tensor")
    if not 1 <= channels <= MAX_CHANNELS:
        raise ValueError(f"decode_pcm_device: {channels} channels (the device path takes 1..{MAX_CHANNELS})")
    if not 0 <= n_frames <= MAX_FRAMES:
        raise ValueError(f"decode_pcm_device: {n_frames} frames (the device path takes up to {MAX_FRAMES})")
    if n_frames * channels * width > int(body.shape[0]):
        raise ValueError(f"decode_pcm_device: {n_frames} frames of {channels} x {width} bytes do not fit in {int(body.shape[0])} bytes")
    device = body.device
    with torch.cuda.device(device):
        out = torch.empty(n_frames, dtype=torch.float32, device=device)
        if n_frames:
            native.check(native.load().m2m_ingest_pcm(body.data_ptr(), n_frames, channels, code, out.data_ptr(),
                                                      native.stream_handle(device)), "m2m_ingest_pcm")
    return out


def _inspect(path):
    """(layout, sample kind, bytes per sample, frames in the file); ``ValueError`` for a file the device path cannot take."""
    with open(path, "rb") as f:
        try:
            raw = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
        except ValueError:                                   # an empty file cannot be mapped
            raw = b""
        try:
            lay = wav_layout(path, raw)
        finally:
            if raw:
                raw.close()
    kind = wav_sample_format(path, lay.tag, lay.bits)
    width = FORMATS[kind][1]
    if lay.n_ch > MAX_CHANNELS:
        raise ValueError(f"{path}: {lay.n_ch} channels (the device path takes 1..{MAX_CHANNELS}; the host path takes any)")
    frames = lay.data_size // (width * lay.n_ch)
    if frames > MAX_FRAMES:
        raise ValueError(f"{path}: {frames} frames exceed the device limit of {MAX_FRAMES}")
    return lay, kind, width, frames


def eligible(path, sr: Optional[float] = None) -> bool:
    """True when ``load_audio_device(path, sr)`` can take the file: RIFF/WAVE, a sample format ``read_wav`` converts, at most 7
    channels and 2^28 frames - and, with ``sr`` given, a rate ratio within 1..1000 / 1..1000.  A file that cannot be read is not."""
    try:
        lay = _inspect(path)[0]
        if sr is not None and lay.rate != sr:
            ratio(lay.rate, sr)
    except (ValueError, OSError):
        return False
    return True


def load_audio_device(path, sr: float, device=None, offset: float = 0.0, duration: Optional[float] = None,
                      pad_to: Optional[int] = None) -> torch.Tensor:
    """``audio.load_audio(path, sr)`` (its scipy definition) as a CUDA fp32 tensor, computed on the device.  ``offset`` / ``duration``
    are seconds at the file's own rate, applied before resampling as ``librosa.load`` applies them: frames
    ``[int(offset * rate), int(offset * rate) + int(duration * rate))``, and only their bytes are uploaded.  With ``pad_to = k`` the
    result is zero-padded to the next multiple of k samples."""
    device = _cuda_device(device)
    lay, kind, width, frames = _inspect(path)
    first = min(frames, max(0, int(offset * lay.rate)))
    count = frames - first if duration is None else min(frames - first, max(0, int(duration * lay.rate)))
    up, down = (1, 1) if lay.rate == sr else ratio(lay.rate, sr)
    capacity = _padded(resampled_length(count, up, down), pad_to)
    if count == 0:
        return torch.zeros(capacity, dtype=torch.float32, device=device)
    frame_bytes = width * lay.n_ch
    with open(path, "rb") as f:
        # a private mapping is writable without touching the file, which lets torch wrap the pages without a copy of its own
        raw = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_COPY)
    host = np.frombuffer(raw, np.uint8, count * frame_bytes, lay.data_offset + first * frame_bytes)
    with torch.cuda.device(device):
        body = torch.from_numpy(host).to(device)             # a fresh allocation: aligned wherever the chunk lay in the file
        del host, raw
        mono = decode_pcm_device(body, count, lay.n_ch, kind)
        if up == down and capacity == count:
            return mono
        return _resample(mono, up, down, capacity)
