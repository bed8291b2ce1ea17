"""The dataset-side augmentation on the device: peak normalisation + pitch shift of a waveform batch.

ref: music2midi/dataset.py:131-133,157-160 — every training clip is normalised with probability 1/2 and transposed by
``randint(-6, 6)`` semitones (audio and note pitches).  ``music2midi_amd.audio`` restates that on the host (numpy, float64
inside) and stays the definition; here the same pipeline runs as HIP kernels (csrc/augment.hip) on the batch that is on the
device anyway for the log-mel kernel, on the caller's stream, without a trip to the host.

    pitch_shift_batch(waveform [B, T] cuda fp32, n_steps, normalize=None)   -> [B, T]
    transpose_batch(inputs, n_steps, normalize=None)                      -> ModelInputs (waveform shifted, notes copied + step)
    draw(B, rng) -> (n_steps, normalize);   augment(inputs, rng) = transpose_batch(inputs, *draw(B, rng))

There is no fallback: a missing library or a refused call raises ``native.NativeError``.
"""
from __future__ import annotations

import ctypes as C
import threading
import weakref
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import native
from .input import ModelInputs

N_BINS = 1025


class Stages:
    """The intermediates of one call, as the host functions name them (``return_stages=True``; the tests localise a failure with
    them).  ``stft[b]`` is ``audio._stft`` transposed ([frames, 1025] complex64), ``stretched_stft[b]`` the phase vocoder's output
    ([stretched_frames, 1025]), ``stretched_wave[b]`` ``audio.time_stretch`` ([stretched_len]); ``None`` for a step-0 clip."""

    def __init__(self, stft, stretched_stft, stretched_wave):
        self.stft, self.stretched_stft, self.stretched_wave = stft, stretched_stft, stretched_wave


def plan(T: int, step: int) -> native.AugmentPlan:
    """What ``audio.pitch_shift`` computes on the way (frames, stretched extents, resampling ratio): host arithmetic, no GPU."""
    p = native.AugmentPlan()
    native.check(native.load().m2m_augment_plan(None, int(T), int(step), C.byref(p)), "m2m_augment_plan")
    return p


def resample_filter(step: int) -> np.ndarray:
    """The fp32 polyphase filter the resampling kernel applies for ``step`` (host arithmetic, no GPU)."""
    lib = native.load()
    n = lib.m2m_augment_filter(int(step), None, 0)
    native.check(min(n, 0), "m2m_augment_filter")
    h = np.zeros(n, np.float32)
    if n:
        native.check(min(lib.m2m_augment_filter(int(step), h.ctypes.data, n), 0), "m2m_augment_filter")
    return h


class _Augmenter:
    """Native handle of one device (read-only tables) + one workspace per stream, each growing with (B, T).  A workspace is
    allocated on, and only ever used by, the stream it is keyed by: calls on different streams of a device do not share the
    intermediates, and a workspace that is replaced by a larger one is returned to the allocator on the stream that used it."""

    def __init__(self, device: torch.device):
        native.require_gpu()
        self.device = device
        handle = C.c_void_p()
        with torch.cuda.device(device):
            native.check(native.load().m2m_augment_create(C.byref(handle)), "m2m_augment_create")
        self.handle = handle
        self.workspaces: dict = {}
        self._finalizer = weakref.finalize(self, native.load().m2m_augment_destroy, handle)

    def workspace_for(self, B: int, T: int) -> torch.Tensor:
        """The workspace of torch's current stream on the device (the stream ``pitch_shift_batch`` enqueues on)."""
        need = native.load().m2m_augment_workspace_bytes(B, T)
        native.check(min(need, 0), "m2m_augment_workspace_bytes")
        with torch.cuda.device(self.device):
            key = native.stream_handle(self.device)
            with _cache_lock:
                ws = self.workspaces.get(key)
                if ws is None or ws.numel() < need:
                    ws = self.workspaces[key] = torch.empty(need, dtype=torch.uint8, device=self.device)
        return ws


_cache: dict = {}
_cache_lock = threading.Lock()


def _augmenter(device: torch.device) -> _Augmenter:
    key = device.index if device.index is not None else torch.cuda.current_device()
    with _cache_lock:
        aug = _cache.get(key)
        if aug is None:
            aug = _cache[key] = _Augmenter(torch.device("cuda", key))
        return aug


def _check_steps(n_steps, B: int) -> np.ndarray:
    steps = np.asarray(list(n_steps))
    if steps.size == 0:
        steps = steps.astype(np.int32)
    if steps.shape != (B,):
        raise ValueError(f"n_steps has {steps.size} entries for a batch of {B}")
    if not np.issubdtype(steps.dtype, np.integer):
        raise TypeError("n_steps must be whole semitones (ints)")
    return steps.astype(np.int32)


def _check_flags(normalize, B: int) -> Optional[np.ndarray]:
    if normalize is None:
        return None
    flags = np.asarray(list(normalize)).astype(bool)
    if flags.shape != (B,):
        raise ValueError(f"normalize has {flags.size} entries for a batch of {B}")
    return flags.astype(np.uint8)


def pitch_shift_batch(waveform: torch.Tensor, n_steps: Sequence[int], normalize=None, return_stages: bool = False):
    """``audio.pitch_shift(audio.normalize(y) if normalize[b] else y, sr, n_steps[b])`` for every clip of a CUDA fp32 batch
    [B, T], on the current stream.  The sample rate does not enter: the shift is a ratio.  Step 0 copies the clip (bit-equal);
    a clip's result does not depend on the rest of the batch.  With ``return_stages`` the result is ``(out, Stages)``."""
    if not (isinstance(waveform, torch.Tensor) and waveform.is_cuda and waveform.dim() == 2 and waveform.dtype == torch.float32):
        raise ValueError("pitch_shift_batch: waveform must be a CUDA float32 tensor [B, T]")
    B, T = waveform.shape
    steps = _check_steps(n_steps, B)
    flags = _check_flags(normalize, B)
    wav = waveform.contiguous()
    lib = native.load()
    aug = _augmenter(wav.device)
    with torch.cuda.device(wav.device):
        out = torch.empty_like(wav)
        stages = None
        if return_stages and B >= 1 and T >= 1:
            p = plan(T, 0)
            bufs = (torch.zeros(B, p.frames, N_BINS, 2, dtype=torch.float32, device=wav.device),
                    torch.zeros(B, p.cap_frames, N_BINS, 2, dtype=torch.float32, device=wav.device),
                    torch.zeros(B, p.cap_len, dtype=torch.float32, device=wav.device))
            stages = native.AugmentStages(*(b.data_ptr() for b in bufs))
        # the limits (B, T, steps, aliasing) are the library's to refuse, before it looks at the workspace
        ws = aug.workspace_for(B, T) if 1 <= B <= 65535 and 1 <= T <= (1 << 22) else None
        native.check(lib.m2m_pitch_shift_f32(aug.handle, wav.data_ptr(), B, T, steps.ctypes.data_as(C.POINTER(C.c_int)),
                                             flags.ctypes.data if flags is not None else None, out.data_ptr(),
                                             ws.data_ptr() if ws is not None else None,
                                             C.byref(stages) if stages is not None else None, native.stream_handle(wav.device)),
                     "m2m_pitch_shift_f32")
    if not return_stages:
        return out
    per_clip = ([], [], [])
    for b in range(B):
        if steps[b] == 0:
            for lst in per_clip:
                lst.append(None)
            continue
        p = plan(T, int(steps[b]))
        per_clip[0].append(torch.view_as_complex(bufs[0][b]))
        per_clip[1].append(torch.view_as_complex(bufs[1][b, :p.stretched_frames]))
        per_clip[2].append(bufs[2][b, :p.stretched_len])
    return out, Stages(*per_clip)


def shift_notes(notes_batch, n_steps) -> tuple:
    """Copies of every clip's note array with the pitch column moved by the clip's step, as ``audio.transpose`` does."""
    out = []
    for notes, step in zip(notes_batch, n_steps):
        notes = np.array(notes, dtype=np.float64, copy=True)
        notes[:, 2] += int(step)
        out.append(notes)
    return tuple(out)


def transpose_batch(inputs: ModelInputs, n_steps: Sequence[int], normalize=None) -> ModelInputs:
    """ref: music2midi/dataset.py:131-133,157-160 for a whole batch: the waveform is (normalised and) shifted on the device,
    every clip's notes are copied with ``notes[:, 2] += step``; ``cond_index`` passes through.  The inputs are not modified."""
    n_steps = [int(s) for s in _check_steps(n_steps, inputs.input_waveform.shape[0])]
    waveform = pitch_shift_batch(inputs.input_waveform, n_steps, normalize)
    notes = shift_notes(inputs.notes_batch, n_steps) if inputs.notes_batch is not None else None
    return type(inputs)(input_waveform=waveform, notes_batch=notes, cond_index=inputs.cond_index)


def draw(B: int, rng: np.random.Generator) -> Tuple[list, list]:
    """The reference's two draws per clip, in its order: ``rng.random() < 0.5`` (normalise) and then ``rng.integers(-6, 6)``
    (semitones, -6..5 as ``np.random.randint(-6, 6)``).  Returns ``(n_steps, normalize)``."""
    n_steps, normalize = [], []
    for _ in range(int(B)):
        normalize.append(bool(rng.random() < 0.5))
        n_steps.append(int(rng.integers(-6, 6)))
    return n_steps, normalize


def augment(inputs: ModelInputs, rng: np.random.Generator) -> ModelInputs:
    return transpose_batch(inputs, *draw(inputs.input_waveform.shape[0], rng))
