"""CPU: the host arithmetic of the on-device augmentation (music2midi_amd.augment, csrc/augment.hip) against what
music2midi_amd/audio.py computes, the polyphase formula the resampling kernel evaluates against scipy's resample_poly, the
reference's random draws, the note handling, and the refusals the library makes without a device."""
import ctypes as C
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
import torch

from music2midi_amd import audio, augment, native
from music2midi_amd.input import ModelInputs

ROOT = Path(__file__).resolve().parents[1]
STEPS = list(range(-12, 13))
LENGTHS = [1, 511, 512, 2085, 5000, 66150]


# ------------------------------------------------------------------------------------------------ m2m_augment_plan
@pytest.mark.parametrize("T", LENGTHS)
def test_plan_matches_what_audio_py_computes(T):
    for step in STEPS:
        p = augment.plan(T, step)
        F = 1 + T // 512                                   # audio._stft: 1 + (T + 2048 - 2048) // 512
        assert p.frames == F and p.cap_frames == 2 * F and p.cap_len == 2 * T
        if step == 0:
            assert (p.stretched_frames, p.stretched_len, p.up, p.down, p.taps) == (F, T, 1, 1, 0)
            continue
        rate = 2.0 ** (-float(step) / 12)
        frac = Fraction(rate).limit_denominator(1000)
        assert p.stretched_frames == len(np.arange(0, F, rate, dtype=np.float64)), (T, step)
        assert p.stretched_len == int(round(T / rate)), (T, step)
        assert (p.up, p.down) == (frac.numerator, frac.denominator), (T, step)
        assert p.taps == 20 * max(p.up, p.down) + 1
        assert p.stretched_frames <= p.cap_frames and p.stretched_len <= p.cap_len


def test_plan_ratio_is_the_one_audio_resample_takes_at_the_training_rate():
    """audio.pitch_shift hands resample() sr / rate and sr, not rate: the fraction is the same for every step."""
    for sr in (16000.0, 22050.0, 44100.0):
        for step in STEPS:
            if step == 0:
                continue
            rate = 2.0 ** (-float(step) / 12)
            frac = Fraction(sr / (sr / rate)).limit_denominator(1000)
            p = augment.plan(5000, step)
            assert (p.up, p.down) == (frac.numerator, frac.denominator), (sr, step)


def test_plan_refuses_out_of_range_arguments():
    for T, step, msg in [(0, 1, "T=0"), ((1 << 22) + 1, 1, "out of range"), (100, 13, "step 13"), (100, -13, "step -13")]:
        with pytest.raises(native.NativeError, match=msg):
            augment.plan(T, step)


# ------------------------------------------------------------------------------------------------ the resampling filter
@pytest.mark.parametrize("step", [s for s in STEPS if s != 0])
def test_filter_is_the_one_resample_poly_designs_for_fp32_input(step):
    """scipy: h = firwin(2 half + 1, 1 / max(up, down), window=("kaiser", 5.0)).astype(float32); h *= up.  The library designs it
    in C in float64 (its own Bessel series and sinc, a sequential sum) and rounds the same way.  Every float64 tap is a product of
    four correctly-rounded-to-a-few-ulp factors whose absolute error is a few float64 eps of the LARGEST tap (sin near a multiple
    of pi loses relative, not absolute, accuracy): 8 eps is the allowance.  After the cast a tap is therefore scipy's fp32 value,
    or its fp32 neighbour where the float64 value sits within that distance of a rounding boundary."""
    from scipy.signal import firwin
    p = augment.plan(5000, step)
    h = augment.resample_filter(step)
    assert h.dtype == np.float32 and len(h) == p.taps
    mx = max(p.up, p.down)
    ref = firwin(20 * mx + 1, 1.0 / mx, window=("kaiser", 5.0)).astype(np.float32)
    ref *= p.up
    diff = np.abs(h.astype(np.float64) - ref.astype(np.float64))
    allowed = np.maximum(np.spacing(np.abs(ref)).astype(np.float64), 8 * np.finfo(np.float64).eps * float(np.abs(ref).max()))
    assert np.all(diff <= allowed), (step, float((diff / allowed).max()))
    # the 20 zeros of the sinc (taps a multiple of max(up, down) from the centre) hold rounding noise of that size in both tables
    zeros = 10 * mx + mx * np.concatenate([np.arange(-10, 0), np.arange(1, 11)])
    assert np.all(np.abs(h[zeros]) <= 8 * np.finfo(np.float64).eps * float(np.abs(ref).max()))
    assert np.array_equal(h, h[::-1])                      # linear phase


def test_step_zero_has_no_filter():
    assert len(augment.resample_filter(0)) == 0


def _polyphase(x, h, up, down):
    """The formula of the resampling kernel, restated: out[n] = sum_m x[m] h[n down - m up + half_len], n < ceil(len up / down)."""
    half = (len(h) - 1) // 2
    n_out = -(-len(x) * up // down)
    out = np.zeros(n_out)
    for n in range(n_out):
        c = n * down
        lo = 0 if c - half <= 0 else (c - half + up - 1) // up
        hi = min((c + half) // up, len(x) - 1)
        m = np.arange(lo, hi + 1)
        out[n] = np.dot(x[m], h[c + half - m * up])
    return out


@pytest.mark.parametrize("up,down", [(1393, 985), (221, 295), (1, 2)])
@pytest.mark.parametrize("n", [777, 4097])
def test_polyphase_formula_equals_resample_poly(up, down, n):
    from scipy.signal import firwin, resample_poly
    x = np.random.default_rng(n + up).standard_normal(n)
    mx = max(up, down)
    h = up * firwin(20 * mx + 1, 1.0 / mx, window=("kaiser", 5.0))
    ref = resample_poly(x, up, down)
    got = _polyphase(x, h, up, down)
    assert got.shape == ref.shape
    # 20 to 41 products of O(1) terms per sample, float64 both ways: a few ulps of the largest sample
    assert np.abs(got - ref).max() <= 64 * np.finfo(np.float64).eps * np.abs(ref).max()
    c = (len(ref) // 2) * down                             # an interior sample: 20 max(up, down) / up taps, give or take one
    taps = (c + 10 * mx) // up - (c - 10 * mx + up - 1) // up + 1
    assert 20 <= taps <= 41


# ------------------------------------------------------------------------------------------------ draws and notes
def test_draw_reproduces_the_references_two_draws_per_clip():
    """ref dataset.py:130-132: ``np.random.rand() < 0.5`` then ``np.random.randint(-6, 6)`` per clip, in that order."""
    rng, twin = np.random.default_rng(1234), np.random.default_rng(1234)
    steps, flags = augment.draw(9, rng)
    want = [(bool(twin.random() < 0.5), int(twin.integers(-6, 6))) for _ in range(9)]
    assert flags == [w[0] for w in want] and steps == [w[1] for w in want]
    assert all(isinstance(s, int) for s in steps) and all(isinstance(f, bool) for f in flags)
    many, flags_many = augment.draw(4000, np.random.default_rng(0))
    assert set(many) == set(range(-6, 6)) and 0.45 < np.mean(flags_many) < 0.55
    assert rng.random() == twin.random()                   # nothing else was drawn


def test_shift_notes_copies_and_moves_the_pitch_column():
    a = np.array([[0.1, 0.5, 60, 80], [0.2, 0.9, 72, 64]])
    b = np.array([[0.0, 1.0, 40, 100]], dtype=np.float32)
    before = (a.copy(), b.copy())
    out = augment.shift_notes((a, b), [5, -6])
    assert isinstance(out, tuple) and len(out) == 2
    for got, src, step in zip(out, (a, b), (5, -6)):
        want = audio.transpose(np.zeros(4, np.float32), src, step, 22050)[1]      # the host function's notes
        assert got.dtype == np.float64 and np.array_equal(got, want) and not np.shares_memory(got, src)
    assert np.array_equal(a, before[0]) and np.array_equal(b, before[1])


def test_transpose_batch_refuses_a_host_waveform_and_wrong_lengths():
    inputs = ModelInputs(input_waveform=torch.zeros(2, 100), notes_batch=(np.zeros((1, 4)),) * 2, cond_index=None)
    with pytest.raises(ValueError, match="CUDA float32"):
        augment.transpose_batch(inputs, [1, 2])
    with pytest.raises(ValueError, match="3 entries for a batch of 2"):
        augment.transpose_batch(inputs, [1, 2, 3])
    with pytest.raises(TypeError, match="whole semitones"):
        augment.transpose_batch(inputs, [1.5, 2.0])


# ------------------------------------------------------------------------------------------------ header and binding
def test_header_declares_what_the_binding_binds():
    header = (ROOT / "include" / "music2midi_amd.h").read_text()
    for name, proto in [
            ("m2m_augment_create", "int  m2m_augment_create(m2m_augment** out);"),
            ("m2m_augment_destroy", "void m2m_augment_destroy(m2m_augment* a);"),
            ("m2m_augment_plan", "int m2m_augment_plan(const m2m_augment* a, int T, int step, m2m_augment_plan_t* out);"),
            ("m2m_augment_filter", "int m2m_augment_filter(int step, float* out_host, int n);"),
            ("m2m_augment_workspace_bytes", "int64_t m2m_augment_workspace_bytes(int B, int T);"),
            ("m2m_pitch_shift_f32", "int m2m_pitch_shift_f32(const m2m_augment* a, const float* wav_dev, int B, int T, const int* steps_host,")]:
        assert proto in header, name
        assert name in native.EXPORTED_SYMBOLS and hasattr(native.load(), name)
    assert "#define M2M_ABI_VERSION 1" in header and native.load().m2m_abi_version() == 1
    assert len(native._SIGNATURES["m2m_pitch_shift_f32"][1]) == 10
    assert native._SIGNATURES["m2m_augment_workspace_bytes"][0] is C.c_int64
    # the structs, field for field
    body = re.search(r"typedef struct \{([^}]*)\} m2m_augment_plan_t;", header).group(1)
    fields = [f.strip() for decl in re.findall(r"int ([a-z_, ]+);", body) for f in decl.split(",")]
    assert fields == [n for n, _ in native.AugmentPlan._fields_] and C.sizeof(native.AugmentPlan) == 4 * len(fields)
    body = re.search(r"typedef struct \{([^}]*)\} m2m_augment_stages;", header).group(1)
    assert re.findall(r"float\* ([a-z_]+);", body) == [n for n, _ in native.AugmentStages._fields_]


def test_workspace_query():
    lib = native.load()
    for B, T in [(1, 1), (3, 2085), (16, 66150)]:
        F = 1 + T // 512
        need = lib.m2m_augment_workspace_bytes(B, T)
        # the STFT, the stretched STFT at the extreme rate (2 F frames) and the stretched waveform (2 T samples)
        assert need >= B * (F * 1025 * 8 + 2 * F * 1025 * 8 + 2 * T * 4)
        assert need <= B * (3 * F * 1025 * 8 + 2 * T * 4 + 4) + 4 * 256
    for B, T in [(0, 100), (65536, 100), (1, 0), (1, (1 << 22) + 1)]:
        assert lib.m2m_augment_workspace_bytes(B, T) == -1
        assert b"out of range" in lib.m2m_last_error()


# ------------------------------------------------------------------------------------------------ refusals without a device
@pytest.mark.parametrize("B,T,steps,out,msg", [
    (0, 100, [0], 0x200000, "batch 0 out of range"),
    (65536, 100, [0], 0x200000, "batch 65536 out of range"),
    (2, 0, [0, 0], 0x200000, "T=0 out of range"),
    (2, (1 << 22) + 1, [0, 0], 0x200000, "out of range"),
    (2, 100, [0, 13], 0x200000, "step 13 of clip 1"),
    (2, 100, [-13, 0], 0x200000, "step -13 of clip 0"),
    (2, 100, [1, 2], 0x100000, "overlaps"),
    (2, 100, [1, 2], 0x100000 + 4 * 199, "overlaps"),
    (2, 100, [1, 2], 0x100000 - 4 * 199, "overlaps"),
])
def test_limits_are_refused_before_the_handle_is_looked_at(B, T, steps, out, msg):
    """The limits are checked on the arguments alone, first: no handle, no device, fake (never dereferenced) device addresses."""
    lib = native.load()
    arr = (C.c_int * max(len(steps), 1))(*steps)
    st = lib.m2m_pitch_shift_f32(None, 0x100000, B, T, arr, None, out, None, None, None)
    assert st == -1
    assert msg in lib.m2m_last_error().decode()


def test_a_valid_call_without_a_handle_is_refused_too():
    lib = native.load()
    arr = (C.c_int * 2)(1, -2)
    assert lib.m2m_pitch_shift_f32(None, 0x100000, 2, 100, arr, None, 0x100000 + 800, None, None, None) == -1
    assert b"null handle" in lib.m2m_last_error()
