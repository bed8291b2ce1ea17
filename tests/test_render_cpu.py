"""CPU: the definition of the note renderer (music2midi_amd/render.py) - the voice's tables, a single note, the order of the sum,
pack, the kernel's tile lists against a brute-force membership test - the refusals the library makes on its arguments alone, and
the host side of the surface built on it (SimpleMIDI.synthesize / fluidsynth, audio.write_wav, render.synthetic_batch)."""
import ctypes as C

import numpy as np
import pytest
import torch

from music2midi_amd import audio, native, render
from music2midi_amd.config import DEFAULT_CONFIG
from music2midi_amd.utils import SimpleMIDI, SimpleInstrument, SimpleNote

from render_cases import POLY_FS, POLY_SAMPLES, poly_batch, records, voice_struct

M2M_ERR_INVALID = -1
RATES = (16000, 48000)


# ------------------------------------------------------------------ the voice
@pytest.mark.parametrize("fs", RATES)
def test_voice_tables(fs):
    v = render.Voice(fs)
    assert v.wave.dtype == np.float32 and v.wave.shape == (6, 4097)
    assert np.array_equal(v.wave[:, 4096], v.wave[:, 0]) and not v.wave[:, 0].any()       # the guard entry; a sum of sines starts at 0
    assert np.array_equal(np.abs(v.wave).max(axis=1), np.ones(6, np.float32))             # scaled to peak 1
    k = np.arange(4096)
    assert np.abs(v.wave[0, :-1] - np.sin(2 * np.pi * k / 4096)).max() < 1e-7
    saw3 = sum(np.sin(2 * np.pi * h * k / 4096) / h for h in (1, 2, 3))
    assert np.abs(v.wave[2, :-1] - saw3 / np.abs(saw3).max()).max() < 1e-7
    f = 440.0 * 2.0 ** ((np.arange(128) - 69) / 12.0)
    for p in range(128):
        if f[p] >= fs / 2:
            assert v.silent[p], p
            continue
        assert not v.silent[p] and v.table[p] == min(6, int(np.floor((fs / 2 - 1) / f[p]))) >= 1, p
        assert int(v.inc[p]) == int(np.floor(f[p] / fs * 2.0 ** 32 + 0.5)), p
        assert f[p] * v.table[p] < fs / 2                                                  # the highest harmonic stays below Nyquist
    tau = 3.0 * 2.0 ** (-(np.arange(128) - 21) / 24.0) + 0.2
    assert np.array_equal(v.dec, np.floor(64.0 / (tau * fs) * 65536.0 + 0.5).astype(np.uint32)) and v.dec.dtype == np.uint32
    assert v.decay.dtype == np.float32 and v.decay.shape == (1025,) and v.decay[0] == 1.0
    assert np.array_equal(v.decay, np.exp(-np.arange(1025) / 64.0).astype(np.float32))
    assert (v.attack, v.release) == (int(0.002 * fs), int(0.05 * fs))
    assert v.inv_attack.dtype == np.float32 and v.inv_attack == np.float32(1) / np.float32(v.attack)


def test_table_choice_and_silent_pitches():
    lo, hi = render.Voice(16000), render.Voice(48000)
    assert [int(lo.table[p]) for p in (0, 21, 60, 69, 84, 96, 108, 119)] == [6, 6, 6, 6, 6, 3, 1, 1]
    assert [int(hi.table[p]) for p in (60, 96, 108, 115, 120, 127)] == [6, 6, 5, 3, 2, 1]
    assert np.flatnonzero(lo.silent).tolist() == list(range(120, 128)) and not hi.silent.any()
    assert {int(t) for t in lo.table[~lo.silent]} == {1, 2, 3, 4, 5, 6} == {int(t) for t in hi.table}
    y = render.render_host(np.array([[0.0, 0.5, 127, 100]]), 16000, 4000)                  # would alias to 3456 Hz
    assert not y.any()
    with pytest.raises(ValueError, match="power of two"):
        render.Voice(16000, table_size=3000)
    with pytest.raises(ValueError, match="power of two"):
        render.Voice(16000, table_size=128)


# ------------------------------------------------------------------ a single note
@pytest.mark.parametrize("fs", RATES)
def test_single_note_extent_and_pitch(fs):
    v = render.default_voice(fs)
    for p in (21, 60, 69, 108):
        n = 2 * fs
        y = render.render_host(np.array([[0.25, 1.25, p, 100]]), fs, n)
        on, off = int(np.floor(0.25 * fs + 0.5)), int(np.floor(1.25 * fs + 0.5))
        assert y.dtype == np.float32 and y.shape == (n,)
        assert not y[:on].any() and not y[off + v.release:].any() and y[on + 1:off + v.release].any()
        assert np.array_equal(y[:on].view(np.uint32), np.zeros(on, np.uint32))             # +0, not -0
        spectrum = np.abs(np.fft.rfft(y * np.hanning(n)))
        assert abs(np.argmax(spectrum) * fs / n - 440.0 * 2.0 ** ((p - 69) / 12.0)) <= fs / n, p   # within one bin
        assert 0.15 < np.abs(y).max() <= 0.25 * 100 / 127 * 1.0001
    # a note that begins before the clip is already sounding at sample 0; the default length is the last off + R
    y = render.render_host(np.array([[-0.5, 0.5, 60, 100]]), fs)
    assert len(y) == int(0.5 * fs) + v.release and y[0] != 0 and y[-1] != 0
    whole = render.render_host(np.array([[0.0, 1.0, 60, 100]]), fs)
    assert np.array_equal(y, whole[int(0.5 * fs):])                                        # the same samples, shifted
    assert render.render_host(np.zeros((0, 4)), fs).shape == (0,)


def test_two_notes_are_the_fp32_sum_in_packed_order():
    fs, n = 16000, 12000
    a, b, c = [0.30, 0.60, 64, 90], [0.10, 0.50, 60, 127], [0.30, 0.45, 67, 40]
    solo = {k: render.render_host(np.array([x]), fs, n) for k, x in (("a", a), ("b", b), ("c", c))}
    y = render.render_host(np.array([a, b, c]), fs, n)
    want = ((np.zeros(n, np.float32) + solo["b"]) + solo["a"]) + solo["c"]                 # by onset; a before c: equal onsets keep their order
    assert want.dtype == np.float32 and np.array_equal(y.view(np.uint32), want.view(np.uint32))
    other = ((np.zeros(n, np.float32) + solo["c"]) + solo["a"]) + solo["b"]
    assert not np.array_equal(y, other)                                                    # the order is observable
    peak = np.abs(y).max()
    assert np.array_equal(render.render_host(np.array([a, b, c]), fs, n, normalize=True), y / peak)
    assert np.array_equal(render.render_batch_host([np.array([a]), np.zeros((0, 4)), np.array([a, b, c])], fs, n),
                          np.stack([solo["a"], np.zeros(n, np.float32), y]))


# ------------------------------------------------------------------ pack
def test_pack_drops_and_orders():
    fs, n = 16000, 16000
    notes = np.array([[0.50, 0.60, 60, 80],        # 0 kept
                      [0.20, 0.20, 61, 80],        # 1 off == on
                      [0.30, 0.10, 62, 80],        # 2 off < on
                      [0.10, 0.40, 125, 80],       # 3 silent at 16 kHz
                      [1.00, 1.20, 63, 80],        # 4 begins at n_samples: no sample inside
                      [-1.00, -0.06, 64, 80],      # 5 released before the clip: off + R = -960 + 800 <= 0
                      [-1.00, -0.04, 65, 80],      # 6 its release reaches into the clip
                      [0.50, 0.70, 66, 1],         # 7 same onset as 0: stays behind it
                      [0.10, 5.00, 67, 127],       # 8 cut by the end
                      [0.50, 0.55, 59, 64],        # 9 same onset again
                      [0.99998, 1.5, 68, 80]])     # 10 rounds to n_samples
    pk = render.pack(notes, fs, n)
    assert pk.index.tolist() == [6, 8, 0, 7, 9]
    assert pk.on.tolist() == [-16000, 1600, 8000, 8000, 8000] and pk.off.tolist() == [-640, 80000, 9600, 11200, 8800]
    assert pk.pitch.tolist() == [65, 67, 60, 66, 59] and pk.on.dtype == np.int64
    assert np.array_equal(pk.gain, np.float32(0.25) * (np.array([80, 127, 80, 1, 64], np.float32) / np.float32(127))) and pk.gain.dtype == np.float32
    assert render.pack(notes, fs).index.tolist() == [6, 8, 0, 7, 9, 4, 10]                 # no n_samples: nothing is cut at the end
    # the same sample grid under the 48 kHz voice: R = 2400 reaches into the clip from note 5, and pitch 125 sounds
    assert render.pack(notes, fs, voice=render.Voice(48000)).index.tolist() == [5, 6, 3, 8, 0, 7, 9, 4, 10]
    assert render.pack(np.array([[2.0 ** -15, 1.0, 60, 80]]), 16384, 100).on.tolist() == [1]   # 0.5 rounds up: floor(x + 0.5)
    with pytest.raises(ValueError, match="before the clip"):
        render.pack(np.array([[-70000.0, 1.0, 60, 80]]), 16000, 100)
    with pytest.raises(ValueError, match="outside 0..127"):
        render.pack(np.array([[0.0, 1.0, 128, 80]]), 16000, 100)


# ------------------------------------------------------------------ the tile lists
def test_tile_lists_against_brute_force_membership():
    v = render.default_voice(POLY_FS)
    packed = [render.pack(n, POLY_FS, POLY_SAMPLES, v) for n in poly_batch()]
    for tile in (render.tile_size(), 1000, 4096):
        tiles = -(-POLY_SAMPLES // tile)
        start, entries = render.tile_lists(packed, POLY_SAMPLES, tile, v.release)
        assert start.dtype == entries.dtype == np.int32 and start.shape == (3 * tiles + 1,)
        assert start[0] == 0 and start[-1] == len(entries) and (np.diff(start) >= 0).all()
        base = 0
        for c, pk in enumerate(packed):
            lo, hi = np.maximum(pk.on, 0), np.minimum(pk.off + v.release, POLY_SAMPLES)
            for t in range(tiles):
                want = [base + i for i in range(len(pk.on)) if lo[i] < (t + 1) * tile and hi[i] > t * tile]     # ascending: packed order
                assert entries[start[c * tiles + t]:start[c * tiles + t + 1]].tolist() == want, (tile, c, t)
            base += len(pk.on)
        assert start[tiles] == start[2 * tiles]                                            # the empty clip
    sounding = np.mean([((packed[0].on <= n) & (n < packed[0].off)).sum() for n in range(24000, 120000, 1000)])
    assert 50 < sounding < 52                                                               # 50.8: the figure render_cases states


# ------------------------------------------------------------------ the C ABI
def test_binding_and_tile():
    lib = native.load()
    for name in ("m2m_render_tile", "m2m_render_notes_f32"):
        assert name in native.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert C.sizeof(native.RenderNote) == 24 and C.sizeof(native.RenderVoice) == 40
    tile = lib.m2m_render_tile()
    assert tile == render.tile_size() and tile >= 64 and tile & (tile - 1) == 0
    # the records render() writes with numpy are the struct's layout
    v = render.default_voice(16000)
    pk = render.pack(np.array([[0.1, 0.2, 60, 100], [-0.1, 9.0, 100, 3]]), 16000, 8000, v)
    rec = records([pk], v, 8000)
    assert rec.shape == (2, 6) and rec[:, 0].tolist() == [-1600, 1600] and rec[:, 1].tolist() == [8000, 3200]
    assert rec[:, 2].view(np.uint32).tolist() == [int(v.inc[100]), int(v.inc[60])] and rec[:, 4].tolist() == [int(v.table[100]) - 1, 5]
    assert np.array_equal(rec[:, 5].view(np.float32), pk.gain)


def test_every_refusal_is_made_without_a_gpu():
    """M2M_ERR_INVALID on the arguments alone: the pointers are never dereferenced, no HIP call is made."""
    lib = native.load()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)                                                                   # never touched: only compared
    v = render.Voice(16000)
    ok = dict(notes=a, n_notes=10, start=a + 1024, entries=a + 2048, n_entries=30, out=a + 4096, n=16000, stride=16000, clips=2,
              wave=a + 8192, decay=a + 12288, voice={})

    def call(**change):
        k = dict(ok, **change)
        vs = voice_struct(v, k["wave"], k["decay"], **(k["voice"] or {}))
        return lib.m2m_render_notes_f32(k["notes"], k["n_notes"], k["start"], k["entries"], k["n_entries"], None if k["voice"] is None else C.byref(vs),
                                        k["out"], k["n"], k["stride"], k["clips"], None)
    bad = [dict(n=0), dict(n=-5), dict(n=(1 << 28) + 1, stride=(1 << 28) + 1), dict(clips=0), dict(clips=65536), dict(n_notes=-1),
           dict(n_notes=(1 << 20) + 1), dict(n_entries=-1), dict(n_entries=1 << 31), dict(n_notes=0, n_entries=1), dict(stride=15999),
           dict(voice=dict(attack=0)), dict(voice=dict(attack=(1 << 24) + 1)), dict(voice=dict(release=0)), dict(voice=dict(release=(1 << 24) + 1)),
           dict(voice=dict(table_size=4097)), dict(voice=dict(table_size=4095)), dict(voice=dict(table_size=128)), dict(voice=dict(table_size=1 << 17)),
           dict(voice=dict(table_size=0)), dict(voice=dict(table_size=-4096)), dict(voice=dict(n_tables=0)), dict(voice=dict(n_tables=65)),
           dict(voice=dict(decay_steps=0)), dict(voice=dict(decay_steps=(1 << 24) + 1)), dict(voice=dict(reserved=1)),
           dict(notes=None), dict(entries=None), dict(start=None), dict(out=None), dict(wave=None), dict(decay=None), dict(voice=None),
           dict(n_notes=0, n_entries=0, start=None), dict(out=a + 4098), dict(notes=a + 1), dict(wave=a + 8195)]
    for change in bad:
        assert call(**change) == M2M_ERR_INVALID, change
        assert b"m2m_render_notes_f32" in lib.m2m_last_error(), change
    assert b"4-byte aligned" in lib.m2m_last_error()


# ------------------------------------------------------------------ the surface on the host
def _midi(notes):
    midi = SimpleMIDI()
    inst = SimpleInstrument()
    inst.notes = [SimpleNote(*n) for n in notes]
    midi.instruments.append(inst)
    return midi


def test_simple_midi_synthesize_and_fluidsynth():
    """Without a GPU these go through the definition; with one they render on it and give the same samples."""
    notes = [(0.0, 0.5, 60, 80), (0.25, 1.0, 64, 100), (0.5, 1.0, 67, 60)]
    midi = _midi(notes)
    y = midi.synthesize(fs=16000)
    assert y.dtype == np.float64 and y.shape == (16000 + 800,)
    assert np.array_equal(y, render.render_host(np.array(notes), 16000).astype(np.float64))
    z = midi.fluidsynth(fs=16000)
    assert z.dtype == np.float64 and z.shape == y.shape and np.abs(z).max() == 1.0 and np.isfinite(z).all()
    assert np.array_equal(z.astype(np.float32), y.astype(np.float32) / np.float32(np.abs(y).max()))
    assert midi.fluidsynth().shape == (44100 + 2205,) and midi.synthesize().shape == (44100 + 2205,)     # PrettyMIDI's default rate
    with pytest.raises(ImportError, match="SoundFont"):
        midi.fluidsynth(fs=16000, sf2_path="piano.sf2")
    assert "not a soundfont" in SimpleMIDI.fluidsynth.__doc__.lower().replace("\n", " ")
    assert _midi([]).fluidsynth(fs=16000).shape == (0,)


def test_write_wav_read_wav_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    y = np.concatenate([rng.uniform(-1, 1, 5000), [1.0, -1.0, 0.0, 1.5, -1.5]]).astype(np.float32)
    audio.write_wav(tmp_path / "y.wav", y, 48000)
    raw = (tmp_path / "y.wav").read_bytes()
    lay = audio.wav_layout("y.wav", raw)
    assert (lay.tag, lay.n_ch, lay.rate, lay.bits, lay.data_size) == (1, 1, 48000, 16, 2 * len(y)) and len(raw) == 44 + 2 * len(y)
    back, rate = audio.read_wav(tmp_path / "y.wav")
    assert rate == 48000 and back.shape == (len(y), 1)
    # half a step of the rounding, plus |y| / 32768 because read_wav divides by 32768 where write_wav multiplies by 32767: within
    # 1 / 32767 up to half of full scale.  Near full scale that flat bound cannot hold for any rounding of y * 32767
    # (y = 32766.49 / 32767 is stored as 32766 and read as 0.99994, 4.6e-5 = 1.5 / 32767 away), so the sum is asserted per sample.
    clipped = np.clip(y.astype(np.float64), -1, 1)
    err = np.abs(back[:, 0].astype(np.float64) - clipped)
    assert (err <= 0.5 / 32767 + np.abs(clipped) / 32768 + 1e-9).all()
    assert err[np.abs(clipped) <= 0.5].max() <= 1 / 32767 and (np.abs(clipped) <= 0.5).sum() > 2000
    assert np.array_equal(np.frombuffer(raw[44:], "<i2"), np.clip(np.round(y.astype(np.float64) * 32767), -32768, 32767).astype(np.int16))
    audio.write_wav(tmp_path / "z.wav", torch.from_numpy(y[:10]).double().numpy(), 16000)
    assert audio.read_wav(tmp_path / "z.wav")[0].shape == (10, 1)


def test_synthetic_batch_is_deterministic_and_bounded():
    a = render.synthetic_batch(np.random.default_rng(5), 4, DEFAULT_CONFIG, device="cpu")
    b = render.synthetic_batch(np.random.default_rng(5), 4, DEFAULT_CONFIG, device="cpu")
    c = render.synthetic_batch(np.random.default_rng(6), 4, DEFAULT_CONFIG, device="cpu")
    fs, seconds = DEFAULT_CONFIG["model"]["sample_rate"], DEFAULT_CONFIG["dataset"]["segment_duration"]
    assert a.input_waveform.shape == (4, fs * seconds) and a.input_waveform.dtype == torch.float32 and not a.input_waveform.is_cuda
    assert torch.equal(a.input_waveform, b.input_waveform) and not torch.equal(a.input_waveform, c.input_waveform)
    assert a.cond_index.shape == (4, 2) and a.cond_index.dtype == torch.long and not a.cond_index.any()
    assert len(a.notes_batch) == 4 and all(np.array_equal(x, y) for x, y in zip(a.notes_batch, b.notes_batch))
    assert torch.equal(a.input_waveform.abs().amax(dim=1), torch.ones(4))
    assert np.array_equal(a.input_waveform.numpy(), render.render_batch_host(a.notes_batch, fs, fs * seconds, normalize=True))
    rng = np.random.default_rng(0)
    counts = []
    for _ in range(400):
        n = render.synthetic_notes(rng, 3.0)
        counts.append(len(n))
        assert n.dtype == np.float64 and n.shape[1] == 4 and (np.diff(n[:, 0]) >= 0).all()
        assert n[:, 0].min() >= 0 and n[:, 1].max() <= 3.0 and (n[:, 1] - n[:, 0] > 0).all() and (n[:, 1] - n[:, 0]).max() <= 1.0 + 1e-12
        assert 21 <= n[:, 2].min() and n[:, 2].max() <= 108 and 1 <= n[:, 3].min() and n[:, 3].max() <= 127
    assert min(counts) >= 1 and max(counts) <= 90 and min(counts) <= 3 and max(counts) >= 88
    # the documented order of the draws
    rng, ref = np.random.default_rng(7), np.random.default_rng(7)
    n = int(ref.integers(1, 91))
    onset, length, pitch = ref.uniform(0.0, 3.0, n), ref.uniform(0.05, 1.0, n), ref.integers(21, 109, n)
    got = render.synthetic_notes(rng, 3.0)
    assert np.array_equal(got[:, 0], np.sort(onset)) and np.array_equal(got[:, 2], pitch[np.argsort(onset, kind="stable")])
