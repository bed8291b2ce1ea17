"""CPU: the host side of the device ingest (music2midi_amd/ingest.py, csrc/ingest.hip) - the length formula, the refusals the library
makes on its arguments alone, read_wav on top of the shared header parser, eligibility, and the fall-back to the host path."""
import copy
import ctypes as C
import struct

import numpy as np
import pytest
import torch

from music2midi_amd import audio, ingest, native
from music2midi_amd.config import DEFAULT_CONFIG

from wav_fixtures import sample_bodies, wav_bytes

# up / down of 44.1k, 48k, 22.05k, 32k, 8k, 11.025k -> 16k and 44.1k -> 22.05k
RATIOS = [(160, 441), (1, 3), (320, 441), (1, 2), (2, 1), (640, 441), (1, 2)]
M2M_ERR_INVALID = -1


# ------------------------------------------------------------------ the library's host arithmetic
def test_resampled_length_is_resample_polys():
    from scipy.signal import resample_poly
    lib = native.load()
    for up, down in RATIOS + [(999, 1000), (1, 6), (1, 1)]:
        for n in (1, 2, 7, 100, 440, 441, 442, 48017, 132300):
            want = len(resample_poly(np.zeros(n, np.float32), up, down))
            assert lib.m2m_ingest_resampled_length(n, up, down) == want == ingest.resampled_length(n, up, down), (n, up, down)
    assert lib.m2m_ingest_resampled_length(0, 1, 3) == 0
    assert lib.m2m_ingest_resampled_length(1 << 28, 1000, 1) == 1000 << 28          # past int32 and past uint32
    for bad in ((-1, 1, 1), ((1 << 28) + 1, 1, 1), (5, 0, 1), (5, 1, 0), (5, 1001, 1), (5, 1, 1001)):
        assert lib.m2m_ingest_resampled_length(*bad) == M2M_ERR_INVALID


def test_phase_major_filter_layout():
    """Row p of the layout the kernel reads is h[p], h[p + up], ... reversed, zero-filled: every tap appears exactly once."""
    lib = native.load()
    for up, down in [(160, 441), (2, 1), (1, 3), (999, 1000), (640, 441)]:
        h = ingest.design_filter(up, down)
        half = 10 * max(up, down)
        assert h.dtype == np.float32 and len(h) == 2 * half + 1
        hp = ingest.phase_major(h, up)
        J = lib.m2m_ingest_phase_taps(up, down)
        assert hp.shape == (up, J) and hp.flags.c_contiguous
        for p in sorted({0, min(1, up - 1), up // 2, up - 1}):
            want = h[p::up][::-1]
            assert np.array_equal(hp[p, J - len(want):], want) and not hp[p, :J - len(want)].any()
    assert lib.m2m_ingest_phase_taps(0, 1) == M2M_ERR_INVALID


def test_filter_is_the_one_resample_poly_builds(monkeypatch):
    """The filter resample_poly hands to upfirdn for fp32 input (behind down - half % down zeros that centre it), bit for bit."""
    import scipy.signal._signaltools as st
    seen = []
    real = st.upfirdn
    monkeypatch.setattr(st, "upfirdn", lambda h, x, up, down, **kw: (seen.append(np.array(h)), real(h, x, up, down, **kw))[1])
    x = np.random.default_rng(1).standard_normal(3000).astype(np.float32)
    for up, down in RATIOS + [(999, 1000), (1, 6)]:
        del seen[:]
        st.resample_poly(x, up, down)
        h = ingest.design_filter(up, down)
        lead = down - (10 * max(up, down)) % down
        assert seen[0].dtype == np.float32 and not seen[0][:lead].any()
        assert np.array_equal(seen[0][lead:lead + len(h)].view(np.uint32), h.view(np.uint32)), (up, down)


def test_every_refusal_is_made_without_a_gpu():
    """M2M_ERR_INVALID on the arguments alone: the pointers are never dereferenced, no HIP call is made."""
    lib = native.load()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    x, out = a, a + 4096                                                            # never touched: only compared
    pcm = lib.m2m_ingest_pcm
    for frames, ch, fmt, src, dst in [(0, 2, 1, x, out), ((1 << 28) + 1, 2, 1, x, out), (10, 0, 1, x, out), (10, 8, 1, x, out),
                                      (10, 2, 6, x, out), (10, 2, -1, x, out), (10, 2, 1, None, out), (10, 2, 1, x, None),
                                      (10, 2, 1, x, x + 16), (10, 2, 1, x + 39, x), (10, 1, 5, x, x + 79)]:
        assert pcm(src, frames, ch, fmt, dst, None) == M2M_ERR_INVALID, (frames, ch, fmt)
        assert native.load().m2m_last_error()
    rs = lib.m2m_ingest_resample_f32
    h = a + 8192
    ok = dict(x=x, n=100, up=160, down=441, h=h, half=4410, out=out, cap=37)
    for change in [dict(n=0), dict(n=(1 << 28) + 1), dict(up=0), dict(up=1001), dict(down=0), dict(down=1001), dict(up=320, down=882, half=8820),
                   dict(half=4409), dict(half=1600), dict(cap=36), dict(cap=(1 << 30) + 1), dict(x=None), dict(h=None), dict(out=None),
                   dict(out=x + 396), dict(out=x - 144), dict(up=1, down=1, half=10, cap=99)]:
        k = dict(ok, **change)
        assert rs(k["x"], k["n"], k["up"], k["down"], k["h"], k["half"], k["out"], k["cap"], None) == M2M_ERR_INVALID, change


# ------------------------------------------------------------------ read_wav on the shared header parser
@pytest.mark.parametrize("n_ch", [1, 2, 3])
def test_read_wav_returns_the_same_arrays(tmp_path, n_ch):
    for kind, (tag, bits, body, want) in sample_bodies(n_ch, 57).items():
        p = tmp_path / f"{kind}.wav"
        p.write_bytes(wav_bytes(tag, n_ch, 22050, bits, body + b"\x01" * (n_ch * (bits // 8) - 1)))       # a partial trailing frame
        y, rate = audio.read_wav(p)
        assert rate == 22050 and y.dtype == np.float32 and y.shape == (57, n_ch)
        assert np.array_equal(y.view(np.uint32), want.view(np.uint32)), kind
        lay = audio.wav_layout(p, p.read_bytes())
        assert (lay.n_ch, lay.rate, lay.bits) == (n_ch, 22050, bits) and audio.wav_sample_format(p, lay.tag, lay.bits) == kind
        assert p.read_bytes()[lay.data_offset:lay.data_offset + lay.data_size].startswith(body)


def test_read_wav_chunk_walk_and_errors(tmp_path):
    tag, bits, body, want = sample_bodies(2, 20)["s16"]
    p = tmp_path / "a.wav"
    p.write_bytes(wav_bytes(tag, 2, 8000, bits, body, before_data=b"LIST" + struct.pack("<I", 6) + b"INFOab", extensible=True))
    assert audio.wav_layout(p, p.read_bytes()).data_offset % 4 == 2
    assert np.array_equal(audio.read_wav(p)[0], want)
    raw = wav_bytes(tag, 2, 8000, bits, body)
    p.write_bytes(raw[:-10])                                                        # a data chunk longer than the file: clipped
    assert np.array_equal(audio.read_wav(p)[0], want[:-3])
    for name, content, message in [
            ("b.wav", b"ID3\x04" + b"\x00" * 40, "not a RIFF/WAVE file (compressed formats need librosa/ffmpeg, which are not installed)"),
            ("c.wav", raw[:12] + raw[36:], "missing 'fmt ' or 'data' chunk"),
            ("d.wav", wav_bytes(1, 0, 8000, 16, body), "bad channel count / sample rate"),
            ("e.wav", wav_bytes(1, 1, 8000, 40, body), "unsupported PCM sample width 40 bits"),
            ("f.wav", wav_bytes(3, 1, 8000, 16, body), "unsupported float sample width 16 bits"),
            ("g.wav", wav_bytes(6, 1, 8000, 8, body), "unsupported WAVE format tag 6 (only PCM and IEEE float)")]:
        q = tmp_path / name
        q.write_bytes(content)
        with pytest.raises(ValueError) as e:
            audio.read_wav(q)
        assert str(e.value) == f"{q}: {message}"


# ------------------------------------------------------------------ eligibility and the fall-back
def test_eligible(tmp_path):
    tag, bits, body, _ = sample_bodies(8, 30)["s16"]
    files = {"ok.wav": wav_bytes(1, 2, 44100, 16, body), "eight.wav": wav_bytes(1, 8, 44100, 16, body),
             "alaw.wav": wav_bytes(6, 1, 8000, 8, body), "seven.wav": wav_bytes(1, 7, 44100, 16, body),
             "mp3.wav": b"ID3\x04" + b"\x00" * 64, "empty.wav": b"", "slow.wav": wav_bytes(1, 1, 7, 16, body)}
    for name, content in files.items():
        (tmp_path / name).write_bytes(content)
    assert ingest.eligible(tmp_path / "ok.wav") and ingest.eligible(tmp_path / "ok.wav", 16000) and ingest.eligible(tmp_path / "seven.wav")
    for name in ("eight.wav", "alaw.wav", "mp3.wav", "empty.wav", "missing.wav"):
        assert not ingest.eligible(tmp_path / name), name
    assert ingest.eligible(tmp_path / "slow.wav") and not ingest.eligible(tmp_path / "slow.wav", 16000)     # 16000 / 7: up > 1000
    assert ingest.ratio(44100, 16000) == (160, 441) and ingest.ratio(1000, 999) == (999, 1000)
    with pytest.raises(ValueError, match="8 channels"):
        ingest.load_audio_device(tmp_path / "eight.wav", 16000, device="cuda:0")
    with pytest.raises(ValueError, match="not on cpu"):
        ingest.load_audio_device(tmp_path / "ok.wav", 16000, device="cpu")


def test_padded_segments_stays_on_the_host_without_the_key_or_a_gpu(tmp_path, monkeypatch):
    from music2midi_amd.model import Music2MIDI

    def boom(*a, **k):
        raise AssertionError("load_audio_device was called")
    monkeypatch.setattr(ingest, "load_audio_device", boom)
    tag, bits, body, _ = sample_bodies(2, 4410)["s16"]
    p = tmp_path / "clip.wav"
    p.write_bytes(wav_bytes(tag, 2, 44100, bits, body))
    want = audio.load_audio(p, 16000)
    m = Music2MIDI(copy.deepcopy(DEFAULT_CONFIG))
    assert "device_ingest" not in m.config.inference
    for key in (None, True):                                                        # absent; set, but the model is on the CPU
        if key:
            m.config.inference.device_ingest = True
        padded, seg = m._padded_segments(p, None, None)
        assert seg == 48000 and padded.shape == (48000,) and padded.device.type == "cpu"
        assert np.array_equal(padded[:len(want)].numpy(), want) and not padded[len(want):].any()
    # with the key, a GPU model and an array: still the host (pretend the model is on a GPU - nothing is launched)
    monkeypatch.setattr(Music2MIDI, "device", property(lambda self: torch.device("cuda", 0)))
    assert m._device_ingest(p, None) and not m._device_ingest(p, want) and not m._device_ingest(None, want)
    m.config.inference.device_ingest = False
    assert not m._device_ingest(p, None)
