"""GPU: the device ingest (music2midi_amd/ingest.py, csrc/ingest.hip) against the host functions of music2midi_amd/audio.py.

Every comparison is np.array_equal, on the bit patterns where signed zeros and denormals matter: the kernels repeat the host's
rounded operations in the host's order (one fp32 accumulator per output, taps in ascending input index, multiply then add), so
any difference is a kernel bug - tap order, contraction or an index - and not noise.

The resampler's tile is 256 outputs per workgroup (IG_TILE in csrc/ingest.hip); a tile's inputs are staged in LDS when they fit
8192 floats, which for up = 1 holds up to down = 29 and fails from down = 30: both sides of that threshold are cases below."""
import copy
import struct

import numpy as np
import pytest
import torch

from music2midi_amd import audio, ingest, native, synth
from music2midi_amd.checkpoint import load_t5_state
from music2midi_amd.config import DEFAULT_CONFIG, T5Geometry

from wav_fixtures import sample_bodies, wav_bytes

pytestmark = pytest.mark.gpu

TILE = 256
# (orig rate, target rate) -> up / down
RATES = {"160/441": (441, 160), "1/3": (3, 1), "320/441": (441, 320), "1/2": (2, 1), "2/1": (1, 2), "640/441": (441, 640),
         "1/6": (6, 1), "1/1": (1, 1), "1/29": (29, 1), "1/30": (30, 1)}


def _signal(T, seed, sr=44100):
    """tests/test_augment_gpu.py's well-conditioned signal: noise plus two sines."""
    t = np.arange(T) / sr
    y = 0.25 * np.random.default_rng(seed).standard_normal(T) + 0.2 * np.sin(2 * np.pi * 440 * t) + 0.15 * np.sin(2 * np.pi * 1318.5 * t)
    return y.astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _lengths_for_outputs(up, down, counts):
    """The longest input that gives exactly c outputs, for every c."""
    return [c * down // up for c in counts if -(-(c * down // up) * up // down) == c and c * down // up >= 1]


# ------------------------------------------------------------------ resampler
@pytest.mark.parametrize("name", list(RATES))
def test_resampler_tap_bounds(name):
    orig, target = RATES[name]
    up, down = (int(v) for v in name.split("/"))
    assert (up, down) == ((1, 1) if orig == target else ingest.ratio(orig, target))
    lengths = [1, 7, 100] + _lengths_for_outputs(up, down, [TILE - 1, TILE, TILE + 1, 2 * TILE + 1]) + [48017, 132300]
    if name == "160/441":
        assert lengths[3:7] == [702, 705, 708, 1413]
    for n in lengths:
        y = _signal(n, n)
        want = audio.resample(y, orig, target)
        got = ingest.resample_device(torch.from_numpy(y).cuda(), orig, target).cpu().numpy()
        assert got.dtype == np.float32 and got.shape == want.shape, (name, n)
        bad = np.flatnonzero(_bits(got) != _bits(want))
        assert not len(bad), f"{name}, {n} samples: {len(bad)} of {len(want)} outputs differ, first at {bad[0]}: {got[bad[0]]!r} != {want[bad[0]]!r}"


def test_resampler_64_bit_indices():
    """1000 Hz -> 999 Hz: up 999, down 1000, 20 001 taps; over 2 200 000 samples m * up and n * down pass 2^31 near the end."""
    n = 2_200_000
    assert ingest.ratio(1000, 999) == (999, 1000) and (n - 1) * 999 > 1 << 31
    y = _signal(n, 5)
    want = audio.resample(y, 1000, 999)
    got = ingest.resample_device(torch.from_numpy(y).cuda(), 1000, 999).cpu().numpy()
    assert got.shape == want.shape == (2_197_800,)
    assert np.array_equal(_bits(got[-10000:]), _bits(want[-10000:]))
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("name", ["160/441", "1/30", "1/1"])
def test_zero_fill_up_to_the_capacity_and_nothing_beyond(name):
    """The launch writes [0, capacity) - the signal, then exact zeros - and not one float on either side of it."""
    orig, target = RATES[name]
    up, down = (int(v) for v in name.split("/"))
    y = _signal(3001, 2)
    want = audio.resample(y, orig, target)
    capacity, guard = -(-len(want) // 1000) * 1000 + 1000, 512                  # padding that spans whole tiles and a partial one
    x = torch.from_numpy(y).cuda()
    buf = torch.full((guard + capacity + guard,), float("nan"), dtype=torch.float32, device="cuda")
    out = buf[guard:guard + capacity]
    hp = None if up == down else ingest._filter_on(x.device, up, down)
    native.check(native.load().m2m_ingest_resample_f32(x.data_ptr(), len(y), up, down, None if hp is None else hp.data_ptr(),
                                                       10 * max(up, down), out.data_ptr(), capacity, native.stream_handle(x.device)),
                 "m2m_ingest_resample_f32")
    host = buf.cpu().numpy()
    assert np.isnan(host[:guard]).all() and np.isnan(host[guard + capacity:]).all()
    assert np.array_equal(_bits(host[guard:guard + len(want)]), _bits(want))
    assert np.array_equal(_bits(host[guard + len(want):guard + capacity]), np.zeros(capacity - len(want), np.uint32))
    # the same through the public call: padded to the next multiple of pad_to
    got = ingest.resample_device(x, orig, target, pad_to=1000).cpu().numpy()
    assert len(got) == -(-len(want) // 1000) * 1000 and np.array_equal(_bits(got[:len(want)]), _bits(want)) and not got[len(want):].any()


def test_equal_rates_return_the_signal():
    x = torch.from_numpy(_signal(1000, 1)).cuda()
    assert ingest.resample_device(x, 16000, 16000) is x
    assert torch.equal(ingest.resample_device(x, 16000.0, 16000.000001), x)      # up / down = 1 / 1 after limit_denominator: a copy


def test_resample_enqueues_on_the_current_stream_without_synchronising():
    """The call can be captured into a graph - a synchronisation or a launch on another stream would end the capture with an
    error - and the replay computes the same samples from new input."""
    y0, y1 = _signal(5000, 7), _signal(5000, 8)
    x = torch.from_numpy(y0).cuda()
    ingest.resample_device(x, 44100, 16000)                                       # the filter is designed and uploaded once, here
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ingest.resample_device(x, 44100, 16000, pad_to=2000)
    x.copy_(torch.from_numpy(y1).cuda())
    graph.replay()
    want = audio.resample(y1, 44100, 16000)
    got = out.cpu().numpy()
    assert np.array_equal(_bits(got[:len(want)]), _bits(want)) and not got[len(want):].any()


# ------------------------------------------------------------------ PCM decode + downmix
@pytest.mark.parametrize("n_ch", [1, 2, 3, 7])
def test_pcm_decode_and_downmix(tmp_path, n_ch):
    """Every format: the extremes, a partial trailing frame, a data chunk at an offset that is 2 mod 4 (a 6-byte LIST chunk
    before it), and the sample bytes at a device address that is no multiple of the sample width."""
    frames = 1003
    for kind, (tag, bits, body, _) in sample_bodies(n_ch, frames, seed=n_ch).items():
        width = bits // 8
        p = tmp_path / f"{kind}.wav"
        p.write_bytes(wav_bytes(tag, n_ch, 8000, bits, body + b"\x7f" * (n_ch * width - 1),
                                before_data=b"LIST" + struct.pack("<I", 6) + b"INFOab"))
        assert audio.wav_layout(p, p.read_bytes()).data_offset % 4 == 2
        want = audio.read_wav(p)[0].mean(axis=1)
        assert want.dtype == np.float32 and want.shape == (frames,)
        got = ingest.load_audio_device(p, 8000).cpu().numpy()
        assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), (kind, n_ch)
        for shift in (0, 1, 2):                                                   # byte-wise reads when the address is not aligned
            dev = torch.from_numpy(np.frombuffer(b"\x00" * shift + body, np.uint8).copy()).cuda()
            got = ingest.decode_pcm_device(dev[shift:], frames, n_ch, kind).cpu().numpy()
            assert np.array_equal(_bits(got), _bits(want)), (kind, n_ch, shift)


# ------------------------------------------------------------------ files
def _write(tmp_path, name, kind, n_ch, rate, seconds, seed):
    y = _signal(int(rate * seconds), seed, rate) * 0.9
    chans = np.stack([y * (0.5 + 0.5 * c) for c in range(n_ch)], axis=1).clip(-1, 1)
    if kind == "s16":
        tag, bits, body = 1, 16, np.round(chans * 32767).astype("<i2").tobytes()
    elif kind == "s24":
        v = np.round(chans.astype(np.float64) * 8388607).astype(np.int32)
        tag, bits, body = 1, 24, (v & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    else:
        tag, bits, body = 3, 32, chans.astype("<f4").tobytes()
    p = tmp_path / name
    p.write_bytes(wav_bytes(tag, n_ch, rate, bits, body))
    return p


@pytest.mark.parametrize("kind,n_ch,rate", [("s16", 2, 44100), ("s24", 1, 48000)])
def test_load_audio_device_is_load_audio(tmp_path, kind, n_ch, rate):
    p = _write(tmp_path, "clip.wav", kind, n_ch, rate, 2.0, 11)
    mono = audio.read_wav(p)[0].mean(axis=1)
    for sr in (16000, 22050):
        want = audio.load_audio(p, sr)
        got = ingest.load_audio_device(p, sr)
        assert got.is_cuda and got.dtype == torch.float32
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (kind, sr)
        part = audio.resample(mono[int(0.5 * rate):int(0.5 * rate) + int(1.0 * rate)], rate, sr)
        got = ingest.load_audio_device(p, sr, offset=0.5, duration=1.0).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(part)), (kind, sr, "slice")
        got = ingest.load_audio_device(p, sr, offset=1.5, duration=9.0, pad_to=4096).cpu().numpy()      # a duration past the end
        tail = audio.resample(mono[int(1.5 * rate):], rate, sr)
        assert len(got) == -(-len(tail) // 4096) * 4096 and np.array_equal(_bits(got[:len(tail)]), _bits(tail)) and not got[len(tail):].any()
    assert len(ingest.load_audio_device(p, 16000, offset=5.0)) == 0


# ------------------------------------------------------------------ through the model
@pytest.fixture(scope="module")
def model():
    from music2midi_amd.model import Music2MIDI
    geom = T5Geometry(DEFAULT_CONFIG["model"]["t5"])
    sd = synth.t5_state_dict(geom, seed=0)
    synth.perturb_layer_norms(sd, 0)
    synth.force_eos_head(sd, geom, active=340, eos_scale=1.6)
    m = Music2MIDI(copy.deepcopy(DEFAULT_CONFIG))
    load_t5_state(m.model, sd, strict=False)
    return m.cuda().eval()


def _float_stereo_file(tmp_path, n_ch=2):
    """The file of tests/test_callers_gpu.py::test_generate_from_a_float_wav_file (with n_ch copies of the channel)."""
    sr_in = 44100
    y = synth.waveform(5, sr_in * 2) * 0.5
    body = np.stack([y] * n_ch, axis=1).astype("<f4").tobytes()
    p = tmp_path / f"clip{n_ch}.wav"
    p.write_bytes(wav_bytes(3, n_ch, sr_in, 32, body))
    return p


def test_generate_through_the_device_ingest(tmp_path, model, monkeypatch):
    m = model
    p, p8 = _float_stereo_file(tmp_path), _float_stereo_file(tmp_path, 8)
    calls = []
    real = ingest.load_audio_device
    monkeypatch.setattr(ingest, "load_audio_device", lambda *a, **k: (calls.append(a[0]), real(*a, **k))[1])
    want = m.generate_notes(audio_y=audio.load_audio(p, 16000), cond_index=[1, 0])
    assert "device_ingest" not in m.config.inference
    assert np.array_equal(m.generate_notes(audio_path=p, cond_index=[1, 0]), want) and not calls        # the key is off: the host path
    m.config.inference.device_ingest = True
    try:
        padded, seg = m._padded_segments(p, None, None)
        host = audio.load_audio(p, 16000)
        assert calls == [p] and padded.is_cuda and padded.shape == (seg,) and seg == 48000
        assert np.array_equal(_bits(padded[:len(host)].cpu().numpy()), _bits(host)) and not padded[len(host):].any()
        assert np.array_equal(m.generate_notes(audio_path=p, cond_index=[1, 0]), want) and calls == [p, p]
        # the decoded ids as well: the notes of a random-init model can be few
        rows, rows_host = m.sample_token_rows(padded, seg, [1, 0]), m.sample_token_rows(m._padded_segments(None, host, None)[0], seg, [1, 0])
        assert len(rows) == 1 and rows[0].numel() >= 2 and torch.equal(rows[0], rows_host[0])
        assert np.array_equal(m.generate_notes(audio_y=host, cond_index=[1, 0]), want) and calls == [p, p]   # an array: the host path
        # 8 channels: not eligible, the host's notes through the host path
        want8 = m.generate_notes(audio_y=audio.load_audio(p8, 16000), cond_index=[1, 0])
        assert np.array_equal(m.generate_notes(audio_path=p8, cond_index=[1, 0]), want8) and calls == [p, p]
    finally:
        del m.config.inference["device_ingest"]


def test_ingest_on_a_side_stream_before_generate(tmp_path, model):
    """The ingest's kernels run on torch's current stream: enqueued on a side stream and joined by an event wait, they feed the
    same decode as on the default stream."""
    m = model
    p = _float_stereo_file(tmp_path)
    seg = m._segment_length()
    want = m.sample_token_rows(ingest.load_audio_device(p, 16000, pad_to=seg), seg, [1, 0])
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        padded = ingest.load_audio_device(p, 16000, pad_to=seg)
        done = torch.cuda.Event()
        done.record(side)
    torch.cuda.current_stream().wait_event(done)
    padded.record_stream(torch.cuda.current_stream())
    got = m.sample_token_rows(padded, seg, [1, 0])
    assert len(got) == len(want) == 1 and want[0].numel() >= 2 and torch.equal(got[0], want[0])
