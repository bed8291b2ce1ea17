"""GPU: the note renderer's kernel (csrc/render.hip) and the device side of music2midi_amd/render.py against render_host, the
definition.  Every comparison is np.array_equal on the samples (and on their bit patterns where a signed zero could hide): the
kernel repeats the definition's integer arithmetic and its rounded fp32 operations in its order, so any difference is a kernel bug -
a contraction, a tile bound, an integer width - and not noise."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from music2midi_amd import native, render
from music2midi_amd.config import DEFAULT_CONFIG
from music2midi_amd.utils import numpy_to_midi

from render_cases import POLY_FS, POLY_SAMPLES, poly_batch, random_notes, records, voice_struct

pytestmark = pytest.mark.gpu

RATES = (16000, 48000)


def _tile():
    return render.tile_size()


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).view(np.uint32)


def _check(notes, fs, n_samples, voice=None, normalize=False):
    """render == render_host for one clip; returns the host samples."""
    want = render.render_host(notes, fs, n_samples, voice, normalize)
    got = render.render(notes, fs, n_samples, voice, normalize)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == want.shape
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert not len(bad), f"{len(bad)} of {len(want)} samples differ, first at {bad[0]}: {got[int(bad[0])].item()!r} != {want[bad[0]]!r}"
    return want


# ------------------------------------------------------------------ every wavetable
@pytest.mark.parametrize("fs", RATES)
def test_one_note_per_wavetable(fs):
    v = render.default_voice(fs)
    audible = np.flatnonzero(~v.silent)
    pitches = [int(audible[v.table[audible] == m][0]) for m in range(1, 7)] + [0, int(audible[-1])]
    assert sorted({int(v.table[p]) for p in pitches}) == [1, 2, 3, 4, 5, 6] and len(pitches) == 8
    for p in pitches:
        y = _check(np.array([[0.01, 0.12, p, 100]]), fs, int(0.2 * fs))
        assert y.any(), p
    if v.silent.any():
        assert not _check(np.array([[0.01, 0.12, int(np.flatnonzero(v.silent)[0]), 100]]), fs, 4000).any()


# ------------------------------------------------------------------ tile boundaries
def test_notes_at_tile_edges():
    fs, T = 16000, _tile()
    R = render.default_voice(fs).release
    assert R < T or R % T                                                                   # a release ends inside a tile
    n = 4 * T
    for on in (T - 1, T, T + 1):
        for off in (2 * T - 1, 2 * T, 2 * T + 1):
            y = _check(np.array([[on / fs, off / fs, 64, 90]]), fs, n)
            assert not y[:on + 1].any() and y[on + 1] != 0 and not y[off + R:].any()           # sample `on` itself is phase 0: zero
    # a release that crosses a tile edge: off + R / 2 is the edge
    _check(np.array([[0.001, (2 * T - R // 2) / fs, 57, 127]]), fs, n)


def test_clip_lengths_around_a_tile():
    fs, T = 16000, _tile()
    for n in (1, T - 1, T, T + 1):
        y = _check(np.array([[0.0, 10.0, 60, 100], [(n - 1) / fs, 10.0, 72, 100], [(T // 2) / fs, 10.0, 48, 100]]), fs, n)   # all cut by the end
        assert len(y) == n and (n == 1 or y.any())
    assert _check(np.array([[0.0, 1.0, 60, 100]]), 48000, 1)[0] == 0.0                      # sample 0 of a note: phase 0


# ------------------------------------------------------------------ edge notes
def test_edge_notes():
    fs, T = 16000, _tile()
    v = render.default_voice(fs)
    n = 2 * T + 77
    short = np.array([[0.01, 0.01 + (v.attack // 2) / fs, 69, 100]])                        # shorter than the attack
    assert short[0, 1] > short[0, 0]
    _check(short, fs, n)
    y = _check(np.array([[-0.3, 0.05, 62, 80]]), fs, n)                                     # already sounding at sample 0
    assert y[0] != 0
    y = _check(np.array([[-(1 << 30) / fs + 1.0, 0.05, 62, 80]]), fs, n)                    # from (almost) the earliest onset there is
    assert y.shape == (n,)
    outside = np.array([[5.0, 6.0, 60, 80], [-2.0, -1.0, 60, 80]])                          # wholly behind and wholly before the clip
    assert not _check(outside, fs, n).any()
    twice = np.array([[0.02, 0.1, 60, 80], [0.02, 0.1, 60, 80]])
    y2, y1 = _check(twice, fs, n), _check(twice[:1], fs, n)
    assert np.array_equal(y2, y1 + y1)
    got = render.render(np.zeros((0, 4)), fs, n)
    assert got.shape == (n,) and np.array_equal(_bits(got), np.zeros(n, np.uint32))
    assert render.render(np.zeros((0, 4)), fs).shape == (0,)


# ------------------------------------------------------------------ integer widths
def test_decay_product_passes_32_bits():
    """tau = 1 ms at 16 kHz: dec = 64 / 16 * 65536 = 2^18, so k * dec passes 2^32 at k = 16384, inside a 2 s note.  A 32-bit
    product would fall back to j = 0 there and sound again; the definition stays at the table's last entry."""
    fs = 16000
    v = render.Voice(fs, tau=(0.0, 24.0, 0.001), decay_steps=512)
    assert int(v.dec[60]) == 1 << 18 and 32000 * int(v.dec[60]) > 1 << 32
    y = _check(np.array([[0.0, 2.0, 60, 127]]), fs, 34000, voice=v)
    assert np.abs(y[16384:16484]).max() < 1e-3 < np.abs(y[:100]).max()
    # the same with a table long enough that the product's high bits pick the entry: j = 4 k runs to 131072
    v = render.Voice(fs, tau=(0.0, 24.0, 0.001), decay_steps=140000)
    _check(np.array([[0.0, 2.0, 60, 127]]), fs, 34000, voice=v)


def test_phase_wraps_and_decay_runs_off_the_table():
    fs = 48000
    v = render.default_voice(fs)
    p = 108                                                                                 # 4186 Hz: the phase wraps 4186 times a second
    assert 96000 * int(v.inc[p]) > 8000 << 32
    _check(np.array([[0.0, 2.0, p, 100]]), fs, 98000)
    short = render.Voice(fs, decay_steps=8)                                                 # j reaches 8 within 8 * 65536 / dec samples
    k_end = 8 * 65536 // int(short.dec[60]) + 1
    assert k_end < 40000
    y = _check(np.array([[0.0, 1.0, 60, 100]]), fs, 48000, voice=short)
    assert y[k_end:].any()                                                                  # held at the last entry, not silenced
    small = render.Voice(fs, table_size=256, harmonics=2, attack=0.0, release=0.0)         # the smallest table, A = R = 1
    assert (small.attack, small.release, small.shift) == (1, 1, 24)
    _check(np.array([[0.0, 0.5, 60, 100], [0.1, 0.3, 100, 50]]), fs, 30000, voice=small)


# ------------------------------------------------------------------ polyphony, batches, bounds
@pytest.fixture(scope="module")
def poly():
    batch = poly_batch()
    return batch, render.render_batch_host(batch, POLY_FS, POLY_SAMPLES)


def test_polyphony_in_a_strided_batch_with_canaries(poly):
    """300 notes over 3 s at 48 kHz, an empty clip and a third one in ONE launch, into rows with a gap between them: NaN before
    the buffer, behind it and in the gaps stays NaN."""
    batch, want = poly
    B, n, stride, guard = 3, POLY_SAMPLES, POLY_SAMPLES + 37, 512
    buf = torch.full((guard + B * stride + guard,), float("nan"), dtype=torch.float32, device="cuda")
    out = buf[guard:guard + B * stride].view(B, stride)[:, :n]
    assert out.stride(0) == stride > n
    voice = render.default_voice(POLY_FS)
    words, counts = render.device_lists([render.pack(x, POLY_FS, n, voice) for x in batch], n, voice)
    render.launch(torch.from_numpy(words).cuda(), counts, voice, out)
    host = buf.cpu().numpy()
    assert np.isnan(host[:guard]).all() and np.isnan(host[guard + B * stride:]).all()
    rows = host[guard:guard + B * stride].reshape(B, stride)
    assert np.isnan(rows[:, n:]).all()
    for b in range(B):
        bad = np.flatnonzero(_bits(rows[b, :n]) != _bits(want[b]))
        assert not len(bad), f"clip {b}: {len(bad)} samples differ, first at {bad[0]}"
    assert np.array_equal(_bits(rows[1, :n]), np.zeros(n, np.uint32)) and np.abs(want[0]).max() > 0.5
    assert np.array_equal(_bits(render.render(batch, POLY_FS, n)), _bits(want))            # contiguous rows, the same launch shape


def _direct(batch, fs, n, voice):
    """The C entry on lists uploaded beforehand: (launch(), out)."""
    dev = torch.device("cuda", torch.cuda.current_device())
    packed = [render.pack(x, fs, n, voice) for x in batch]
    start, entries = render.tile_lists(packed, n, _tile(), voice.release)
    rec = torch.from_numpy(records(packed, voice, n)).to(dev)
    start_d, entries_d = torch.from_numpy(start).to(dev), torch.from_numpy(entries).to(dev)
    wave, decay = voice.on_device(dev)
    vs = voice_struct(voice, wave.data_ptr(), decay.data_ptr())
    out = torch.full((len(batch), n), float("nan"), dtype=torch.float32, device=dev)
    lib = native.load()
    keep = (rec, start_d, entries_d, wave, decay)

    def launch():
        assert keep is not None
        native.check(lib.m2m_render_notes_f32(rec.data_ptr(), rec.shape[0], start_d.data_ptr(), entries_d.data_ptr(), len(entries), C.byref(vs),
                                              out.data_ptr(), n, out.stride(0), len(batch), native.stream_handle(dev)), "m2m_render_notes_f32")
    return launch, out


def test_graph_capture_and_side_stream(poly):
    batch, want = poly
    voice = render.default_voice(POLY_FS)
    launch, out = _direct(batch, POLY_FS, POLY_SAMPLES, voice)
    launch()                                                                                # warm: the code object is loaded
    assert np.array_equal(_bits(out), _bits(want))
    side = torch.cuda.Stream()
    out.fill_(float("nan"))
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        launch()
    assert torch.isnan(out).all()                                                           # captured, not run
    graph.replay()
    assert np.array_equal(_bits(out), _bits(want))
    # render() on a side stream, joined by an event
    side2 = torch.cuda.Stream()
    side2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side2):
        got = render.render(batch, POLY_FS, POLY_SAMPLES)
        done = torch.cuda.Event()
        done.record(side2)
    torch.cuda.current_stream().wait_event(done)
    got.record_stream(torch.cuda.current_stream())
    assert np.array_equal(_bits(got), _bits(want))


def test_normalize(poly):
    batch, _ = poly
    want = render.render_batch_host(batch, POLY_FS, POLY_SAMPLES, normalize=True)
    got = render.render(batch, POLY_FS, POLY_SAMPLES, normalize=True)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.abs(want[0]).max() == 1.0 == np.abs(want[2]).max() and not want[1].any()
    _check(batch[2], POLY_FS, None, normalize=True)                                         # one clip, the default length


# ------------------------------------------------------------------ end to end
def _small_config():
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["model"]["t5"].update(d_model=128, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2)
    cfg["trainer"].update(log_every_n_steps=1000)
    return cfg


def test_generate_audio_is_render_host_of_generate_notes():
    from music2midi_amd import synth
    from music2midi_amd.model import Music2MIDI
    cfg = _small_config()
    cfg["inference"]["midi_grammar"] = True                                                 # random weights write no valid note otherwise
    torch.manual_seed(5)
    m = Music2MIDI(cfg).cuda().eval()
    clip = synth.waveform(3, 7 * 16000, "music")
    notes, sound = m.generate_audio(audio_y=clip)
    print(f"generate_audio: {len(notes)} notes, {sound.numel()} samples at 16 kHz")
    assert len(notes) > 0 and notes.shape[1] == 4 and np.array_equal(notes, m.generate_notes(audio_y=clip))
    assert len(render.pack(notes, 16000).on) > 0                                            # notes that sound, not only rows
    assert sound.is_cuda and sound.device == m.device and sound.dtype == torch.float32 and sound.numel() > 0
    assert sound.abs().max().item() == 1.0                                                  # normalised by default
    assert np.array_equal(_bits(sound), _bits(render.render_host(notes, 16000, normalize=True)))
    _, raw = m.generate_audio(audio_y=clip, fs=48000, normalize=False)
    assert raw.numel() != sound.numel() and abs(raw.numel() - 3 * sound.numel()) <= 3
    assert 0 < raw.abs().max().item() != 1.0                                                # not normalised
    assert np.array_equal(_bits(raw), _bits(render.render_host(notes, 48000)))


def test_the_stand_in_midi_object_gives_a_preview(tmp_path):
    """ref webui.py:64-67: generate -> write -> fluidsynth(fs=48000) -> the preview file, on the stand-in MIDI object."""
    from music2midi_amd import audio
    notes = random_notes(4, 40, 3.0)
    midi = numpy_to_midi(notes)
    midi.write(str(tmp_path / "out.mid"))
    y = midi.fluidsynth(fs=48000)
    assert y.dtype == np.float64 and np.isfinite(y).all() and np.abs(y).max() == 1.0
    assert len(y) == int(np.floor(notes[:, 1].max() * 48000 + 0.5)) + 2400
    assert np.array_equal(y.astype(np.float32), render.render_host(notes, 48000, normalize=True))
    assert np.array_equal(midi.synthesize(fs=16000).astype(np.float32), render.render_host(notes, 16000))
    audio.write_wav(tmp_path / "out.wav", y, 48000)
    back, rate = audio.read_wav(tmp_path / "out.wav")
    assert rate == 48000 and back.shape == (len(y), 1) and np.abs(back[:, 0] - y).max() < 1e-4


def test_a_training_step_on_a_synthetic_batch():
    from music2midi_amd.model import Music2MIDI
    cfg = _small_config()
    batch = render.synthetic_batch(np.random.default_rng(2), 2, cfg)
    host = render.synthetic_batch(np.random.default_rng(2), 2, cfg, device="cpu")
    assert batch.input_waveform.is_cuda and batch.input_waveform.shape == (2, 48000) and batch.cond_index.is_cuda
    assert np.array_equal(_bits(batch.input_waveform), _bits(host.input_waveform))
    assert all(1 <= len(n) <= 90 for n in batch.notes_batch)
    torch.manual_seed(5)
    m = Music2MIDI(cfg).cuda().eval()
    m.train_precision = "fp32"
    loss = m.training_step(batch, 0)
    assert torch.isfinite(loss).item()
