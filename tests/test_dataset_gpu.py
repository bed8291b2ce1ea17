"""GPU: the dataset's crop kernel (csrc/dataset.hip) and the device side of music2midi_amd/dataset.py against crop_host, the host
definition (read_wav, the slice, mean over the channels, audio.resample of the slice alone).

Every comparison is on the bit patterns, as in test_ingest_gpu.py: the kernel repeats the host's rounded operations in the host's
order, so any difference is a kernel bug - a tap, a window bound, a contraction - and not noise.  The kernel's tile is 256 outputs
per workgroup, its LDS window 4096 input frames (dataset.LDS_WINDOW)."""
import copy
import ctypes as C
import struct

import numpy as np
import pytest
import torch

from music2midi_amd import audio, dataset, ingest, native
from music2midi_amd.dataset import Music2MIDIDataset

from dataset_fixtures import add_recording, config, notes_with, signal, wav

pytestmark = pytest.mark.gpu

SR = 22050
LIST_CHUNK = b"LIST" + struct.pack("<I", 6) + b"INFOab"          # moves the data chunk to an offset that is 2 mod 4


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).view(np.uint32)


def _upload(raw: bytes) -> torch.Tensor:
    return torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).cuda()


def _launch(specs, T, out=None):
    """m2m_dataset_crop_f32 on clips given as (uint8 CUDA tensor that starts at the clip's first frame, frames, channels, kind, rate)."""
    dev = torch.device("cuda", torch.cuda.current_device())
    clips = (native.DatasetClip * len(specs))()
    for c, (body, frames, n_ch, kind, rate) in zip(clips, specs):
        up, down = dataset._host_ratio(rate, SR)
        assert body.numel() >= frames * n_ch * ingest.FORMATS[kind][1]
        c.bytes_dev = body.data_ptr()
        c.h_phase_dev = None if up == down else ingest._filter_on(dev, up, down).data_ptr()
        c.n_frames, c.channels, c.format = frames, n_ch, ingest.FORMATS[kind][0]
        c.up, c.down, c.half = up, down, 10 * max(up, down)
    table = torch.empty(C.sizeof(clips), dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.empty((len(specs), T), dtype=torch.float32, device=dev)
    native.check(native.load().m2m_dataset_crop_f32(clips, len(specs), table.data_ptr(), out.data_ptr(), out.stride(0), T,
                                                    native.stream_handle(dev)), "m2m_dataset_crop_f32")
    return out


# ------------------------------------------------------------------ the kernel, called directly
def test_tile_edges():
    """One mono f32 clip at 1 / 2: inputs that give exactly 255, 256, 257 and 513 outputs (a partial tile, a full one, one output
    in the second, one in the third), and the shortest clips."""
    for n in (1, 7, 510, 512, 514, 1026):
        y = signal(n, n, 44100)
        want = audio.resample(y, 44100, SR)
        assert len(want) == -(-n // 2)
        got = _launch([(_upload(y.tobytes()), n, 1, "f32", 44100)], len(want))
        assert got.shape == (1, len(want))
        bad = np.flatnonzero(_bits(got[0]) != _bits(want))
        assert not len(bad), f"{n} frames: {len(bad)} of {len(want)} outputs differ, first at {bad[0]}"
    assert [-(-n // 2) for n in (510, 512, 514, 1026)] == [255, 256, 257, 513]


@pytest.fixture(scope="module")
def trap(tmp_path_factory):
    """A 44.1 kHz s16 stereo recording of 1.5 s: full scale, then 0.5 s at amplitude 0.01, then full scale again."""
    root = tmp_path_factory.mktemp("trap")
    rate, seg = 44100, 22050
    y = signal(3 * seg, 21, rate, scale=1.2).clip(-1, 1)
    y[seg:2 * seg] = signal(seg, 22, rate, scale=0.01 / 0.6)
    assert np.abs(y[seg:2 * seg]).max() < 0.03 and np.abs(y[:seg]).max() == 1.0 == np.abs(y[2 * seg:]).max()
    add_recording(root, "trap", wav("s16", 2, rate, 1.5, 0, mono=y), notes_with([2, 2, 2], 0.5))
    return root


def test_the_neighbours_of_a_clip_do_not_exist_for_the_filter(trap):
    ds = Music2MIDIDataset(trap, ["trap"], config(), device="cuda")
    assert ds.residency() == (["trap"], [], [])
    path = trap / "audio" / "trap.wav"
    got = ds.crop_device([0], [0.5])
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == (1, 11025)
    assert np.array_equal(_bits(got), _bits(ds.crop_host([0], [0.5])))
    assert np.array_equal(_bits(got[0]), _bits(ingest.load_audio_device(path, SR, offset=0.5, duration=0.5)))
    # NOT the same span of the resampled whole, whose first and last outputs saw the full-scale frames next to the clip
    whole = audio.resample(audio.read_wav(path)[0].mean(axis=1), 44100, SR)[11025:22050]
    assert np.array_equal(_bits(got[0, 50:-50]), _bits(whole[50:-50]))
    assert not np.array_equal(_bits(got[0]), _bits(whole))
    assert np.abs(got[0, :10].cpu().numpy() - whole[:10]).max() > 1e-3 and np.abs(got[0, -10:].cpu().numpy() - whole[-10:]).max() > 1e-3
    # the clip at the recording's first frame and the clip that ends on its last frame, by direct calls on the data chunk
    raw = path.read_bytes()
    lay = audio.wav_layout(path, raw)
    chunk = raw[lay.data_offset:lay.data_offset + lay.data_size]
    assert len(chunk) == 3 * 22050 * 4
    body = _upload(chunk)
    y = audio.read_wav(path)[0].mean(axis=1)
    for first in (0, 22050, 44100):
        want = audio.resample(y[first:first + 22050], 44100, SR)
        got = _launch([(body[first * 4:], 22050, 2, "s16", 44100)], 11025)
        assert np.array_equal(_bits(got[0]), _bits(want)), first


MIXED = [("u8", 1, 8000), ("f32", 1, 22050), ("s16", 2, 44100), ("s24", 3, 48000), ("f64", 7, 96000), ("s32", 2, 32000)]


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    """Six recordings of 1.5 s: every sample format, six rates (22 050 Hz is the 1 / 1 path), 1 to 7 channels, the 24-bit one with
    its data chunk at an offset that is 2 mod 4."""
    root = tmp_path_factory.mktemp("mixed")
    ids = []
    for k, (kind, n_ch, rate) in enumerate(MIXED):
        pid = f"{kind}_{rate}"
        add_recording(root, pid, wav(kind, n_ch, rate, 1.5, 30 + k, before_data=LIST_CHUNK if kind == "s24" else b""), notes_with([3, 2], 0.5),
                      genre=("pop", "rock", "classical")[k % 3], difficulty=("beginner", "advanced")[k % 2])
        ids.append(pid)
    assert audio.wav_layout("s24", (root / "audio" / "s24_48000.wav").read_bytes()).data_offset % 4 == 2
    return root, ids


def test_one_launch_over_mixed_clips(mixed, monkeypatch):
    root, ids = mixed
    ds = Music2MIDIDataset(root, ids, config(), device="cuda")
    assert ds.segment_samples == 11025 and ds.residency() == (ids, [], [])
    assert ds.resident_bytes() == sum(int(1.5 * rate) * n_ch * ingest.FORMATS[kind][1] for kind, n_ch, rate in MIXED)
    calls = []
    real = native.load().m2m_dataset_crop_f32
    monkeypatch.setattr(native.load(), "m2m_dataset_crop_f32", lambda *a: (calls.append(a[1]), real(*a))[1])
    indices, starts = [0, 1, 2, 3, 4, 5, 2], [0.5, 0.0, 0.5, 0.0, 0.5, 0.0, 0.0]
    got = ds.crop_device(indices, starts)
    assert calls == [7]                                                            # one launch for the whole batch
    want = ds.crop_host(indices, starts)
    assert got.shape == want.shape == (7, 11025)
    for b, i in enumerate(indices):
        bad = np.flatnonzero(_bits(got[b]) != _bits(want[b]))
        assert not len(bad), f"{ids[i]}: {len(bad)} outputs differ, first at {bad[0]}"


def test_nothing_is_written_outside_the_rows_and_the_tails_are_zero(mixed):
    root, ids = mixed
    specs, wants = [], []
    for pid, (kind, n_ch, rate) in list(zip(ids, MIXED))[:4]:
        path = root / "audio" / f"{pid}.wav"
        raw = path.read_bytes()
        lay = audio.wav_layout(path, raw)
        frames = int(0.5 * rate)
        specs.append((_upload(raw[lay.data_offset:lay.data_offset + lay.data_size]), frames, n_ch, kind, rate))
        wants.append(audio.resample(audio.read_wav(path)[0][:frames].mean(axis=1), rate, SR))
    B, T, stride, guard = len(specs), 11025 + 300, 11025 + 300 + 37, 512
    buf = torch.full((guard + B * stride + guard,), float("nan"), dtype=torch.float32, device="cuda")
    out = buf[guard:guard + B * stride].view(B, stride)[:, :T]
    assert out.stride(0) == stride > T
    _launch(specs, T, out=out)
    host = buf.cpu().numpy()
    assert np.isnan(host[:guard]).all() and np.isnan(host[guard + B * stride:]).all()
    rows = host[guard:guard + B * stride].reshape(B, stride)
    assert np.isnan(rows[:, T:]).all()
    for b, want in enumerate(wants):
        assert len(want) == 11025 and np.array_equal(_bits(rows[b, :11025]), _bits(want)), b
        assert np.array_equal(_bits(rows[b, 11025:T]), np.zeros(300, np.uint32)), b   # exact +0, a whole tile of padding and a partial one


# ------------------------------------------------------------------ the routes
@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    """Three 44.1 kHz s16 stereo recordings, one with 8 channels (not eligible) and one at a rate whose 1 / 16 tile does not fit
    the LDS window."""
    root = tmp_path_factory.mktemp("routes")
    lib = native.load()
    fast = next(r for r in (352800, 705600) if lib.m2m_dataset_crop_window(*dataset._host_ratio(r, SR)) > dataset.LDS_WINDOW)
    assert dataset._host_ratio(fast, SR) == ingest.ratio(fast, SR)                 # within 1..1000: eligible, refused for its window only
    ids = ["cd0", "cd1", "cd2", "eight", "fast"]
    for k, (pid, kind, n_ch, rate) in enumerate([("cd0", "s16", 2, 44100), ("cd1", "s16", 2, 44100), ("cd2", "s16", 2, 44100),
                                                 ("eight", "s16", 8, 44100), ("fast", "u8", 1, fast)]):
        add_recording(root, pid, wav(kind, n_ch, rate, 1.5, 50 + k), notes_with([3, 2], 0.5))
    return root, ids


def test_streamed_and_host_routes(routes):
    root, ids = routes
    one = 66150 * 4                                                                # bytes of one stereo recording
    ds = Music2MIDIDataset(root, ids[:3], config(), device="cuda", resident_bytes=one + 100)
    assert ds.residency() == (["cd0"], ["cd1", "cd2"], []) and ds.resident_bytes() == one
    assert Music2MIDIDataset(root, ids[:3], config(), device="cuda", resident_bytes=0).residency() == ([], ids[:3], [])
    ds = Music2MIDIDataset(root, ids, config(), device="cuda", resident_bytes=one + 100)
    assert ds.residency() == (["cd0"], ["cd1", "cd2"], ["eight", "fast"])
    assert ingest.eligible(root / "audio" / "fast.wav", SR) and not ingest.eligible(root / "audio" / "eight.wav", SR)
    indices, starts = [4, 1, 0, 3, 2, 1], [0.5, 0.0, 0.5, 0.0, 0.5, 0.5]
    got, want = ds.crop_device(indices, starts), ds.crop_host(indices, starts)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(ds.crop_device([2, 1], [0.0, 0.5])), _bits(ds.crop_host([2, 1], [0.0, 0.5])))      # streamed clips only
    assert np.array_equal(_bits(ds.crop_device([3, 4], [0.5, 0.0])), _bits(ds.crop_host([3, 4], [0.5, 0.0])))      # host rows only
    dev = ds.batch(indices, np.random.default_rng(4), augment=False)
    host = ds.batch(indices, np.random.default_rng(4), augment=False, device_crop=False)
    assert dev.input_waveform.is_cuda and host.input_waveform.is_cuda and torch.equal(dev.input_waveform, host.input_waveform)
    assert torch.equal(dev.cond_index, host.cond_index) and all(np.array_equal(a, b) for a, b in zip(dev.notes_batch, host.notes_batch))


# ------------------------------------------------------------------ through the model
def test_batch_end_to_end(mixed):
    from music2midi_amd.model import Music2MIDI
    root, ids = mixed
    cfg = config(batch_size=4)
    cfg["model"]["t5"].update(d_model=128, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2)
    cfg["trainer"].update(log_every_n_steps=1000, device_labels=True)
    ds = Music2MIDIDataset(root, ids, cfg, device="cuda")
    indices = [2, 0, 5, 3]
    dev = ds.batch(indices, np.random.default_rng(3))
    host = ds.batch(indices, np.random.default_rng(3), device_crop=False)
    plain = ds.batch(indices, np.random.default_rng(3), augment=False)
    assert dev.input_waveform.shape == (4, 11025) and torch.equal(dev.input_waveform, host.input_waveform)
    assert not torch.equal(dev.input_waveform, plain.input_waveform)               # the augmentation ran
    assert torch.equal(dev.cond_index, host.cond_index) and dev.cond_index.tolist() == [ds.cond_indices[i] for i in indices]
    assert len(dev.notes_batch) == 4 and all(np.array_equal(a, b) and a.dtype == np.float64 for a, b in zip(dev.notes_batch, host.notes_batch))
    torch.manual_seed(5)
    m = Music2MIDI(copy.deepcopy(cfg)).cuda().eval()                              # random-init weights; eval(): no dropout
    m.train_precision = "fp32"
    assert m._labels(dev.notes_batch).is_cuda
    losses = [m.training_step(batch, 0).clone() for batch in (dev, host)]
    assert torch.isfinite(losses[0]) and torch.equal(losses[0], losses[1])


def test_crop_device_on_a_side_stream(mixed):
    """crop_device enqueues on torch's current stream and waits for nothing: on a side stream, joined by an event, it gives the rows
    of the default stream."""
    root, ids = mixed
    ds = Music2MIDIDataset(root, ids, config(), device="cuda", resident_bytes=200000)   # streamed clips as well
    assert ds.residency().resident and ds.residency().streamed
    indices, starts = [0, 1, 2, 3, 4, 5], [0.0, 0.5, 0.0, 0.5, 0.0, 0.5]
    want = ds.crop_device(indices, starts)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = ds.crop_device(indices, starts)
        done = torch.cuda.Event()
        done.record(side)
    torch.cuda.current_stream().wait_event(done)
    got.record_stream(torch.cuda.current_stream())
    assert torch.equal(got, want) and np.array_equal(_bits(got), _bits(ds.crop_host(indices, starts)))
