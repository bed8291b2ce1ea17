"""GPU: the beat tracker's kernels (csrc/beats.hip) EQUAL to the definition (music2midi_amd/beats.py) on identical inputs - envelopes
with planted ties at every comparison and clips that cross the workgroup's tile, periods, score tables, beats and counts at every
size around the kernel's block and tile borders - and the whole device path held to the planted truth of beats_cases.py."""
import numpy as np
import pytest
import torch

from music2midi_amd import align, beats

from beats_cases import CASES, F_CAP, case, f_measure, period_ok

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ m2m_beat_envelope
def _planted_L(rng, frames):
    """Random log energies whose predecessors lie on multiples of 1/16, with rises of exactly k / 16 and one ulp below, rises above
    16, bands exactly at M - ln 20 and one ulp below, silent frames and frames at exactly -6.0 and one ulp above."""
    L = (rng.integers(-140, 30, (frames, 88)) / 16.0).astype(np.float32)       # every value a multiple of 1/16
    for t in range(1, frames):
        bands = rng.choice(88, 12, replace=False)
        for i, k in enumerate((1, 2, 5, 17)):
            L[t, bands[i]] = L[t - 1, bands[i]] + np.float32(k / 16)           # exactly k / 16: k
            L[t, bands[4 + i]] = np.nextafter(L[t - 1, bands[4 + i]] + np.float32(k / 16), np.float32(-100))     # one ulp below: k - 1
        L[t - 1, bands[8]], L[t, bands[8]] = -13.5, 2.75                       # a rise of 16.25: cut at 255
        if t % 3 == 0:
            M = L[t].max()
            L[t, bands[9]] = M - align.D_THRESH[3]                             # exactly at the threshold: counted
            L[t, bands[10]] = np.nextafter(M - align.D_THRESH[3], np.float32(-100))       # one ulp below: not
    if frames > 12:
        L[5] = rng.uniform(-13.8, -6.5, 88)                                    # silent
        L[9] = np.minimum(L[9], np.float32(-6.0))
        L[9, 40] = -6.0                                                        # M == -6.0 exactly: silent
        L[10] = np.minimum(L[10], np.float32(-6.5))
        L[10, 41] = np.nextafter(np.float32(-6.0), np.float32(0))              # one ulp above: not silent
    return L


def test_envelope_equals_the_definition():
    rng = np.random.default_rng(0)
    clips = [_planted_L(rng, f) for f in (1, 2, 3, 1025, 33, 64, 65)]          # 32 frames per workgroup: 33, 64, 65 cross its edge
    got = beats.onset_envelope(clips)
    for k, (L, e) in enumerate(zip(clips, got)):
        want = beats.onset_envelope_host(L)
        assert e.dtype == torch.int32 and e.is_cuda
        assert np.array_equal(e.cpu().numpy(), want), (k, len(L), np.flatnonzero(e.cpu().numpy() != want)[:8])
    want = beats.onset_envelope_host(clips[3])
    assert want[0] == 0 and want[5] == 0 and want[9] == 0 and want[10] > 0 and want.max() > 255 and want[32] > 0 and want[64] > 0
    one = beats.onset_envelope(clips[3])
    assert np.array_equal(one.cpu().numpy(), want)
    top = np.zeros((40, 88), np.float32)
    top[::2] = -20.0                                                           # every band rises by 20 in every other frame: the bound
    assert beats.onset_envelope(top).cpu().numpy().tolist() == [0, 22440] * 20
    with pytest.raises(ValueError):
        beats.onset_envelope([np.zeros((0, 88), np.float32)])


# ------------------------------------------------------------------ m2m_beat_track
def _check(got, want, what):
    assert got[0] == want[0], (what, got[0], want[0])
    assert got[1].dtype == np.int64 and np.array_equal(got[1], want[1]), (what, np.flatnonzero(got[1] != want[1]))
    assert got[2].dtype == np.int32 and got[2].shape == want[2].shape and np.array_equal(got[2], want[2]), (what, got[2][:12], want[2][:12])


def _kinds(rng, F):
    train = np.zeros(F, np.int32)
    train[::23] = 5000
    sparse = (rng.integers(0, 22441, F) * (rng.random(F) < 0.1)).astype(np.int32)
    return (("silent", np.zeros(F, np.int32)), ("constant", np.full(F, 300, np.int32)), ("train", train),
            ("random", rng.integers(0, 22441, F).astype(np.int32)), ("sparse", sparse))


def test_track_sizes_and_envelope_kinds_in_one_launch():
    """1 .. 4097 frames - around the first lags (15, 16, 17), the autocorrelation's reach (200, 201, 202), twice it (401) and its tile
    (1025) - of silent, constant, impulse-train and random envelopes as ONE launch, the smallest clip next to the largest."""
    rng = np.random.default_rng(1)
    sizes = (1, 4097, 2, 15, 16, 17, 31, 200, 201, 202, 401, 1025)
    envs, kinds = [], []
    for F in sizes:
        for kind, e in _kinds(rng, F):
            envs.append(e), kinds.append((kind, F))
    got = beats.track_envelopes(envs)
    assert len(got) == 5 * len(sizes)
    for g, e, what in zip(got, envs, kinds):
        _check(g, beats.track_envelope_host(e), what)
        if what[0] == "silent":
            assert g[0] == 25 and len(g[2]) == 0 and not g[1].any()
    _check(beats.track_envelopes(envs[7]), got[7], "one clip")


def test_track_forced_periods_next_to_estimated_ones():
    rng = np.random.default_rng(2)
    envs, periods = [], []
    for period in (15, None, 16, 25, 0, 99, 100, None):
        for kind, e in _kinds(rng, 777)[2:]:
            envs.append(e), periods.append(period)
    zero = np.zeros((101, 201), np.int32)
    for tables in ({}, {"table": zero}, {"prior": beats.tempo_prior(90.0, 1.0), "table": beats.penalty_table(400.0), "default_period": 40}):
        got = beats.track_envelopes(envs, periods, **tables)
        for g, e, p in zip(got, envs, periods):
            _check(g, beats.track_envelope_host(e, p, **tables), (p, sorted(tables)))
            assert not p or g[0] == p
    for bad in (14, 101):
        with pytest.raises(ValueError, match="forced period"):
            beats.track_envelopes(envs[:1], [bad])
    with pytest.raises(ValueError, match="32768"):
        beats.track_envelopes(np.zeros(32769, np.int32))


def test_track_the_bound_case():
    """Spikes of 22440 every 25 frames over 32768 frames: the longest clip, the largest novelty, the autocorrelation's largest sums."""
    e = np.zeros(32768, np.int32)
    e[::25] = 22440
    got = beats.track_envelopes([e, e[:100]], [None, 100])
    _check(got[0], beats.track_envelope_host(e), "bound")
    _check(got[1], beats.track_envelope_host(e[:100], 100), "next to it")
    assert got[0][0] == 25 and got[0][2].tolist() == list(range(0, 32768, 25))


def test_track_on_another_stream_and_twice():
    rng = np.random.default_rng(3)
    envs = [e for _, e in _kinds(rng, 3000)[2:]]
    first = beats.track_envelopes(envs)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = beats.track_envelopes(envs)
    side.synchronize()
    again = beats.track_envelopes(envs)
    for k, e in enumerate(envs):
        _check(other[k], first[k], "stream")
        _check(again[k], first[k], "second call")
        _check(first[k], beats.track_envelope_host(e), "definition")


# ------------------------------------------------------------------ the whole device path
def _differing_envelope_values(y):
    dev = torch.device("cuda", torch.cuda.current_device())
    L, frames = align._band_log_energies_device([torch.from_numpy(y).to(dev)], dev)
    got = beats._envelope_device(L, frames, dev).cpu().numpy()
    want = beats.onset_envelope_host(align.band_log_energies_host(y))
    assert got.shape == want.shape
    return float((got != want).mean()), int(np.abs(got.astype(np.int64) - want).max())


def test_track_batch_finds_the_planted_beats():
    """Held to the truth, not to the definition: the band energies come from the frontend kernel and differ from numpy's in the last
    bits, so a few envelope values, and with them a beat, may differ.  Three recordings of different lengths, one launch per stage."""
    specs = (CASES[0], CASES[2], CASES[3])
    cases = [case(*s) for s in specs]
    results = beats.track_batch([c["audio"] for c in cases])
    for spec, c, r in zip(specs, cases, results):
        f = f_measure(r.beat_times, c["beats"])
        share, worst = _differing_envelope_values(c["audio"])
        print(f"{spec}: P {r.period} ({r.bpm:.1f} BPM), {len(r.beat_times)} beats for {len(c['beats'])}, F {f:.3f}; "
              f"envelope values that differ from the definition's: {share:.5f} (by at most {worst})")
        assert isinstance(r, beats.BeatResult) and np.array_equal(r.beat_times, r.beat_frames / 50.0) and r.score.shape == (101,)
        assert period_ok(r.period, c["bpm"])
        assert f >= F_CAP
    # the routes the device path does not take: audio that is not finite goes through the definition; too little audio is refused
    bad = cases[0]["audio"].copy()
    bad[100] = np.inf
    assert isinstance(beats.track(bad), beats.BeatResult)
    with pytest.raises(ValueError, match="1025"):
        beats.track(np.zeros(1024, np.float32))
    from music2midi_amd import audio
    r16 = beats.track(torch.from_numpy(audio.resample(cases[0]["audio"], 22050, 16000)).cuda(), sr=16000)
    assert period_ok(r16.period, cases[0]["bpm"]) and f_measure(r16.beat_times, cases[0]["beats"]) >= F_CAP


def test_track_notes_equals_the_definition_and_finds_the_beats():
    cases = [case(*s) for s in CASES]
    got = beats.track_notes([c["notes"] for c in cases], [c["frames"] for c in cases])
    for c, r in zip(cases, got):
        want = beats.track_notes_host(c["notes"], c["frames"])                 # the envelope is made on the host in both paths
        assert r.period == want.period and np.array_equal(r.beat_frames, want.beat_frames) and np.array_equal(r.score, want.score)
        assert period_ok(r.period, c["bpm"]) and f_measure(r.beat_times, c["beats"]) >= F_CAP
    one = beats.track_notes(cases[1]["notes"])
    assert isinstance(one, beats.BeatResult) and period_ok(one.period, cases[1]["bpm"])
    # the dataset filter on the device route
    c = cases[2]
    wp = np.array([[0.0, 30.0], [0.0, 30.0]])
    result = align.AlignResult(c["notes"], wp, 0, 0, {"wp_std": 1.0, "time_diff_ratio": 0.01})
    metrics, ok = beats.filter_pair(result, c["notes"], 30.0)
    assert ok and np.array_equal(beats.aligned_beats(c["notes"], wp), beats.track_notes_host(c["notes"]).beat_times)


def test_generate_beats_and_the_beat_grid_on_a_random_model(tmp_path):
    from music2midi_amd import audio
    import copy
    from music2midi_amd.config import DEFAULT_CONFIG
    from music2midi_amd.model import Music2MIDI
    from music2midi_amd.utils import SimpleMIDI
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["model"]["t5"].update(d_model=128, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2)
    cfg["inference"]["midi_grammar"] = True                                    # random weights write no valid note otherwise
    torch.manual_seed(5)
    model = Music2MIDI(cfg).cuda().eval()
    c = case(*CASES[0])
    y = audio.resample(c["audio"], 22050, 16000).astype(np.float32)
    r = model.generate_beats(audio_y=y, sr=16000)
    f = f_measure(r.beat_times, c["beats"])
    print(f"generate_beats: P {r.period}, F {f:.3f}")
    assert isinstance(r, beats.BeatResult) and period_ok(r.period, c["bpm"]) and f >= F_CAP
    plain = model.generate(audio_y=y, sr=16000)
    midi = model.generate(audio_y=y, sr=16000, beat_grid=True)
    assert isinstance(midi, SimpleMIDI) and np.array_equal(midi.beat_times, r.beat_times)
    assert getattr(plain, "beat_times", None) is None
    want = np.array([[n.start, n.end, n.pitch, n.velocity] for n in plain.instruments[0].notes], dtype=np.float64).reshape(-1, 4)
    assert np.array_equal(midi.note_array(), want)                             # the notes are what they were
    midi.write(tmp_path / "grid.mid")
    assert (tmp_path / "grid.mid").read_bytes().count(b"\xff\x51\x03") == len(r.beat_times) + (0 if r.beat_times[0] == 0 else 1)
    snapped = model.generate(audio_y=y, sr=16000, beat_grid=True, quantize=4)
    assert np.array_equal(snapped.beat_times, r.beat_times)
    assert len(want) > 0 and np.array_equal(snapped.note_array(), beats.quantize(want, r.beat_times, 4))
    with pytest.raises(ValueError, match="beat_grid"):
        model.generate(audio_y=y, sr=16000, quantize=4)
    model.config.inference.beat_grid = True
    assert np.array_equal(model.generate(audio_y=y, sr=16000).beat_times, r.beat_times)       # the config key does the same
