"""CPU: the definition of the beat tracker (music2midi_amd/beats.py) on hand-made inputs with the results worked out in the test, the
dataset filter, the beat grid and the tempo-mapped MIDI file, what the library answers on its arguments alone, and the definition's
quality on the seeded cases of beats_cases.py."""
import ctypes as C
import struct
from pathlib import Path

import numpy as np
import pytest

from music2midi_amd import align, beats, native
from music2midi_amd.config import default_config
from music2midi_amd.utils import SimpleInstrument, SimpleMIDI, SimpleNote, numpy_to_midi, simple_midi

from beats_cases import CASES, F_CAP, LIMIT_CASE, case, f_measure, period_ok

M2M_ERR_INVALID = -1
GOLDEN = Path(__file__).resolve().parent / "golden" / "beats"


# ------------------------------------------------------------------ a plain loop over Python integers
def plain_track(e, period=0, prior=None, table=None, default_period=25):
    """The module docstring's definition, frame by frame and candidate by candidate in Python integers."""
    prior = beats.tempo_prior() if prior is None else prior
    table = beats.penalty_table() if table is None else table
    e = [int(x) for x in e]
    F = len(e)
    o = [max(0, 25 * e[t] - sum(e[u] for u in range(max(0, t - 12), min(F, t + 13)))) for t in range(F)]
    a = [0] * 201
    nz = [t for t in range(F) if o[t]]
    for k in range(15, min(200, F - 1) + 1):
        a[k] = sum(o[t] * o[t - k] for t in nz if t >= k) // (F - k)
    score = [0] * 101
    for l in range(15, 101):
        score[l] = (a[l] + a[2 * l] // 2) * int(prior[l])
    P = period
    if not P:
        P = max(range(15, 101), key=lambda l: (score[l], -l))
        if score[P] == 0:
            P = default_period
    if not any(o):
        return P, score, []
    s = sum(o) // max(1, len(nz))
    lo, hi = (P + 1) // 2, 2 * P
    Cs, back = [0] * F, [-1] * F
    for t in range(F):
        Cs[t] = o[t]
        if t >= lo:
            best, pick = None, None
            for tau in range(lo, min(hi, t) + 1):
                v = Cs[t - tau] - ((int(table[P][tau]) * s) >> 8)
                if best is None or v > best:                                   # the first of equal values stays: the smallest tau
                    best, pick = v, tau
            Cs[t], back[t] = o[t] + best, t - pick
    start = max(0, F - P)
    t = max(range(start, F), key=lambda u: (Cs[u], -u))
    chain = []
    while t >= 0:
        chain.append(t)
        t = back[t]
    return P, score, chain[::-1]


def _same(e, period=None, **tables):
    got = beats.track_envelope_host(e, period, **tables)
    want = plain_track(e, period or 0, **tables)
    assert got[0] == want[0] and got[1].dtype == np.int64 and got[1].tolist() == want[1], (got[0], want[0])
    assert got[2].dtype == np.int32 and got[2].tolist() == want[2]
    return got


# ------------------------------------------------------------------ the tables and the envelopes
def test_tables():
    prior, table = beats.tempo_prior(), beats.penalty_table()
    assert prior.dtype == np.int32 and prior.shape == (101,) and not prior[:15].any() and prior[25] == 4096 and prior.argmax() == 25
    assert prior[50] == round(4096 * np.exp(-0.5 * 4.0)) == 554                # one octave off at half an octave's width: two sigma
    assert beats.tempo_prior(100.0, 1.0)[30] == 4096 and beats.tempo_prior(100.0, 1.0)[60] == round(4096 * np.exp(-0.5))
    assert table.dtype == np.int32 and table.shape == (101, 201) and not table[:15].any() and not table[:, 0].any()
    assert all(table[P, P] == 0 for P in range(15, 101)) and table[25, 50] == round(25600 * np.log(2.0) ** 2) == 12300
    assert table.max() == table[100, 1] == 542914 and max(table[P, (P + 1) // 2:2 * P + 1].max() for P in range(15, 101)) == 12300
    assert beats.penalty_table(50.0)[25, 50] == 6150


def test_onset_envelope_by_hand():
    floor = np.float32(-13.8)
    L = np.full((6, 88), floor, dtype=np.float32)
    L[:, 0] = 0.0                                                              # the loudest band of frames 0..4: M = 0, never rises
    d3 = align.D_THRESH[3]                                                     # M - ln 20 = -2.9957 there
    L[:, 7], L[2:, 7] = -2.0, -1.0                                             # frame 2: a rise of exactly 1.0: 16
    L[:, 9], L[3:, 9] = np.float32(-1.0) - np.float32(5 / 16), -1.0            # frame 3: exactly 5 / 16: 5
    L[:, 10], L[3:, 10] = np.nextafter(np.float32(-1.0) - np.float32(5 / 16), np.float32(0)), -1.0     # one ulp less: 4
    L[:, 11], L[4:, 11] = -0.5, -2.9                                           # frame 4: a fall counts nothing
    L[:, 12], L[4:, 12] = -13.0, 0.0                                           # 13 * 16 = 208
    L[5, 13] = 3.0                                                             # frame 5: M = 3; 16.8 * 16 is cut at 255
    L[5, 14] = np.float32(3.0) - d3                                            # exactly at M - ln 20: counted
    L[5, 15] = np.nextafter(np.float32(3.0) - d3, np.float32(-100))            # one ulp below: not counted
    e = beats.onset_envelope_host(L)
    at_threshold = int((L[5, 14] - L[4, 14]) * np.float32(16.0))
    assert at_threshold == 220 and e.dtype == np.int32 and e.tolist() == [0, 0, 16, 5 + 4, 208, 255 + 220]
    # frame 0 is 0 whatever it holds; a frame at exactly -6.0 is silent, one just above is not
    L = np.full((3, 88), floor, dtype=np.float32)
    L[1, 3], L[2, 3] = -6.0, np.nextafter(np.float32(-6.0), np.float32(0))
    assert beats.onset_envelope_host(L).tolist() == [0, 0, 0]
    L[1, 3] = floor
    assert beats.onset_envelope_host(L).tolist() == [0, 0, 124]                # (13.8 - 6) * 16 = 124.8
    assert beats.onset_envelope_host(np.zeros((0, 88), np.float32)).shape == (0,) and beats.onset_envelope_host(L[:1]).tolist() == [0]
    loud = np.zeros((2, 88), np.float32)
    loud[0] = -20.0
    assert beats.onset_envelope_host(loud).tolist() == [0, 88 * 255] and beats.ENV_MAX == 22440


def test_note_envelope():
    notes = np.array([[0.0, 0.5, 60, 80], [0.009, 0.5, 62, 80], [0.01, 0.5, 64, 80], [0.99, 1.02, 65, 80], [1.5, 1.6, 60, 80], [-0.02, 0.1, 60, 80]])
    e = beats.note_envelope(notes)
    assert e.dtype == np.int32 and len(e) == 1 + 80 and e[0] == 128 and e[1] == 64 and e[50] == 64 and e[75] == 64 and e.sum() == 5 * 64
    assert beats.note_envelope(notes, 60).sum() == 4 * 64                      # the onset at 1.5 s lies outside 60 frames
    assert beats.note_envelope(np.repeat(notes[:1], 400, axis=0))[0] == 22440  # 64 * 400 is cut at the bound
    assert beats.note_envelope(np.zeros((0, 4))).tolist() == [0]


# ------------------------------------------------------------------ the tracker
def test_impulse_train_of_period_25():
    E = 1000
    e = np.zeros(500, np.int32)
    e[::25] = E
    o = beats.novelty(e)
    assert o.dtype == np.int64 and o[::25].tolist() == [24 * E] * 20 and o.sum() == 20 * 24 * E      # alone in its window of 25
    P, score, found = _same(e)
    a25, a50, a100 = 19 * (24 * E) ** 2 // 475, 18 * (24 * E) ** 2 // 450, 16 * (24 * E) ** 2 // 400
    assert P == 25 and int(score[25]) == (a25 + a50 // 2) * 4096 and int(score[50]) == (a50 + a100 // 2) * 554
    assert not score[:15].any() and not score[26:50].any() and found.tolist() == list(range(0, 500, 25))


def test_plateaus_exercise_every_tie():
    """A penalty table of zeros and equal impulses every 5 frames: every candidate that lies on an impulse ties, the smallest tau has
    to win; and a constant envelope, whose novelty lives at the two ends only."""
    zero = np.zeros((101, 201), np.int32)
    e = np.zeros(90, np.int32)
    e[::5] = 700
    for period in (15, 16, 20):
        P, _, found = _same(e, period, table=zero)
        assert P == period
    # two equal frames at the start, period 15 (lo = 8, hi = 30): C[8] = C[0] (tau = 8 alone), C[9] ties between C[1] (tau = 8) and
    # C[0] (tau = 9) and takes tau = 8; every later frame ties too.  The first maximum of C over [5, 20) is C[8]: the beats are 0, 8.
    two = np.zeros(20, np.int32)
    two[:2] = 500
    assert beats.novelty(two)[:3].tolist() == [23 * 500, 23 * 500, 0]
    P, _, found = _same(two, 15, table=zero)
    assert found.tolist() == [0, 8]
    flat = np.full(60, 300, np.int32)
    o = beats.novelty(flat)
    assert o[:13].tolist() == [300 * (12 - t) for t in range(13)] and not o[12:48].any() and o[::-1][:12].tolist() == o[:12].tolist()
    _same(flat)
    _same(flat, 15, table=zero)
    _same(np.full(300, 22440, np.int32))


@pytest.mark.parametrize("F", (1, 2, 15, 16, 17))
def test_shortest_clips(F):
    e = np.full(F, 100, np.int32)
    P, score, found = _same(e)
    if F <= 15:                                                                # no lag of 15 or more fits: the default period, one beat
        assert P == 25 and not score.any() and found.tolist() == [0]
    if F == 16:                                                                # o[0] = o[15] = 25 * 100 - 13 * 100
        assert P == 15 and int(score[15]) == (1200 * 1200 // 1) * 1382 and not score[16:].any()
    if F == 17:                                                                # lag 15: 1200 * 1100 * 2 // 2; lag 16: 1200 * 1200 // 1
        assert int(score[15]) == 1200 * 1100 * 1382 and int(score[16]) == 1200 * 1200 * int(beats.tempo_prior()[16]) and P == 16
    _same(np.arange(F, dtype=np.int32) * 7 % 50)


def test_silent_clip_and_forced_periods():
    P, score, found = _same(np.zeros(300, np.int32))
    assert P == 25 and not score.any() and len(found) == 0
    assert _same(np.zeros(300, np.int32), 40)[0] == 40
    assert beats.track_envelope_host(np.zeros(300, np.int32), default_period=30)[0] == 30
    rng = np.random.default_rng(0)
    e = (rng.integers(0, 3000, 700) * (rng.random(700) < 0.2)).astype(np.int32)
    for period in (15, 100):
        P, _, found = _same(e, period)
        assert P == period and (np.diff(found) >= (period + 1) // 2).all() and (np.diff(found) <= 2 * period).all()
    _same(e)
    for bad in (14, 101, -3):
        with pytest.raises(ValueError, match="forced period"):
            beats.track_envelope_host(e, bad)
    with pytest.raises(ValueError, match="frames"):
        beats.track_envelope_host(np.zeros(0, np.int32))
    with pytest.raises(ValueError, match="22440"):
        beats.track_envelope_host(np.full(30, 22441, np.int32))


def test_envelope_at_its_bound():
    """Spikes of 22440 every 25 frames over 32768 frames: the autocorrelation's largest sums against Python integers."""
    e = np.zeros(32768, np.int32)
    e[::25] = 22440
    o = beats.novelty(e)
    assert o.max() == 24 * 22440 == 538560 < 2 ** 20
    score = beats.tempo_score(o)
    n, sq = len(range(0, 32768, 25)), 538560 ** 2
    a = {k: (n - k // 25) * sq // (32768 - k) for k in (25, 50, 75, 100, 150, 200)}
    assert n * sq < 2 ** 55 and int(score[25]) == (a[25] + a[50] // 2) * 4096 and int(score[100]) == (a[100] + a[200] // 2) * int(beats.tempo_prior()[100])
    assert int(score[75]) == (a[75] + a[150] // 2) * int(beats.tempo_prior()[75]) and not score[26:50].any()
    P, _, found = beats.track_envelope_host(e)
    assert P == 25 and found.tolist() == list(range(0, 32768, 25)) and len(found) <= 32768 // 8 + 1


# ------------------------------------------------------------------ the dataset filter
def test_beat_metrics_by_hand():
    times = [1.0 + 0.5 * k for k in range(30)]
    times[5] = 3.6                                                             # part 1 is (3.0, 3.6, 4.0): second difference -0.2
    times.insert(13, times[12] + 0.05)                                         # 0.05 s after its predecessor: dropped
    notes = np.zeros((9, 4))
    notes[:, 0] = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 1.5, 2.0, 2.5]                # six before the first beat, three inside part 0
    notes[:, 1] = notes[:, 0] + 0.1
    m = beats.beat_metrics(times, 16.0, notes)
    # 31 values in parts of 4, 3, 3, ...; part 0 spans 1.5 s, part 1 1.0 s.  The reference's zip pairs the six notes BEFORE the first
    # beat with part 0's span and the three notes of part 0 with part 1's: 6 / 1.5 = 4 and 3 / 1.0 = 3
    assert set(m) == {"max_beat_fluctuation", "max_note_density"}
    assert m["max_beat_fluctuation"] == pytest.approx(0.2, abs=1e-12) and m["max_note_density"] == 4.0
    assert beats.beat_metrics(times, 16.0, notes[6:])["max_note_density"] == 3.0
    with pytest.raises(ValueError):
        beats.beat_metrics([1.0], 2.0, notes)
    with pytest.raises(ValueError):
        beats.beat_metrics([], 2.0, notes)


def test_passes_filter_is_strict():
    cfg = default_config()
    at = {"wp_std": 5, "max_beat_fluctuation": 1.2, "max_note_density": 25, "time_diff_ratio": 0.2}
    below = {k: v * 0.999 for k, v in at.items()}
    assert beats.passes_filter(below, cfg) and beats.passes_filter(below)
    for name in at:
        assert not beats.passes_filter(dict(below, **{name: at[name]}), cfg), name       # equality fails: the comparison is strict
        assert not beats.passes_filter({k: v for k, v in below.items() if k != name}, cfg)
        assert not beats.passes_filter(dict(below, **{name: float("nan")}), cfg)
    assert not beats.passes_filter(None, cfg)


def test_filter_pair_and_aligned_beats_on_the_host(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)             # the definition's route, with or without a GPU
    c = case(*CASES[2])                                                        # 30 s, 54 beats: every tenth holds more than two
    wp = np.array([[0.0, 60.0], [0.0, 30.0]])                                  # the recording runs at half the cover's speed
    got = beats.aligned_beats(c["notes"], wp)
    assert np.array_equal(got, 2.0 * beats.track_notes_host(c["notes"]).beat_times)
    aligned = c["notes"].copy()
    aligned[:, :2] *= 2.0
    result = align.AlignResult(aligned, wp, 0, 0, {"wp_std": 1.0, "time_diff_ratio": 0.01})
    metrics, ok = beats.filter_pair(result, c["notes"], 60.0)
    print(metrics)
    assert set(metrics) == {"wp_std", "time_diff_ratio", "max_beat_fluctuation", "max_note_density"} and ok
    assert metrics == beats.filter_metrics(result, c["notes"], 60.0)
    assert beats.filter_pair(result, c["notes"][:1], 60.0) == (None, False)    # one onset: too few beats, the filter fails


# ------------------------------------------------------------------ the grid
def test_quantize_by_hand():
    grid = [1.0, 1.5, 2.1]
    notes = np.array([[1.27, 1.3, 60, 80], [0.1, 1.9, 61, 81], [2.45, 2.5, 62, 82], [1.374, 1.376, 63, 83], [1.375, 2.0, 64, 84]])
    got = beats.quantize(notes, grid, 2)
    # two points per beat: ... 0.5, 0.75, 1.0, 1.25, 1.5, 1.8, 2.1, 2.4, 2.7 (the first and the last interval go on outside the beats)
    want = [[1.25, 1.5], [0.0, 1.8], [2.4, 2.7], [1.25, 1.5], [1.5, 2.1]]
    assert got.dtype == np.float64 and np.allclose(got[:, :2], want, atol=1e-12) and np.array_equal(got[:, 2:], notes[:, 2:])
    assert np.allclose(beats.quantize(notes[:1], grid, 1)[:, :2], [[1.5, 2.1]])         # halves round up; the offset one step on
    assert np.allclose(beats.grid_times(beats.grid_positions([0.3, 1.2, 1.9, 5.0], grid), grid), [0.3, 1.2, 1.9, 5.0])
    for bad in ([1.0], [1.0, 1.0], [2.0, 1.0]):
        with pytest.raises(ValueError):
            beats.quantize(notes, bad)
    with pytest.raises(ValueError):
        beats.quantize(notes, grid, 0)


# ------------------------------------------------------------------ the file
def read_midi(path):
    """(format, resolution, tracks); a track is a list of (tick, kind, data): 'tempo' microseconds, 'on' / 'off' (channel, pitch,
    velocity), 'meta' type.  No running status: SimpleMIDI.write uses none."""
    raw = Path(path).read_bytes()
    assert raw[:4] == b"MThd" and struct.unpack(">I", raw[4:8])[0] == 6
    fmt, n_tracks, resolution = struct.unpack(">HHH", raw[8:14])
    at, tracks = 14, []
    for _ in range(n_tracks):
        assert raw[at:at + 4] == b"MTrk"
        end = at + 8 + struct.unpack(">I", raw[at + 4:at + 8])[0]
        at, tick, events = at + 8, 0, []
        while at < end:
            delta = 0
            while True:
                delta, more, at = (delta << 7) | (raw[at] & 0x7F), raw[at] & 0x80, at + 1
                if not more:
                    break
            tick += delta
            status = raw[at]
            if status == 0xFF:
                kind, length = raw[at + 1], raw[at + 2]
                body = raw[at + 3:at + 3 + length]
                events.append((tick, "tempo", int.from_bytes(body, "big")) if kind == 0x51 else (tick, "meta", kind))
                at += 3 + length
            elif status & 0xF0 == 0xC0:
                at += 2
            else:
                assert status & 0xF0 in (0x80, 0x90), hex(status)
                events.append((tick, "on" if status & 0xF0 == 0x90 else "off", (status & 0xF, raw[at + 1], raw[at + 2])))
                at += 3
        assert at == end and events[-1][1:] == ("meta", 0x2F)
        tracks.append(events)
    return fmt, resolution, tracks


def seconds_of(tick, tempi, resolution):
    """The time of a tick under the set-tempo events (tick, microseconds)."""
    t, last, us = 0.0, 0, 500000
    for at, value in tempi:
        if at >= tick:
            break
        t, last, us = t + (at - last) * us / 1e6 / resolution, at, value
    return t + (tick - last) * us / 1e6 / resolution


NOTES = np.array([[0.0, 0.5, 60, 80], [0.26, 1.3, 64, 90], [1.0, 1.25, 67, 1], [2.123, 3.5, 72, 127], [2.123, 2.2, 48, 64]])


@pytest.mark.parametrize("first", (0.5, 0.0))
def test_tempo_mapped_file_read_back(tmp_path, first):
    grid = np.array([0.5, 1.0, 1.6, 2.1]) - (0.5 - first)
    midi = simple_midi(NOTES)
    assert midi.beat_times is None
    midi.beat_times = grid
    midi.write(tmp_path / "grid.mid")
    fmt, res, tracks = read_midi(tmp_path / "grid.mid")
    assert fmt == 0 and res == 384 and len(tracks) == 1
    tempi = [(t, v) for t, kind, v in tracks[0] if kind == "tempo"]
    lead = 0 if first == 0 else 1
    spans = ([first] if lead else []) + [0.5, 0.6, 0.5, 0.5]                   # the span before the first beat; the last interval goes on
    assert tempi == [(k * 384, round(1e6 * s)) for k, s in enumerate(spans)]
    for k, b in enumerate(grid):                                               # beat k at tick (k + 1) * resolution, or k * resolution
        assert abs(seconds_of((k + lead) * 384, tempi, res) - b) < 1e-9
    ons = sorted((seconds_of(t, tempi, res), d[1]) for t, kind, d in tracks[0] if kind == "on")
    offs = sorted((seconds_of(t, tempi, res), d[1]) for t, kind, d in tracks[0] if kind == "off")
    tick = 0.6 / 384                                                           # the longest tick of the map
    assert [p for _, p in ons] == [60, 64, 67, 48, 72] or [p for _, p in ons] == [60, 64, 67, 72, 48]
    for (got, pitch), want in zip(ons, sorted(zip(NOTES[:, 0], NOTES[:, 2]))):
        assert abs(got - want[0]) <= tick and pitch == want[1]
    for (got, pitch), want in zip(offs, sorted(zip(NOTES[:, 1], NOTES[:, 2]))):
        assert abs(got - want[0]) <= tick and pitch == want[1]


def test_tempo_map_with_two_instruments_and_its_refusals(tmp_path):
    midi = SimpleMIDI()
    for i, (prog, name) in enumerate(((0, "Piano"), (40, "Violin"))):
        inst = SimpleInstrument(prog, name)
        inst.notes = [SimpleNote(*r) for r in NOTES[i::2]]
        midi.instruments.append(inst)
    midi.beat_times = [0.5, 1.0, 1.6]
    midi.write(tmp_path / "two.mid")
    fmt, res, tracks = read_midi(tmp_path / "two.mid")
    assert fmt == 1 and len(tracks) == 3
    assert [e for e in tracks[0] if e[1] == "tempo"] == [(0, "tempo", 500000), (384, "tempo", 500000), (768, "tempo", 600000), (1152, "tempo", 600000)]
    assert not any(kind == "tempo" for track in tracks[1:] for _, kind, _ in track)
    assert sum(kind == "on" for _, kind, _ in tracks[1]) == 3 and sum(kind == "on" for _, kind, _ in tracks[2]) == 2
    for bad in ([0.0, 17.0], [1.0, 1.0, 2.0], [2.0, 1.0], [-0.5, 0.5], [0.0, float("nan")], [0.0, 1e-7]):
        midi.beat_times = bad
        with pytest.raises(ValueError):
            midi.write(tmp_path / "bad.mid")
    midi.beat_times = [0.0, 16.7]                                              # 16.7 s fit the 24 bits
    midi.write(tmp_path / "slow.mid")


def test_write_without_beat_times_gives_the_bytes_it_gave(tmp_path):
    """tests/golden/beats/*.mid were written by the parent commit's SimpleMIDI.write from NOTES."""
    midi = numpy_to_midi(NOTES)
    if not isinstance(midi, SimpleMIDI):
        midi = simple_midi(NOTES)
    midi.write(tmp_path / "one.mid")
    assert (tmp_path / "one.mid").read_bytes() == (GOLDEN / "plain_one_track.mid").read_bytes()
    midi.beat_times = [1.0]                                                    # fewer than two beats: no map
    midi.write(tmp_path / "one_beat.mid")
    assert (tmp_path / "one_beat.mid").read_bytes() == (GOLDEN / "plain_one_track.mid").read_bytes()
    two = SimpleMIDI()
    for i, (prog, name) in enumerate(((0, "Piano"), (40, "Violin"))):
        inst = SimpleInstrument(prog, name)
        inst.notes = [SimpleNote(*r) for r in NOTES[i::2]]
        two.instruments.append(inst)
    two.write(tmp_path / "two.mid")
    assert (tmp_path / "two.mid").read_bytes() == (GOLDEN / "plain_two_tracks.mid").read_bytes()


# ------------------------------------------------------------------ the C ABI
def test_binding_matches_the_header():
    lib = native.load()
    header = (native._LIB_PATH.parents[2] / "include" / "music2midi_amd.h").read_text()
    for name in ("m2m_beat_envelope", "m2m_beat_track_workspace_bytes", "m2m_beat_track"):
        assert name in native.EXPORTED_SYMBOLS and hasattr(lib, name) and f" {name}(" in header, name
        decl = header[header.index(f"\nint{'64_t' if 'bytes' in name else ''} {name}("):]
        decl = decl[:decl.index(";")]
        assert decl.count(",") + 1 == len(native._SIGNATURES[name][1]), name
    assert C.sizeof(native.BeatClip) == 16 and [n for n, _ in native.BeatClip._fields_] == ["env_offset", "frames", "period", "beat_offset"]
    for name, value in (("MAX_FRAMES", beats.MAX_FRAMES), ("LAG_MIN", beats.LAG_MIN), ("LAG_MAX", beats.LAG_MAX), ("HALF", beats.H),
                        ("ENV_MAX", beats.ENV_MAX)):
        assert f"#define M2M_BEAT_{name} {value} " in header, name
    assert float(align.D_THRESH[3]).hex() == "0x1.7f74280000000p+1"            # the literal csrc/beats.hip writes out


def _bytes(frames):
    f = np.asarray(frames, np.int32)
    return native.load().m2m_beat_track_workspace_bytes(f.ctypes.data_as(C.c_void_p), len(f))


def test_workspace_bytes_and_its_refusals():
    # the clip table (256 bytes for up to 16 clips), then four bytes per frame, rounded up to 256
    assert _bytes([1]) == 256 + 256 and _bytes([64]) == 512 and _bytes([65]) == 256 + 512
    assert _bytes([32768]) == 256 + 4 * 32768 and _bytes([1, 4097, 17]) == 256 + 16640
    assert _bytes([5] * 17) == 512 + 512
    for frames in ([0], [32769], [5, -1]):
        assert _bytes(frames) == M2M_ERR_INVALID, frames
        assert b"m2m_beat_track_workspace_bytes" in native.load().m2m_last_error()
    assert native.load().m2m_beat_track_workspace_bytes(None, 1) == M2M_ERR_INVALID
    assert native.load().m2m_beat_track_workspace_bytes(np.zeros(1, np.int32).ctypes.data_as(C.c_void_p), 0) == M2M_ERR_INVALID


def test_every_refusal_is_made_without_a_gpu():
    """M2M_ERR_INVALID on the arguments alone: the pointers are never dereferenced, no HIP call is made."""
    lib = native.load()
    buf = (C.c_float * 8192)()
    a = (C.addressof(buf) + 255) // 256 * 256                                  # never touched: only compared
    ok = dict(env=a, n_env=500, clips=((0, 300, 0, 0), (300, 200, 25, 39)), n=2, prior=a + 1024, pen=a + 2048, default=25, ws=a + 4096, wsb=1 << 20,
              P=a + 8192, score=a + 8200, beats=a + 12288, cap=66, count=a + 16384)

    def call(**change):
        k = dict(ok, **change)
        clips = None if k["clips"] is None else (native.BeatClip * len(k["clips"]))(*[native.BeatClip(*c) for c in k["clips"]])
        return lib.m2m_beat_track(k["env"], k["n_env"], clips, k["n"], k["prior"], k["pen"], k["default"], k["ws"], k["wsb"], k["P"], k["score"],
                                  k["beats"], k["cap"], k["count"], None)
    bad = [dict(n=0), dict(n=65536), dict(n_env=0), dict(n_env=499), dict(n_env=(1 << 26) + 1), dict(default=14), dict(default=101),
           dict(clips=((0, 0, 0, 0), (300, 200, 25, 39))), dict(clips=((0, 32769, 0, 0), (300, 200, 25, 39)), n_env=40000, cap=5000),
           dict(clips=((-1, 300, 0, 0), (300, 200, 25, 39))), dict(clips=((0, 300, 14, 0), (300, 200, 25, 39))),
           dict(clips=((0, 300, 101, 0), (300, 200, 25, 39))), dict(clips=((0, 300, -1, 0), (300, 200, 25, 39))),
           dict(clips=((0, 300, 0, 0), (300, 200, 25, 38))), dict(clips=((0, 300, 0, -1), (300, 200, 25, 39))), dict(cap=65), dict(cap=0),
           dict(cap=1 << 31), dict(env=None), dict(clips=None), dict(prior=None), dict(pen=None), dict(ws=None), dict(P=None), dict(beats=None),
           dict(count=None), dict(env=a + 2), dict(prior=a + 1025), dict(ws=a + 4100), dict(score=a + 8196), dict(beats=a + 12289)]
    for change in bad:
        assert call(**change) == M2M_ERR_INVALID, change
        assert b"m2m_beat_track" in lib.m2m_last_error(), change
    assert call(wsb=2000) == -3 and b"needed" in lib.m2m_last_error()        # M2M_ERR_NOMEM: 256 + 2048 are needed
    for args in ((a, a + 1024, 0, 5, 5, a + 2048, None), (a, a + 1024, 65536, 5, 5, a + 2048, None), (a, a + 1024, 1, 6, 5, a + 2048, None),
                 (a, a + 1024, 1, 0, 5, a + 2048, None), (a, a + 1024, 1, 5, 0, a + 2048, None), (a, a + 1024, 1, 5, (1 << 26) + 1, a + 2048, None),
                 (None, a + 1024, 1, 5, 5, a + 2048, None), (a, None, 1, 5, 5, a + 2048, None), (a, a + 1024, 1, 5, 5, None, None),
                 (a + 2, a + 1024, 1, 5, 5, a + 2048, None), (a, a + 1024, 1, 5, 5, a + 2049, None)):
        assert lib.m2m_beat_envelope(*args) == M2M_ERR_INVALID, args
        assert b"m2m_beat_envelope" in lib.m2m_last_error(), args


def test_host_layer_refusals_without_a_gpu():
    with pytest.raises(ValueError, match="1025"):
        beats.track_host(np.zeros(1024, np.float32))
    with pytest.raises(ValueError):
        beats.tempo_score(np.zeros(40), prior=np.zeros(100, np.int32))
    with pytest.raises(ValueError):
        beats.track_envelope_host(np.zeros(40, np.int32), table=-beats.penalty_table())
    with pytest.raises(ValueError):
        beats.note_envelope(np.zeros((1, 4)), 0)
    silent = beats.track_host(np.zeros(4000, np.float32))
    assert silent.period == 25 and silent.bpm == 120.0 and len(silent.beat_times) == 0 and silent.score.shape == (101,)
    bad = np.zeros(8000, np.float32)
    bad[100] = np.inf
    assert isinstance(beats.track_host(bad), beats.BeatResult)                 # audio that is not finite still gets an answer


# ------------------------------------------------------------------ the quality of the definition
@pytest.mark.parametrize("spec", CASES, ids=lambda s: f"seed{s[0]}-{int(s[1])}bpm-{int(s[3])}s")
def test_definition_finds_the_planted_beats(spec):
    c = case(*spec)
    for what, r in (("audio", beats.track_host(c["audio"])), ("notes", beats.track_notes_host(c["notes"], c["frames"]))):
        f = f_measure(r.beat_times, c["beats"])
        print(f"{spec} {what}: P {r.period} ({r.bpm:.1f} BPM), {len(r.beat_times)} beats for {len(c['beats'])}, F {f:.3f}")
        assert isinstance(r, beats.BeatResult) and r.beat_frames.dtype == np.int32 and np.array_equal(r.beat_times, r.beat_frames / 50.0)
        assert period_ok(r.period, c["bpm"])
        assert f >= F_CAP


def test_limit_case_is_a_documented_limit():
    """72 BPM, outside the range the prior keeps at its own metrical level: the case exists and runs, nothing is asserted about it."""
    c = case(*LIMIT_CASE)
    for what, r in (("audio", beats.track_host(c["audio"])), ("notes", beats.track_notes_host(c["notes"], c["frames"]))):
        print(f"limit {what}: P {r.period} ({r.bpm:.1f} BPM for 72), F {f_measure(r.beat_times, c['beats']):.3f}")
        assert isinstance(r, beats.BeatResult)
