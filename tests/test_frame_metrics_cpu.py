"""CPU: the definition of the frame-level metrics (music2midi_amd.frame_metrics) on hand-worked inputs; the multi-track
``SimpleMIDI.write``; and what the device form (scoring.frame_counts / error_notes, csrc/frame_roll.hip) decides without a device - the
header against the binding and every refusal of its entry points - and the host route of ``Music2MIDI``'s frame methods for ids that
are not on a GPU."""
import ctypes as C
import struct
from pathlib import Path

import numpy as np
import pytest
import torch

import frame_metrics_cases as fc
from music2midi_amd import evaluation, frame_metrics, native, note_metrics, scoring
from music2midi_amd.utils import SimpleInstrument, SimpleMIDI, SimpleNote, numpy_to_midi

ROOT = Path(__file__).resolve().parents[1]
FAKE = 0x100000                          # a device address that is never dereferenced: every refusal comes first
TOK = fc.TOK


# ------------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("name", list(fc.CRAFTED))
def test_crafted_cases_have_the_stated_counts_and_notes(name):
    labels, decoded, counts, lists = fc.CRAFTED[name]
    est = fc.est_seconds(decoded)
    assert np.array_equal(TOK.decode(fc.id_rows([decoded], 24))[0], est)      # the id rows of the GPU test decode to these notes
    got = frame_metrics.frame_counts(labels, est)
    assert got == counts and all(type(v) is int for v in got)
    rolls = frame_metrics.error_rolls(labels, est)
    assert all(r.dtype == bool and r.shape == rolls[0].shape and r.shape[0] == 128 for r in rolls)
    assert tuple(int(r.sum()) for r in rolls) == counts[:3]
    for roll, want in zip(rolls, lists):
        notes = frame_metrics.roll_to_notes(roll)
        assert notes.dtype == np.float64 and np.array_equal(notes, fc.note_list(want)), (name, notes, want)
    melody = frame_metrics.error_rolls(labels, est, melody_only=True)
    assert all(r.shape == (12, rolls[0].shape[1]) for r in melody) and tuple(int(r.sum()) for r in melody) == counts[3:]
    if name in fc.CRAFTED_MELODY:
        for roll, want in zip(melody, fc.CRAFTED_MELODY[name]):
            assert np.array_equal(frame_metrics.roll_to_notes(roll), fc.note_list(want)), name
    # MIDI objects are taken as the arrays are
    assert frame_metrics.frame_counts(numpy_to_midi(labels), numpy_to_midi(est)) == counts


def test_definition_details():
    # both sides empty: no frames at all
    rolls = frame_metrics.error_rolls(fc.ref(), fc.ref())
    assert all(r.shape == (128, 0) for r in rolls) and frame_metrics.roll_to_notes(rolls[0]).shape == (0, 4)
    assert all(r.shape == (12, 0) for r in frame_metrics.error_rolls(fc.ref(), fc.ref(), melody_only=True))
    # notes with end <= start do not exist: not in the rolls, not in n_frames
    with_dead = fc.ref((0.0, 0.5, 60), (3.0, 3.0, 62), (9.0, 2.0, 64))
    assert frame_metrics.n_frames_of(with_dead, fc.ref()) == 50
    assert frame_metrics.frame_counts(with_dead, fc.ref((0.0, 0.5, 60))) == (49, 0, 0, 49, 0, 0)
    # sounding is piano_roll != 0, the last frame silent
    roll = frame_metrics.sounding(fc.ref((0.0, 0.1, 60), (0.05, 0.1, 60)), 10)
    assert roll.dtype == bool and roll.shape == (128, 10) and roll[60].tolist() == [True] * 9 + [False] and roll.sum() == 9
    assert np.array_equal(roll, evaluation.piano_roll(fc.ref((0.0, 0.1, 60), (0.05, 0.1, 60)), 10) != 0)
    # the melody roll: the class of the highest pitch, nothing in a silent frame
    full = np.zeros((128, 4), dtype=bool)
    full[[60, 67], 0] = True
    full[127, 1] = True
    full[0, 3] = True
    mel = frame_metrics.melody_roll(full)
    assert mel.shape == (12, 4) and mel.dtype == bool and mel.sum() == 3 and mel[7, 0] and mel[127 % 12, 1] and mel[0, 3]
    top = evaluation.highest_pitches(full.astype(np.float64))
    assert top.tolist() == [67, 127, -1, 0]
    # roll_to_notes: runs at both borders of the roll, one float64 division per time
    edge = np.zeros((3, 7), dtype=bool)
    edge[0, :2] = edge[2, 5:] = edge[1, 3] = True
    assert np.array_equal(frame_metrics.roll_to_notes(edge), fc.note_list([(0.0, 0.02, 0), (0.03, 0.04, 1), (0.05, 0.07, 2)]))
    assert frame_metrics.roll_to_notes(edge)[2, 1] == 7 / 100


def test_frame_edges_are_the_float64_products():
    """``x * 100`` in float64 is below the decimal reading for these times: the frame is one below it, at a start and at an end."""
    times = [0.29, 0.57, 1.13, 2.3, 4.35, 8.2]
    below = [28, 56, 112, 229, 434, 819]
    assert [int(t * 100) for t in times] == below and 0.29 * 100 == 28.999999999999996 and 0.07 * 100 == 7.000000000000001
    assert int(0.07 * 100) == 7
    for t, frame in zip(times, below):
        as_end = frame_metrics.sounding(fc.ref((0.0, t, 60), (0.0, 9.0, 0)), 900)
        as_start = frame_metrics.sounding(fc.ref((t, 9.0, 60)), 900)
        assert as_end[60].sum() == frame and not as_end[60, frame] and as_end[60, frame - 1]
        assert as_start[60, frame] and not as_start[60, frame - 1]
        notes = frame_metrics.roll_to_notes(frame_metrics.error_rolls(fc.ref((0.0, t, 60), (0.0, 9.0, 0)), fc.ref())[1])
        assert notes[0].tolist() == [0.0, frame / 100, 60.0, 1.0]
    # n_frames: 0.07 / 0.01 = 7.000000000000001 -> 8 frames, not 7
    assert frame_metrics.n_frames_of(fc.ref((0.0, 0.07, 60)), fc.ref()) == 8 == len(np.arange(0, 0.07, 1 / 100))


def test_scores_are_precision_recall_f1_of_the_counts():
    prf = note_metrics.precision_recall_f1
    z = np.zeros((2, 2), dtype=np.int64)
    c = scoring.FrameCounts(np.array([[3, 0], [1, 0]]), np.array([[1, 2], [1, 0]]), np.array([[0, 0], [2, 5]]),
                            np.array([[2, 0], [0, 0]]), np.array([[0, 1], [0, 1]]), z, np.array([10, 20]))
    assert c.precision.tolist() == [4 / 6, 0.0] and c.recall.tolist() == [4 / 6, 0.0] and c.f1.tolist() == [prf(4, 6, 6)[2], 0.0]
    assert c.melody_precision.tolist() == [1.0, 0.0] and c.melody_recall.tolist() == [1.0, 0.0] and c.melody_f1.tolist() == [1.0, 0.0]
    assert c.per_timeline_f1.tolist() == [[prf(3, 4, 3)[2], 0.0], [prf(1, 2, 3)[2], 0.0]] and c.f1.dtype == np.float64
    d = evaluation.frame_scores(c.tp, c.fn, c.fp, c.melody_tp, c.melody_fn, c.melody_fp)
    assert set(d) == {p + k for p in ("", "melody_") for k in ("precision", "recall", "f1", "tp", "fn", "fp")}
    assert d["tp"].tolist() == [4, 0] and d["fn"].tolist() == [2, 2] and d["fp"].tolist() == [2, 5] and d["tp"].dtype == np.int64
    assert np.array_equal(d["f1"], c.f1) and np.array_equal(d["melody_recall"], c.melody_recall) and d["melody_fn"].tolist() == [0, 2]
    assert set(evaluation.frame_scores(c.tp, c.fn, c.fp)) == {"precision", "recall", "f1", "tp", "fn", "fp"}


def test_frame_scores_host_is_the_definition_per_threshold():
    names = list(fc.CRAFTED)
    ids = fc.id_rows([fc.CRAFTED[n][1] for n in names], 24)
    labels = [fc.CRAFTED[n][0] for n in names]
    got = evaluation.frame_scores_host(TOK, ids, labels, thresholds=[0.0, -1.0])
    sums = np.sum([fc.CRAFTED[n][2] for n in names], axis=0)
    for i, key in enumerate(("tp", "fn", "fp", "melody_tp", "melody_fn", "melody_fp")):
        assert got[key].tolist() == [sums[i]] * 2, key
    p, r, f = note_metrics.precision_recall_f1(sums[0], sums[0] + sums[1], sums[0] + sums[2])
    assert (got["precision"][0], got["recall"][0], got["f1"][0]) == (p, r, f)
    with pytest.raises(ValueError, match="need token_logprobs"):
        evaluation.frame_scores_host(TOK, ids, labels, thresholds=[0.5])
    import music2midi.evaluation as drop_in
    assert drop_in.frame_scores_tokens is evaluation.frame_scores_tokens and drop_in.evaluate_midi_result is evaluation.evaluate_midi_result


# ------------------------------------------------------------------------------------------------ MIDI objects and files
def test_evaluate_midi_result_has_the_three_instruments():
    labels, decoded, _, lists = fc.CRAFTED["half overlap"]
    for target, predict in ((labels, fc.est_seconds(decoded)), (numpy_to_midi(labels), numpy_to_midi(fc.est_seconds(decoded)))):
        midi = evaluation.evaluate_midi_result(target, predict)
        assert [(i.name, i.program) for i in midi.instruments] == [("TP", 0), ("FN", 1), ("FP", 2)]
        for inst, want in zip(midi.instruments, lists):
            assert [(n.start, n.end, n.pitch, n.velocity) for n in inst.notes] == [(s, e, p, 1) for s, e, p in want]
    labels, decoded, _, _ = fc.CRAFTED["melody top changes mid-note"]
    midi = frame_metrics.evaluate_midi_result(labels, fc.est_seconds(decoded), melody_only=True)
    for inst, want in zip(midi.instruments, fc.CRAFTED_MELODY["melody top changes mid-note"]):
        assert [(n.start, n.end, n.pitch) for n in inst.notes] == want
    assert midi.get_end_time() == 1.99


def _parse_midi(data: bytes):
    """(format, division, tracks): per track the list of (tick, event) with event a (status, a, b) tuple, ("program", channel,
    program) or ("meta", type, payload)."""
    assert data[:4] == b"MThd" and struct.unpack(">I", data[4:8])[0] == 6
    fmt, n_tracks, division = struct.unpack(">HHH", data[8:14])
    pos, tracks = 14, []
    for _ in range(n_tracks):
        assert data[pos:pos + 4] == b"MTrk"
        end = pos + 8 + struct.unpack(">I", data[pos + 4:pos + 8])[0]
        pos, tick, events = pos + 8, 0, []
        while pos < end:
            delta = 0
            while True:
                delta, more, pos = delta << 7 | data[pos] & 0x7F, data[pos] & 0x80, pos + 1
                if not more:
                    break
            tick += delta
            if data[pos] == 0xFF:
                length = data[pos + 2]
                events.append((tick, ("meta", data[pos + 1], data[pos + 3:pos + 3 + length])))
                pos += 3 + length
            elif data[pos] & 0xF0 == 0xC0:
                events.append((tick, ("program", data[pos] & 0x0F, data[pos + 1])))
                pos += 2
            else:
                events.append((tick, (data[pos], data[pos + 1], data[pos + 2])))
                pos += 3
        assert pos == end and events[-1][1] == ("meta", 0x2F, b"")
        tracks.append(events)
    assert pos == len(data)
    return fmt, division, tracks


def test_simple_midi_write_one_instrument_is_format_0(tmp_path):
    midi = SimpleMIDI(resolution=384, initial_tempo=120.0)
    midi.instruments.append(SimpleInstrument(program=0, name="Piano"))
    midi.instruments[0].notes = [SimpleNote(0.5, 1.0, 60, 80)]
    midi.write(tmp_path / "one.mid")
    # 384 ticks per quarter at 120 bpm: 768 ticks per second; 0.5 s = 384 = VLQ 83 00
    want = (b"MThd" + bytes([0, 0, 0, 6, 0, 0, 0, 1, 0x01, 0x80]) + b"MTrk" + bytes([0, 0, 0, 24])   # 7 + 3 + 5 + 5 + 4 bytes of track data
            + bytes([0x00, 0xFF, 0x51, 0x03, 0x07, 0xA1, 0x20])        # tempo 500000 us per quarter
            + bytes([0x00, 0xC0, 0x00])                                # program 0
            + bytes([0x83, 0x00, 0x90, 60, 80])                        # note on at tick 384
            + bytes([0x83, 0x00, 0x80, 60, 0])                         # note off 384 ticks later
            + bytes([0x00, 0xFF, 0x2F, 0x00]))
    assert (tmp_path / "one.mid").read_bytes() == want
    fmt, division, tracks = _parse_midi(want)
    assert (fmt, division, len(tracks)) == (0, 384, 1)
    SimpleMIDI().write(tmp_path / "none.mid")                          # no instrument: an empty format-0 file, as before
    assert _parse_midi((tmp_path / "none.mid").read_bytes())[0] == 0


def test_simple_midi_write_three_instruments_is_format_1(tmp_path):
    midi = SimpleMIDI()
    for program, (name, notes) in enumerate((("TP", [(0.5, 1.0, 60)]), ("FN", [(0.0, 0.25, 62), (0.25, 0.5, 64)]), ("FP", []))):
        inst = SimpleInstrument(program=program, name=name)
        inst.notes = [SimpleNote(s, e, p, 1) for s, e, p in notes]
        midi.instruments.append(inst)
    midi.write(tmp_path / "three.mid")
    fmt, division, tracks = _parse_midi((tmp_path / "three.mid").read_bytes())
    assert (fmt, division, len(tracks)) == (1, 384, 4)
    assert tracks[0] == [(0, ("meta", 0x51, bytes([0x07, 0xA1, 0x20]))), (0, ("meta", 0x2F, b""))]
    assert tracks[1] == [(0, ("meta", 0x03, b"TP")), (0, ("program", 0, 0)), (384, (0x90, 60, 1)), (768, (0x80, 60, 0)),
                         (768, ("meta", 0x2F, b""))]
    assert tracks[2] == [(0, ("meta", 0x03, b"FN")), (0, ("program", 1, 1)), (0, (0x91, 62, 1)), (192, (0x81, 62, 0)), (192, (0x91, 64, 1)),
                         (384, (0x81, 64, 0)), (384, ("meta", 0x2F, b""))]
    assert tracks[3] == [(0, ("meta", 0x03, b"FP")), (0, ("program", 2, 2)), (0, ("meta", 0x2F, b""))]
    # the channel wraps at 16
    many = SimpleMIDI()
    many.instruments = [SimpleInstrument(program=i, name=f"i{i}") for i in range(18)]
    many.write(tmp_path / "many.mid")
    _, _, tracks = _parse_midi((tmp_path / "many.mid").read_bytes())
    assert len(tracks) == 19 and tracks[17][1] == (0, ("program", 0, 16)) and tracks[18][1] == (0, ("program", 1, 17))


# ------------------------------------------------------------------------------------------------ header, binding, refusals
def test_header_declares_what_the_binding_binds():
    header = (ROOT / "include" / "music2midi_amd.h").read_text()
    for name, proto in [
            ("m2m_score_frame_counts", "int m2m_score_frame_counts(const int32_t* notes_dev, const int32_t* counts_dev, const float* note_lp_dev, "
                                       "int R, int L, int sequential,"),
            ("m2m_score_error_notes", "int m2m_score_error_notes(const int32_t* notes_dev, const int32_t* counts_dev, const float* note_lp_dev, "
                                      "int R, int L, int sequential,"),
            ("m2m_score_error_notes_capacity", "int m2m_score_error_notes_capacity(int R, int L, int sequential, int max_timeline_labels, "
                                               "int melody_only);"),
            ("m2m_score_error_notes_workspace_bytes", "int64_t m2m_score_error_notes_workspace_bytes(int n_timelines, int frame_cap, "
                                                      "int melody_only);")]:
        assert proto in header, name
        assert name in native.EXPORTED_SYMBOLS and hasattr(native.load(), name)
    assert header.index("int m2m_score_note_counts(") < header.index("int m2m_score_frame_counts(") \
        < header.index("int m2m_score_error_notes(") < header.index("Audio ingest")
    assert f"#define M2M_SCORE_FRAME_TILE {scoring.FRAME_TILE}" in header and scoring.FRAME_TILE % 32 == 0
    args = native._SIGNATURES["m2m_score_frame_counts"][1]
    assert len(args) == 17 and [i for i, a in enumerate(args) if a is C.c_double] == [6]
    args = native._SIGNATURES["m2m_score_error_notes"][1]
    assert len(args) == 20 and [i for i, a in enumerate(args) if a is C.c_double] == [6] and args[12] is C.c_float and args[16] is C.c_int64
    lib = native.load()
    tile_words = scoring.FRAME_TILE // 32
    for T, cap, melody in ((1, 1, 0), (5, scoring.FRAME_TILE, 1), (3, scoring.FRAME_TILE + 1, 0), (128, 24000, 0), (1, 1 << 22, 1)):
        tiles, rows, up = -(-cap // scoring.FRAME_TILE), 12 if melody else 128, lambda n: (n + 7) // 8 * 8
        assert lib.m2m_score_error_notes_workspace_bytes(T, cap, melody) == up(4 * T) + up(12 * T * tiles) + 4 * T * 3 * rows * tiles * tile_words
    for bad in ((0, 1, 0), (65536, 1, 0), (1, 0, 0), (1, (1 << 22) + 1, 0), (1, 1, 2)):
        assert lib.m2m_score_error_notes_workspace_bytes(*bad) == -1
    # the capacity: N_ref + N_est runs per kind, twice that on the melody roll
    assert lib.m2m_score_error_notes_capacity(4, 64, 0, 10, 0) == 74 and lib.m2m_score_error_notes_capacity(4, 64, 0, 10, 1) == 148
    assert lib.m2m_score_error_notes_capacity(4, 64, 1, 10, 0) == 266 and lib.m2m_score_error_notes_capacity(1, 1, 0, 0, 0) == 1
    for bad in ((0, 1, 0, 0, 0), (1, 2049, 0, 0, 0), (1, 1, 2, 0, 0), (1, 1, 0, -1, 0), (1, 1, 0, (1 << 24) + 1, 0), (1, 1, 0, 0, 2)):
        assert lib.m2m_score_error_notes_capacity(*bad) == -1


def _counts(R=4, L=72, seq=0, ts=0.05, labels=FAKE, offsets=FAKE, n_labels=10, T=None, cap=3000, thr=FAKE, K=3, lp=FAKE, notes=FAKE,
            counts=FAKE, out=FAKE, frames=FAKE):
    lib = native.load()
    T = (1 if seq else R) if T is None else T
    st = lib.m2m_score_frame_counts(notes, counts, lp, R, L, seq, ts, labels, offsets, n_labels, T, cap, thr, K, out, frames, None)
    return st, lib.m2m_last_error().decode()


def _notes(R=4, L=72, seq=0, ts=0.05, labels=FAKE, offsets=FAKE, n_labels=10, T=None, cap=3000, floor=-1.0, melody=0, max_labels=5,
           lp=FAKE, ws=FAKE, ws_bytes=None, notes=FAKE, counts=FAKE, out=FAKE, out_counts=FAKE):
    lib = native.load()
    T = (1 if seq else R) if T is None else T
    if ws_bytes is None:
        ws_bytes = max(8, lib.m2m_score_error_notes_workspace_bytes(max(T, 1), min(max(cap, 1), 1 << 22), melody if melody in (0, 1) else 0))
    st = lib.m2m_score_error_notes(notes, counts, lp, R, L, seq, ts, labels, offsets, n_labels, T, cap, floor, melody, max_labels, ws,
                                   ws_bytes, out, out_counts, None)
    return st, lib.m2m_last_error().decode()


SHARED_REFUSALS = [
    (dict(R=0, T=0), "0 rows out of range"),
    (dict(R=65536), "65536 rows out of range"),
    (dict(L=0), "L=0 out of range"),
    (dict(L=2049), "L=2049 out of range"),
    (dict(seq=2, T=1), "sequential must be 0 or 1"),
    (dict(R=4, T=3), "3 timelines for 4 rows"),
    (dict(R=4, seq=1, T=4), "4 timelines for 4 rows"),
    (dict(ts=0.0), "time_step 0 out of range"),
    (dict(ts=float("nan")), "time_step nan out of range"),
    (dict(n_labels=-1), "-1 label notes out of range"),
    (dict(n_labels=(1 << 24) + 1), "label notes out of range"),
    (dict(cap=0), "frame_cap 0 out of range"),
    (dict(cap=(1 << 22) + 1), "frame_cap 4194305 out of range"),
    (dict(notes=None), "null notes"),
    (dict(counts=None), "null notes"),
    (dict(offsets=None), "null notes"),
    (dict(labels=None, n_labels=3), "null labels"),
]


@pytest.mark.parametrize("kw,msg", SHARED_REFUSALS + [
    (dict(K=0), "0 thresholds out of range"),
    (dict(K=65), "65 thresholds out of range"),
    (dict(out=None), "null notes"),
    (dict(frames=None), "null notes"),
    (dict(lp=None, K=3), "3 thresholds need the notes' log-probabilities"),
    (dict(thr=None, K=1), "null min_logprobs with log-probabilities"),
])
def test_frame_counts_refuses_on_the_arguments_alone(kw, msg):
    st, err = _counts(**kw)
    assert st == -1 and msg in err and "m2m_score_frame_counts" in err, err


@pytest.mark.parametrize("kw,msg", SHARED_REFUSALS + [
    (dict(out=None), "null notes"),
    (dict(out_counts=None), "null notes"),
    (dict(melody=2), "melody_only must be 0 or 1"),
    (dict(max_labels=-1), "max_timeline_labels -1 out of range"),
    (dict(max_labels=(1 << 24) + 1), "max_timeline_labels 16777217 out of range"),
    (dict(floor=float("nan")), "min_logprob is NaN"),
    (dict(lp=None, floor=-1.0), "a threshold needs the notes' log-probabilities"),
    (dict(ws=None), "null or misaligned workspace"),
    (dict(ws=FAKE + 4), "null or misaligned workspace"),
    (dict(ws_bytes=native.load().m2m_score_error_notes_workspace_bytes(4, 3000, 0) - 1), "needed (m2m_score_error_notes_workspace_bytes)"),
])
def test_error_notes_refuses_on_the_arguments_alone(kw, msg):
    st, err = _notes(**kw)
    assert st == -1 and msg in err and "m2m_score_error_notes" in err, err


def test_python_layer_refuses_before_the_library():
    ids = torch.zeros((2, 8), dtype=torch.long)
    two = [np.zeros((0, 4))] * 2
    with pytest.raises(ValueError, match="frame_counts: thresholds=.* need token_logprobs"):
        scoring.frame_counts(TOK, ids, two, thresholds=[0.0, 0.5])
    with pytest.raises(ValueError, match="need token_logprobs"):
        evaluation.frame_scores_tokens(TOK, ids, two, thresholds=[0.3])
    with pytest.raises(ValueError, match="CUDA int64"):
        scoring.frame_counts(TOK, ids, two, thresholds=[0.0, -1.0])
    with pytest.raises(ValueError, match="frame_counts: 65 thresholds out of range"):
        scoring.frame_counts(TOK, ids, two, token_logprobs=torch.zeros((2, 8)), thresholds=[0.5] * 65)
    with pytest.raises(ValueError, match="frame_counts: 0 thresholds out of range"):
        scoring.frame_counts(TOK, ids, two, thresholds=[])
    with pytest.raises(ValueError, match="error_notes: min_confidence=0.5 needs token_logprobs"):
        scoring.error_notes(TOK, ids, two, min_confidence=0.5)
    with pytest.raises(ValueError, match="min_confidence has to be a probability"):
        scoring.error_notes(TOK, ids, two, token_logprobs=torch.zeros((2, 8)), min_confidence=1.5)
    with pytest.raises(ValueError, match="CUDA int64"):
        scoring.error_notes(TOK, ids, two)


def test_label_checks_of_the_python_layer(monkeypatch):
    """The number of label arrays and their eligibility are checked after the detokenise, which needs a device: it is replaced by a
    stand-in that returns the shapes a decode of these ids would have."""
    ids = torch.zeros((2, 8), dtype=torch.long)
    fake = scoring.DeviceNotes(torch.zeros((2, 8, 3), dtype=torch.int32), torch.zeros(2, dtype=torch.int32), "batched", 0.05, 80, 0)
    monkeypatch.setattr(scoring, "detokenize", lambda *a, **k: fake)
    good = np.array([[0.1, 0.5, 60, 80.0]])
    bad = np.array([[0.1, 0.5, 60, 0.5]])
    for call, who in ((scoring.frame_counts, "frame_counts"), (scoring.error_notes, "error_notes")):
        with pytest.raises(ValueError, match=f"{who}: 3 label arrays for 2 timelines"):
            call(TOK, ids, [good] * 3)
        with pytest.raises(ValueError, match=f"{who}: the labels are not eligible for the device path: timeline 1: .*a velocity below 1"):
            call(TOK, ids, [good, bad])


# ------------------------------------------------------------------------------------------------ Music2MIDI without a device
def test_music2midi_methods_take_the_host_route_for_cpu_ids(monkeypatch):
    """``Music2MIDI``'s three frame methods over a stand-in model that "decodes" fixed CPU rows: the definition from the same ids."""
    import copy
    from types import SimpleNamespace

    import confidence_cases as cc
    from music2midi_amd import confidence, model as model_mod
    from music2midi_amd.config import DEFAULT_CONFIG, load_config
    from music2midi_amd.input import ModelInputs
    from music2midi_amd.model import Music2MIDI

    class Host:
        for _name in ("frame_scores_batch", "frame_scores_recording", "error_midi_recording", "_recording_token_ids", "sample_scored_rows",
                      "sample_token_rows", "_segment_chunks", "_padded_segments", "_resolve_audio", "_segment_length", "_device_ingest",
                      "_grammar_kwargs"):
            locals()[_name] = getattr(Music2MIDI, _name)
        device = torch.device("cpu")

        def __init__(self, ids, lp):
            cfg = copy.deepcopy(DEFAULT_CONFIG)
            cfg["inference"] = dict(batch_size=2)
            self.config = load_config(cfg)
            self.ids, self.lp, self.calls, self.next_row = torch.from_numpy(ids), torch.from_numpy(lp), [], 0
            self.model = SimpleNamespace(generate=self._decode, tokenizer=TOK, geometry=SimpleNamespace(pad_token_id=0))

        def _cond_rows(self, n_rows, cond_index):
            return torch.zeros((n_rows, 2), dtype=torch.long)

        def _decode(self, inputs, max_length, **kw):
            self.calls.append(dict(kw, max_length=max_length))
            lo, hi = self.next_row, self.next_row + inputs.input_waveform.shape[0]
            self.next_row = hi % len(self.ids)
            ids = self.ids[lo:hi]
            width = max(2, int((ids != 0).any(0).nonzero().max()) + 1)
            if not kw.get("return_dict_in_generate"):
                return ids[:, :width]
            return SimpleNamespace(sequences=ids[:, :width], logprobs=self.lp[lo:hi, 1:width])

    def same(got, want):
        assert set(got) == set(want) and len(want) == 12
        for name in want:
            assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name

    monkeypatch.setattr(model_mod, "frame_scores_tokens", lambda *a, **k: pytest.fail("the device path was taken for host ids"))
    # a labelled batch
    _, ids, lp = cc.fuzz(2, 64, 0.10, 22)
    ids[:, 0], lp[:, 0] = 0, 0.0
    labels = [TOK.decode(ids)[r][::2] + [0.012, 0.02, 0, 0] for r in range(2)]
    inputs = ModelInputs(input_waveform=torch.zeros(2, 8), notes_batch=tuple(labels), cond_index=None)
    budget = 4 * max(len(l) for l in labels)
    thresholds = [0.0, 0.5, 0.9]
    m = Host(ids, lp)
    same(m.frame_scores_batch(inputs, thresholds=thresholds), evaluation.frame_scores_host(TOK, ids, labels, token_logprobs=lp, thresholds=thresholds))
    assert m.calls == [dict(return_dict_in_generate=True, output_logprobs=True, max_length=budget)]
    plain = Host(ids, lp)
    got = plain.frame_scores_batch(inputs)
    same(got, evaluation.frame_scores_host(TOK, ids, labels))
    assert plain.calls == [dict(max_length=budget)] and got["tp"][0] > 0      # no log-probabilities without a positive threshold
    sums = np.sum([frame_metrics.frame_counts(l, d) for l, d in zip(labels, TOK.decode(ids))], axis=0)
    assert [int(got[k][0]) for k in ("tp", "fn", "fp", "melody_tp", "melody_fn", "melody_fp")] == sums.tolist()
    with pytest.raises(ValueError, match="min_confidence has to be a probability"):
        Host(ids, lp).frame_scores_batch(inputs, thresholds=[0.5, 1.5])
    # a recording of three segments
    _, ids, lp = cc.fuzz(3, 64, 0.10, 21)
    ids[:, 0], lp[:, 0] = 0, 0.0
    audio = np.zeros(int(2.5 * 3 * 16000), dtype=np.float32)
    everything = TOK.decode(ids, mode="sequential", duration_per_batch=3)
    label = everything[::2] + [0.012, 0.02, 0, 0]
    m = Host(ids, lp)
    same(m.frame_scores_recording(label, audio_y=audio, thresholds=[0.0, 0.4]),
         evaluation.frame_scores_host(TOK, ids, label, "sequential", 3, token_logprobs=lp, thresholds=[0.0, 0.4]))
    assert m.calls == [dict(return_dict_in_generate=True, output_logprobs=True, max_length=1024)] * 2
    plain = Host(ids, lp)
    same(plain.frame_scores_recording(label, audio_y=audio), evaluation.frame_scores_host(TOK, ids, label, "sequential", 3))
    assert plain.calls == [dict(max_length=1024)] * 2
    for melody_only in (False, True):
        midi = Host(ids, lp).error_midi_recording(label, audio_y=audio, melody_only=melody_only)
        want = frame_metrics.evaluate_midi_result(label, everything, melody_only)
        assert [(i.name, i.program) for i in midi.instruments] == [("TP", 0), ("FN", 1), ("FP", 2)]
        for a, b in zip(midi.instruments, want.instruments):
            assert [(n.start, n.end, n.pitch) for n in a.notes] == [(n.start, n.end, n.pitch) for n in b.notes]
        assert len(midi.instruments[0].notes) > 0
    kept, _ = confidence.decode_with_confidence(TOK, ids, lp, "sequential", 3, 0.4)
    midi = Host(ids, lp).error_midi_recording(label, audio_y=audio, min_confidence=0.4)
    want = frame_metrics.evaluate_midi_result(label, kept)
    assert [len(i.notes) for i in midi.instruments] == [len(i.notes) for i in want.instruments] and len(kept) < len(everything)
