"""CPU: the definition of per-note confidence (music2midi_amd.confidence) against ``MidiTokenizer.decode`` and against rows whose
six columns per note are written out; the refusals of ``m2m_score_detokenize_scored`` on its arguments alone; the ``Music2MIDI``
paths that need no device (the host fallback, the refusal under beam search, the velocity mapping)."""
import copy
import ctypes as C
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import confidence_cases as cc
from music2midi_amd import confidence, native, scoring
from music2midi_amd.config import DEFAULT_CONFIG, load_config
from music2midi_amd.model import Music2MIDI

ROOT = Path(__file__).resolve().parents[1]
FAKE = 0x100000                          # a device address that is never dereferenced: every refusal comes first
TOK = cc.TOK


# ------------------------------------------------------------------------------------------------ the definition against decode
def _same_notes(got, want):
    return got.dtype == np.float64 and got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("R,L,rate,seed", cc.FUZZ_SETS)
def test_definition_equals_tokenizer_decode_on_fuzz_rows(R, L, rate, seed):
    _, ids, lp = cc.fuzz(R, L, rate, seed)
    want = TOK.decode(ids, mode="batched")
    got, conf = confidence.decode_with_confidence(TOK, ids, lp, mode="batched", min_confidence=0)
    assert len(got) == len(conf) == R
    for g, c, w in zip(got, conf, want):
        assert _same_notes(g, w) and c.dtype == np.float64 and c.shape == (len(w),)
    want_seq = TOK.decode(ids, mode="sequential", duration_per_batch=3)
    got_seq, conf_seq = confidence.decode_with_confidence(TOK, ids, lp, mode="sequential", duration_per_batch=3, min_confidence=0.0)
    assert _same_notes(got_seq, want_seq) and np.array_equal(conf_seq, np.concatenate(conf), equal_nan=True)
    assert got_seq[:, 1].max() > 3.0 * (R - 1)                # the rows were shifted
    # the set is not vacuous: closed notes in at least half the rows, an OFFSET that closes two notes, time that goes backwards
    cols = [confidence.note_columns(TOK, row)[1] for row in ids]
    assert sum(len(w) > 0 for w in want) * 2 >= R
    assert any(len(np.unique(c[:, 5])) < len(c) for c in cols)
    assert any(cc.time_goes_backwards(row) for row in ids)
    # the log-probabilities do not move a note: other values, the same notes
    other, _ = confidence.decode_with_confidence(TOK, ids, np.zeros_like(lp), mode="batched")
    assert all(_same_notes(g, w) for g, w in zip(other, want))
    # the filter keeps a subset in order, and what it keeps is what its rule says
    some, some_conf = confidence.decode_with_confidence(TOK, ids, lp, mode="batched", min_confidence=0.5)
    for r in range(R):
        _, parts = confidence.note_logprobs(TOK, ids[r], lp[r])
        with np.errstate(invalid="ignore"):
            keep = ~((parts[:, 0] + parts[:, 1]) < np.float32(np.log(0.5)))
        assert np.array_equal(some[r], want[r][keep]) and np.array_equal(some_conf[r], conf[r][keep], equal_nan=True)
    assert 0 < sum(len(s) for s in some) < sum(len(w) for w in want)


def test_hand_written_rows_columns_and_sums_by_value():
    ids, lp = cc.hand_batch()
    decoded = TOK.decode(ids, mode="batched")
    for r, (name, (tokens, notes)) in enumerate(cc.HAND_ROWS.items()):
        assert len(tokens) <= 16
        idx, cols = confidence.note_columns(TOK, ids[r])
        assert idx.tolist() == [list(n[:3]) for n in notes], name
        assert cols.tolist() == [list(n[3]) for n in notes], name
        idx2, parts = confidence.note_logprobs(TOK, ids[r], lp[r])
        assert np.array_equal(idx2, idx) and parts.dtype == np.float32 and parts.shape == (len(notes), 2)
        for (_, _, _, c), (on, off) in zip(notes, parts.tolist()):
            assert on == -(c[0] + c[1] + c[2] + 3) / 64 and off == -(c[3] + c[4] + c[5] + 3) / 64, name   # lp[i] = -(i + 1) / 64: exact
        got, conf = confidence.decode_with_confidence(TOK, ids[r:r + 1], lp[r:r + 1])
        assert _same_notes(got[0], decoded[r]), name
        assert conf[0].tolist() == [float(np.exp(np.float64(np.float32(a + b)))) for a, b in parts.tolist()], name
    # a start index shifts both time indices and nothing else
    idx, cols = confidence.note_columns(TOK, ids[0], start_idx=60)
    assert idx.tolist() == [[60, 70, 60], [60, 70, 64]] and cols.tolist() == [[0, 1, 2, 4, 5, 6], [0, 1, 3, 4, 5, 7]]


def test_sum_order_is_time_plus_mode_then_pitch_in_float32():
    """(a + b) + c and a + (b + c) differ for these three values in float32: the definition is the first."""
    tokens = cc.HAND_ROWS["two pitches under one ONSET"][0]
    lp = np.zeros(len(tokens), dtype=np.float32)
    a, b, c = np.float32(-1e-8), np.float32(-1.0), np.float32(1.0)
    lp[0], lp[1], lp[2] = a, b, c                              # time, ONSET, the first pitch
    assert np.float32(np.float32(a + b) + c) != np.float32(a + np.float32(b + c))
    _, parts = confidence.note_logprobs(TOK, tokens, lp)
    assert parts[0, 0] == np.float32(np.float32(a + b) + c) == 0.0 and parts[0, 1] == 0.0


def test_nan_and_minus_inf_under_a_threshold():
    ids, lp = cc.special_batch()
    plain = TOK.decode(ids, mode="batched")
    _, parts = confidence.note_logprobs(TOK, ids[0], lp[0])
    assert parts.view(np.uint32)[0, 0] == cc.NAN_BITS and parts[1, 0] == -np.inf and np.isfinite(parts[:, 1]).all()
    _, shared = confidence.note_logprobs(TOK, ids[2], lp[2])
    assert shared.view(np.uint32)[:, 1].tolist() == [cc.NAN_BITS] * 2 and np.isfinite(shared[:, 0]).all()   # one event, both notes
    for floor, kept0 in [(0.0, [0, 1]), (-1.0, [0, 1]), (1e-30, [0]), (0.5, [0]), (1.0, [0])]:
        notes, conf = confidence.decode_with_confidence(TOK, ids, lp, min_confidence=floor)
        assert np.array_equal(notes[0], plain[0][kept0]), floor          # the NaN total is kept, the -inf total goes
        assert np.isnan(conf[0][0]) and (len(kept0) == 1 or conf[0][1] == 0.0)
        assert np.array_equal(notes[2], plain[2]) and np.isnan(conf[2]).all()
    # the boundary: a threshold equal to a note's own confidence keeps it, the next double above drops it
    _, conf = confidence.decode_with_confidence(TOK, ids[1:2], lp[1:2])
    own = float(conf[0][0])
    assert len(confidence.decode_with_confidence(TOK, ids[1:2], lp[1:2], min_confidence=own)[0][0]) == 2 - (conf[0][1] < own)
    assert confidence.keep_mask(np.array([[-0.25, -0.5]], dtype=np.float32), float(np.exp(-0.75)))[0]
    assert not confidence.keep_mask(np.array([[-0.25, -0.5]], dtype=np.float32), 0.5)[0]
    for bad in (1.0000001, 2, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="min_confidence"):
            confidence.decode_with_confidence(TOK, ids, lp, min_confidence=bad)
    assert confidence.min_logprob(0) == -np.inf and confidence.min_logprob(-3) == -np.inf and confidence.min_logprob(1.0) == 0.0
    assert confidence.min_logprob(0.5).dtype == np.float32 and confidence.min_logprob(0.5) == np.float32(np.log(0.5))
    with pytest.raises(ValueError, match="log-probabilities for"):
        confidence.note_logprobs(TOK, ids[0], lp[0, :-1])
    with pytest.raises(ValueError, match="duration_per_batch is required"):
        confidence.decode_with_confidence(TOK, ids, lp, mode="sequential")
    with pytest.raises(ValueError, match="Invalid argument mode=both"):
        confidence.decode_with_confidence(TOK, ids, lp, mode="both")


# ------------------------------------------------------------------------------------------------ header, binding, refusals
def test_header_declares_what_the_binding_binds():
    header = (ROOT / "include" / "music2midi_amd.h").read_text()
    proto = ("int m2m_score_detokenize_scored(const int64_t* ids_dev, int R, int L, int64_t row_stride, int64_t steps_per_row,\n"
             "                                int pitch_offset, int time_offset, int vocab_size,\n"
             "                                const float* logprobs_dev, int64_t lp_row_stride, float min_logprob,\n"
             "                                int32_t* notes_dev, int32_t* counts_dev, float* note_lp_dev, void* stream);")
    assert proto in header
    name = "m2m_score_detokenize_scored"
    assert name in native.EXPORTED_SYMBOLS and hasattr(native.load(), name)
    res, args = native._SIGNATURES[name]
    assert res is C.c_int and len(args) == 15 and args[9] is C.c_int64 and args[10] is C.c_float
    assert "#define M2M_ABI_VERSION 1" in header and native.load().m2m_abi_version() == 1


def _scored(R=4, L=72, stride=None, steps=0, po=5, to=133, V=400, ids=FAKE, lp=FAKE, lp_stride=None, floor=-1.0, notes=FAKE, counts=FAKE,
            note_lp=FAKE):
    lib = native.load()
    st = lib.m2m_score_detokenize_scored(ids, R, L, L if stride is None else stride, steps, po, to, V, lp, L if lp_stride is None else lp_stride,
                                         floor, notes, counts, note_lp, None)
    return st, lib.m2m_last_error().decode()


@pytest.mark.parametrize("kw,msg", [
    (dict(R=0), "0 rows out of range"),
    (dict(R=65536), "65536 rows out of range"),
    (dict(L=0), "L=0 out of range"),
    (dict(L=2049), "L=2049 out of range"),
    (dict(L=72, stride=71), "row stride 71 below L=72"),
    (dict(L=72, lp_stride=71), "log-probability row stride 71 below L=72"),
    (dict(V=0), "vocab_size 0 out of range"),
    (dict(V=4097), "vocab_size 4097 out of range"),
    (dict(po=4), "pitch_offset 4 below"),
    (dict(po=5, to=134), "129 pitch ids out of range"),
    (dict(to=133, V=132), "time_offset 133 beyond vocab_size 132"),
    (dict(steps=-1), "steps_per_row -1 out of range"),
    (dict(R=65535, steps=40000), "does not fit in int32"),
    (dict(R=65535, L=2048, stride=40000), "the id tensor does not fit in int32 elements"),
    (dict(R=65535, L=2048, lp_stride=40000), "the log-probability tensor does not fit in int32 elements"),
    (dict(ids=None), "null ids"),
    (dict(notes=None), "null ids"),
    (dict(counts=None), "null ids"),
    (dict(lp=None), "null logprobs"),
    (dict(note_lp=None), "null logprobs"),
])
def test_scored_detokenize_refuses_on_the_arguments_alone(kw, msg):
    st, err = _scored(**kw)
    assert st == -1 and err.startswith("m2m_score_detokenize_scored: ") and msg in err, err


def test_python_layer_refuses_before_the_library():
    ids = torch.zeros((2, 8), dtype=torch.long)
    lp = torch.zeros((2, 8))
    with pytest.raises(ValueError, match="CUDA float32"):
        scoring.detokenize_scored(TOK, ids, lp)
    with pytest.raises(ValueError, match="min_confidence"):
        scoring.detokenize_scored(TOK, ids, lp, min_confidence=1.5)
    with pytest.raises(ValueError, match="needs token_logprobs"):
        scoring.chroma_counts(TOK, ids, [np.zeros((0, 4))] * 2, min_confidence=0.5)
    with pytest.raises(ValueError, match="carry no log-probabilities"):
        scoring.DeviceNotes(None, None, "batched", 0.05, 80, 0).confidence_numpy()


# ------------------------------------------------------------------------------------------------ Music2MIDI without a device
class _Host:
    """``Music2MIDI``'s inference methods over a stand-in model that "decodes" fixed CPU rows, two segments per call."""
    for _name in ("generate", "generate_notes", "sample_scored_rows", "sample_token_rows", "sample_tokens", "score_recording", "score_batch",
                  "_segment_chunks", "_padded_segments", "_resolve_audio", "_segment_length", "_device_ingest", "_grammar_kwargs"):
        locals()[_name] = getattr(Music2MIDI, _name)
    device = torch.device("cpu")

    def __init__(self, ids, lp, **inference):
        cfg = copy.deepcopy(DEFAULT_CONFIG)
        cfg["inference"] = dict(batch_size=2, **inference)
        self.config = load_config(cfg)
        self.ids, self.lp, self.calls, self.next_row = torch.from_numpy(ids), torch.from_numpy(lp), [], 0
        self.model = SimpleNamespace(generate=self._decode, tokenizer=TOK, geometry=SimpleNamespace(pad_token_id=0))

    def _cond_rows(self, n_rows, cond_index):
        return torch.zeros((n_rows, 2), dtype=torch.long)

    def _decode(self, inputs, max_length, **kw):
        self.calls.append(kw)
        lo, hi = self.next_row, self.next_row + inputs.input_waveform.shape[0]
        self.next_row = hi % len(self.ids)
        ids = self.ids[lo:hi]
        width = max(2, int((ids != 0).any(0).nonzero().max()) + 1)   # the columns a decode returns: up to the longest row's end
        if not kw.get("return_dict_in_generate"):
            return ids[:, :width]
        return SimpleNamespace(sequences=ids[:, :width], logprobs=self.lp[lo:hi, 1:width])


def _host_case():
    _, ids, lp = cc.fuzz(3, 64, 0.10, 21)
    ids[2, 30:] = 0                                           # the second call returns fewer columns than the first
    ids[:, 0], lp[:, 0] = 0, 0.0                              # the start token: its log-probability is not the model's
    return ids, lp, np.zeros(int(2.5 * 3 * 16000), dtype=np.float32)   # 2.5 segments of audio: three rows


def test_generate_notes_on_cpu_ids_is_the_host_definition():
    ids, lp, audio = _host_case()
    m = _Host(ids, lp)
    plain = m.generate_notes(audio_y=audio)
    assert m.calls == [{}] * 2 and np.array_equal(plain, TOK.decode(ids, mode="sequential", duration_per_batch=3))
    m.calls.clear()
    notes, conf = m.generate_notes(audio_y=audio, return_confidence=True)
    assert m.calls == [dict(return_dict_in_generate=True, output_logprobs=True)] * 2
    want_notes, want_conf = confidence.decode_with_confidence(TOK, ids, lp, "sequential", 3)
    assert len(notes) > 4 and np.array_equal(notes, plain) and np.array_equal(notes, want_notes)
    assert np.array_equal(conf, want_conf, equal_nan=True)
    # a threshold alone returns the notes only; the config key is the default of the argument
    floor = float(np.sort(want_conf[~np.isnan(want_conf)])[len(want_conf) // 2])
    want_some, want_some_conf = confidence.decode_with_confidence(TOK, ids, lp, "sequential", 3, floor)
    assert 0 < len(want_some) < len(want_notes)
    some = m.generate_notes(audio_y=audio, min_confidence=floor)
    assert isinstance(some, np.ndarray) and np.array_equal(some, want_some)
    keyed = _Host(ids, lp, min_note_confidence=floor, midi_grammar=True)
    got, got_conf = keyed.generate_notes(audio_y=audio, return_confidence=True)
    assert np.array_equal(got, want_some) and np.array_equal(got_conf, want_some_conf, equal_nan=True)
    assert keyed.calls == [dict(return_dict_in_generate=True, output_logprobs=True, midi_grammar=True)] * 2
    assert np.array_equal(keyed.generate_notes(audio_y=audio, min_confidence=0.0), plain)     # the argument wins over the key
    with pytest.raises(ValueError, match="min_confidence"):
        m.generate_notes(audio_y=audio, min_confidence=1.5)
    # score_recording under a threshold: the host score of the filtered notes
    from music2midi_amd import evaluation
    from music2midi_amd.utils import numpy_to_midi
    label = want_notes[::2]
    assert m.score_recording(label, audio_y=audio, min_confidence=floor) == \
        evaluation.evaluate_batch([numpy_to_midi(label)], [numpy_to_midi(want_some)])
    assert m.score_recording(label, audio_y=audio) == evaluation.evaluate_batch([numpy_to_midi(label)], [numpy_to_midi(want_notes)])


def test_score_batch_honours_the_config_key_on_the_host():
    from music2midi_amd import evaluation
    from music2midi_amd.input import ModelInputs
    from music2midi_amd.utils import numpy_to_midi
    labels, ids, lp = cc.fuzz(2, 64, 0.10, 22)
    ids[:, 0], lp[:, 0] = 0, 0.0
    inputs = ModelInputs(input_waveform=torch.zeros(2, 8), notes_batch=tuple(labels), cond_index=None)
    floor = 0.5
    kept, _ = confidence.decode_with_confidence(TOK, ids, lp, min_confidence=floor)
    everything = TOK.decode(ids, mode="batched")
    assert 0 < sum(len(k) for k in kept) < sum(len(e) for e in everything)
    m = _Host(ids, lp, min_note_confidence=floor)
    want = evaluation.evaluate_batch([numpy_to_midi(n) for n in labels], [numpy_to_midi(n) for n in kept])
    assert m.score_batch(inputs) == want and m.calls == [dict(return_dict_in_generate=True, output_logprobs=True)]
    plain = _Host(ids, lp)
    assert plain.score_batch(inputs) == evaluation.evaluate_batch([numpy_to_midi(n) for n in labels], [numpy_to_midi(n) for n in everything])
    assert plain.calls == [{}] and want != plain.score_batch(inputs)


def test_confidence_is_refused_under_beam_search():
    ids, lp, audio = _host_case()
    m = _Host(ids, lp, num_beams=2)
    for call in (lambda: m.generate_notes(audio_y=audio, return_confidence=True), lambda: m.generate_notes(audio_y=audio, min_confidence=0.3),
                 lambda: m.generate(audio_y=audio, confidence_velocity=True),
                 lambda: m.score_recording(np.zeros((0, 4)), audio_y=audio, min_confidence=0.3)):
        with pytest.raises(ValueError, match="num_beams > 1"):
            call()
    assert m.calls == []


def test_confidence_velocity_bounds():
    v = confidence.confidence_velocities(np.array([0.0, 1e-9, 0.0039, 0.004, 0.5, 0.9999, 1.0, 1.5, np.inf, np.nan]))
    assert v.dtype == np.float64 and v.tolist() == [1, 1, 1, 1, 64, 127, 127, 127, 127, 1]
    assert all(x == max(1, min(127, int(round(127 * c)))) for x, c in zip(v.tolist(), [0.0, 1e-9, 0.0039, 0.004, 0.5, 0.9999, 1.0, 1.5]))
    ids, lp, audio = _host_case()
    m = _Host(ids, lp)
    midi = m.generate(audio_y=audio, confidence_velocity=True)
    notes, conf = m.generate_notes(audio_y=audio, return_confidence=True)
    got = sorted((n.start, n.end, n.pitch, n.velocity) for inst in midi.instruments for n in inst.notes)
    want = sorted((s, e, int(pch), int(vel)) for (s, e, pch, _), vel in zip(notes.tolist(), confidence.confidence_velocities(conf).tolist())
                  if e > s)
    assert got == want and len({x[3] for x in got}) > 3 and all(1 <= x[3] <= 127 for x in got)
    plain = m.generate(audio_y=audio)
    assert {n.velocity for inst in plain.instruments for n in inst.notes} == {TOK.config.default_velocity}
