"""GPU: per-note confidence on the device (scoring.detokenize_scored, csrc/score.hip) against its definition on the host
(music2midi_amd.confidence) - the same notes and the same float32 parts bit for bit, at the row capacity, through strided views,
through the counts kernel after the filter, and end to end through ``Music2MIDI`` on random-init weights."""
import copy

import numpy as np
import pytest
import torch

import confidence_cases as cc
from music2midi_amd import confidence, evaluation, scoring, synth
from music2midi_amd.config import DEFAULT_CONFIG, T5Geometry
from music2midi_amd.tokenizer import EOS, OFFSET, ONSET
from music2midi_amd.utils import numpy_to_midi

pytestmark = pytest.mark.gpu
TOK = cc.TOK
t, p = cc.t, cc.p


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _host(ids, lp, mode, floor):
    """(notes, confidence, parts) of the definition, each a list per row or concatenated as the mode says."""
    kw = dict(duration_per_batch=3) if mode == "sequential" else {}
    notes, conf = confidence.decode_with_confidence(TOK, ids, lp, mode=mode, min_confidence=floor, **kw)
    parts = []
    for r in range(len(ids)):
        _, pr = confidence.note_logprobs(TOK, ids[r], lp[r])
        parts.append(pr[confidence.keep_mask(pr, floor)])
    return notes, conf, parts if mode == "batched" else np.concatenate(parts)


def _check(ids, lp, mode, floor, ids_dev=None, lp_dev=None):
    """One scored call against the definition: notes equal, the two float32 parts bitwise equal, the confidences equal."""
    kw = dict(duration_per_batch=3) if mode == "sequential" else {}
    notes, conf, parts = _host(ids, lp, mode, floor)
    dn = scoring.detokenize_scored(TOK, torch.from_numpy(ids).cuda() if ids_dev is None else ids_dev,
                                   torch.from_numpy(lp).cuda() if lp_dev is None else lp_dev, mode=mode, min_confidence=floor, **kw)
    assert dn.note_lp.dtype == torch.float32 and tuple(dn.note_lp.shape) == (*ids.shape, 2)
    got, got_parts, got_conf = dn.to_numpy(), dn.note_lp_numpy(), dn.confidence_numpy()
    if mode == "sequential":
        notes, conf, parts, got, got_parts, got_conf = [notes], [conf], [parts], [got], [got_parts], [got_conf]
    assert len(got) == len(notes) == len(got_parts) == len(got_conf)
    for r, (g, w) in enumerate(zip(got, notes)):
        assert g.dtype == np.float64 and g.shape == w.shape and np.array_equal(g, w), (mode, floor, r)
        assert got_parts[r].dtype == np.float32 and np.array_equal(_bits(got_parts[r]), _bits(parts[r])), (mode, floor, r)
        assert got_conf[r].dtype == np.float64 and np.array_equal(got_conf[r], conf[r], equal_nan=True), (mode, floor, r)
    return notes, conf


def _own_threshold(ids, lp):
    """The confidence of one decoded note of the set, a median one: as a threshold it keeps that note (the boundary)."""
    _, conf = confidence.decode_with_confidence(TOK, ids, lp)
    flat = np.concatenate(conf)
    flat = np.sort(flat[np.isfinite(flat) & (flat > 0)])
    return float(flat[len(flat) // 2])


CASES = {"hand": cc.hand_batch, "nan and -inf": cc.special_batch}
CASES.update({f"fuzz {R}x{L} at {rate}": (lambda a=(R, L, rate, seed): cc.fuzz(*a)[1:]) for R, L, rate, seed in cc.FUZZ_SETS if R == 8})


@pytest.mark.parametrize("case", list(CASES))
def test_device_equals_definition_exactly(case):
    ids, lp = CASES[case]()
    own = _own_threshold(ids, lp)
    plain = TOK.decode(ids, mode="batched")
    for mode in ("batched", "sequential"):
        kept = {}
        for floor in (0.0, 0.5, own):
            notes, conf = _check(ids, lp, mode, floor)
            kept[floor] = sum(len(n) for n in notes)
            assert any((c == own).any() for c in conf) or floor == 0.5       # the note whose confidence is the threshold is kept
        assert kept[0.0] == sum(len(n) for n in plain) and kept[own] < kept[0.0]
    # with the threshold at 0 the notes are the plain detokenise's, and that export is what it was
    got = scoring.detokenize(TOK, torch.from_numpy(ids).cuda())
    assert got.note_lp is None and all(np.array_equal(g, w) for g, w in zip(got.to_numpy(), plain))
    if case.startswith("fuzz"):
        assert kept[0.5] < kept[0.0]
        parts = np.concatenate(_host(ids, lp, "batched", 0.0)[2])
        assert np.isnan(parts).any() and np.isneginf(parts).any()             # notes whose total is NaN, notes whose total is -inf


def test_capacity_at_the_longest_row():
    """L = 2048, one row per call: a row of open notes only, a row that closes 1916 notes with one run of 128 OFFSET events, and
    a row whose single note is closed by the last of a chain of 2041 OFFSET events of its pitch."""
    rng = np.random.default_rng(5)
    open_only = [t(0), ONSET] + [p(i % 128) for i in range(2045)] + [EOS]
    n_open = 2048 - 4 - 128
    closed = [t(0), ONSET] + [p(i % 128) for i in range(n_open)] + [t(1), OFFSET] + [p(i) for i in range(128)]
    chain = [t(199), ONSET, p(60), t(5), OFFSET] + [p(60)] * 2040 + [t(250), OFFSET, p(60)]
    for row, n_notes in ((open_only, 0), (closed, n_open), (chain, 1)):
        assert len(row) == 2048
        ids = np.asarray([row], dtype=np.int64)
        lp = (-rng.exponential(0.12, ids.shape)).astype(np.float32)
        assert len(TOK.decode(ids)[0]) == n_notes
        for mode in ("batched", "sequential"):
            notes, _ = _check(ids, lp, mode, 0.0)
            assert len(notes[0]) == n_notes
        own = _own_threshold(ids, lp) if n_notes else 0.5
        notes, _ = _check(ids, lp, "batched", own)
        assert len(notes[0]) == (0 if n_notes == 0 else 1 if n_notes == 1 else n_open - n_open // 2)
    idx, cols = confidence.note_columns(TOK, chain)
    assert idx.tolist() == [[199, 250, 60]] and cols.tolist() == [[0, 1, 2, 2045, 2046, 2047]]


def test_strided_views_and_an_id_outside_the_vocabulary():
    _, ids, lp = cc.fuzz(8, 64, 0.10, 11)
    wide_ids = torch.full((8, 100), 7, dtype=torch.long)
    wide_lp = torch.full((8, 120), -9.0)
    wide_ids[:, 10:74] = torch.from_numpy(ids)
    wide_lp[:, 33:97] = torch.from_numpy(lp)
    ids_view, lp_view = wide_ids.cuda()[:, 10:74], wide_lp.cuda()[:, 33:97]
    assert ids_view.stride() == (100, 1) and lp_view.stride() == (120, 1)
    for mode in ("batched", "sequential"):
        _check(ids, lp, mode, 0.5, ids_view, lp_view)
    spread = torch.zeros((8, 128))
    spread[:, ::2] = torch.from_numpy(lp)
    with pytest.raises(ValueError, match="unit inner stride"):
        scoring.detokenize_scored(TOK, ids_view, spread.cuda()[:, ::2])
    with pytest.raises(ValueError, match="token_logprobs"):
        scoring.detokenize_scored(TOK, ids_view, lp_view[:, :-1])
    with pytest.raises(ValueError, match="CUDA float32"):
        scoring.detokenize_scored(TOK, ids_view, lp_view.double())
    # an id outside the vocabulary: the row is refused, the others are unharmed
    bad = ids.copy()
    bad[2, 30] = 400
    dn = scoring.detokenize_scored(TOK, torch.from_numpy(bad).cuda(), torch.from_numpy(lp).cuda(), min_confidence=0.5)
    for call in (dn.to_numpy, dn.confidence_numpy, dn.note_lp_numpy,
                 lambda: scoring.chroma_counts(TOK, torch.from_numpy(bad).cuda(), [np.zeros((0, 4))] * 8, token_logprobs=torch.from_numpy(lp).cuda(),
                                               min_confidence=0.5)):
        with pytest.raises(ValueError, match="token row 2 holds an id outside"):
            call()
    counts, notes, parts = dn.counts.cpu().numpy(), dn.notes.cpu().numpy(), dn.note_lp.cpu().numpy()
    assert counts[2] == -1
    for r in (0, 1, 3, 4, 5, 6, 7):
        idx, pr = confidence.note_logprobs(TOK, ids[r], lp[r])
        keep = confidence.keep_mask(pr, 0.5)
        assert counts[r] == keep.sum() and np.array_equal(notes[r, :counts[r]], idx[keep].astype(np.int32))
        assert np.array_equal(_bits(parts[r, :counts[r]]), _bits(pr[keep]))
    # rows and columns of size zero
    empty = scoring.detokenize_scored(TOK, torch.zeros((3, 0), dtype=torch.long).cuda(), torch.zeros((3, 0)).cuda())
    assert empty.to_numpy()[2].shape == (0, 4) and empty.confidence_numpy()[2].shape == (0,)
    none = scoring.detokenize_scored(TOK, torch.zeros((0, 5), dtype=torch.long).cuda(), torch.zeros((0, 5)).cuda())
    assert none.to_numpy() == [] and none.confidence_numpy() == []


def _host_counts(label, decoded):
    tm, om = evaluation.extract_midi_melody(numpy_to_midi(label), numpy_to_midi(decoded))
    both = (tm >= 0) & (om >= 0)
    return int((both & ((tm - om) % 12 == 0)).sum()), int((tm >= 0).sum()), len(tm)


def test_counts_after_filtering():
    labels, ids, lp = cc.fuzz(8, 64, 0.10, 11)
    ids_dev, lp_dev = torch.from_numpy(ids).cuda(), torch.from_numpy(lp).cuda()
    plain = TOK.decode(ids, mode="batched")
    scores = {}
    for floor in (0.0, 0.5, _own_threshold(ids, lp)):
        kept, _ = confidence.decode_with_confidence(TOK, ids, lp, min_confidence=floor)
        want = np.array([_host_counts(l, d) for l, d in zip(labels, kept)], dtype=np.int64)
        got = scoring.chroma_counts(TOK, ids_dev, labels, token_logprobs=lp_dev, min_confidence=floor)
        for name, col in (("correct", 0), ("voiced", 1), ("frames", 2)):
            assert np.array_equal(getattr(got, name), want[:, col]), (floor, name)
        host = evaluation.evaluate_batch([numpy_to_midi(n) for n in labels], [numpy_to_midi(n) for n in kept])
        assert got.score == host
        assert evaluation.evaluate_tokens(TOK, ids_dev, labels, token_logprobs=lp_dev, min_confidence=floor) == host
        scores[floor] = host
    assert len(set(scores.values())) > 1                       # the filter moves the score
    unfiltered = scoring.chroma_counts(TOK, ids_dev, labels)
    want = np.array([_host_counts(l, d) for l, d in zip(labels, plain)], dtype=np.int64)
    assert np.array_equal(unfiltered.correct, want[:, 0]) and np.array_equal(unfiltered.voiced, want[:, 1])
    assert np.array_equal(unfiltered.frames, want[:, 2]) and unfiltered.score == scores[0.0]
    # one recording: the rows are its segments, one label array
    label = np.concatenate([n + [3.0 * i, 3.0 * i, 0, 0] for i, n in enumerate(labels)])
    kept, _ = confidence.decode_with_confidence(TOK, ids, lp, mode="sequential", duration_per_batch=3, min_confidence=0.5)
    got = scoring.chroma_counts(TOK, ids_dev, label, mode="sequential", duration_per_batch=3, token_logprobs=lp_dev, min_confidence=0.5)
    assert (int(got.correct[0]), int(got.voiced[0]), int(got.frames[0])) == _host_counts(label, kept)
    assert got.score == evaluation.evaluate_batch([numpy_to_midi(label)], [numpy_to_midi(kept)]) and 0.0 < got.score < 1.0


@pytest.fixture(scope="module")
def random_init_model():
    from music2midi_amd.checkpoint import load_t5_state
    from music2midi_amd.model import Music2MIDI
    geom = T5Geometry(DEFAULT_CONFIG["model"]["t5"])
    sd = synth.t5_state_dict(geom, seed=0)
    synth.perturb_layer_norms(sd, 0)
    synth.force_eos_head(sd, geom, active=340, eos_scale=1.6)
    m = Music2MIDI(copy.deepcopy(DEFAULT_CONFIG))
    load_t5_state(m.model, sd, strict=False)
    return m.cuda().eval()


@pytest.mark.parametrize("grammar", [False, True])
def test_end_to_end_on_the_random_init_model(random_init_model, grammar):
    """``generate_notes(return_confidence=True)`` against the definition applied to that call's own sequences and log-probabilities,
    against plain ``generate_notes``, and ``score_recording`` / ``score_batch`` under a threshold against the host score of the
    filtered notes.  Random weights close few notes on their own; under the token grammar the rows are well-formed groups."""
    from music2midi_amd.input import ModelInputs
    m = random_init_model
    m.config.inference.pop("min_note_confidence", None)
    m.config.inference["midi_grammar"] = grammar
    audio = synth.waveform(33, 7 * 16000)                      # 7 s: three segments
    plain = m.generate_notes(audio_y=audio, cond_index=[4, 2])

    seen = []
    real = m.model.generate

    def recording(*a, **kw):
        out = real(*a, **kw)
        seen.append((kw, out))
        return out
    m.model.generate = recording
    try:
        notes, conf = m.generate_notes(audio_y=audio, cond_index=[4, 2], return_confidence=True)
    finally:
        m.model.generate = real
    assert len(seen) == 1 and seen[0][0]["return_dict_in_generate"] is True and seen[0][0]["output_logprobs"] is True
    assert seen[0][0].get("midi_grammar", False) is grammar
    sequences, logprobs = seen[0][1].sequences.cpu().numpy(), seen[0][1].logprobs.cpu().numpy()
    assert sequences.shape[0] == 3 and logprobs.shape == (3, sequences.shape[1] - 1)
    lp = np.concatenate([np.zeros((3, 1), dtype=np.float32), logprobs], axis=1)
    want_notes, want_conf = confidence.decode_with_confidence(TOK, sequences, lp, "sequential", 3)
    print(f"end to end, grammar {grammar}: {sequences.shape[1]} columns, {len(notes)} notes, confidences {np.sort(conf)[[0, -1]] if len(conf) else '-'}")
    assert np.array_equal(notes, want_notes) and np.array_equal(conf, want_conf)
    assert ((conf >= 0) & (conf <= 1)).all() and (not grammar or len(notes) >= 2)
    # the scored head selects what the plain head selects: the same notes
    assert np.array_equal(notes, plain)
    # a threshold: the median confidence drops the notes below it, on the device as in the definition
    floor = float(np.sort(conf)[len(conf) // 2]) if len(conf) else 0.5
    kept, kept_conf = confidence.decode_with_confidence(TOK, sequences, lp, "sequential", 3, floor)
    assert len(kept) <= len(notes) and (len(np.unique(conf)) < 2 or 0 < len(kept) < len(notes))
    got, got_conf = m.generate_notes(audio_y=audio, cond_index=[4, 2], return_confidence=True, min_confidence=floor)
    assert np.array_equal(got, kept) and np.array_equal(got_conf, kept_conf)
    assert np.array_equal(m.generate_notes(audio_y=audio, cond_index=[4, 2], min_confidence=floor), kept)
    label = np.concatenate([plain[::2] + [0.0, 0.05, 0, 0], [[0.5, 2.5, 60, 80]]])
    host = evaluation.evaluate_batch([numpy_to_midi(label)], [numpy_to_midi(kept)])
    assert m.score_recording(label, audio_y=audio, cond_index=[4, 2], min_confidence=floor) == host
    assert m.score_recording(label, audio_y=audio, cond_index=[4, 2]) == evaluation.evaluate_batch([numpy_to_midi(label)], [numpy_to_midi(plain)])
    # velocities from confidences
    midi = m.generate(audio_y=audio, cond_index=[4, 2], confidence_velocity=True)
    assert sorted(n.velocity for inst in midi.instruments for n in inst.notes) == \
        sorted(int(v) for v, (s, e, _, _) in zip(confidence.confidence_velocities(conf), notes) if e > s)
    # score_batch reads the config key
    labels = (np.array([[0.10, 0.40, 60, 80], [0.50, 1.00, 64, 80], [1.20, 1.90, 67, 80], [2.00, 2.60, 72, 80]]),
              np.array([[0.05, 0.30, 50, 80], [0.70, 1.10, 55, 80]]))
    wav = torch.from_numpy(synth.waveform_batch(40, 2, 48000))
    idx = torch.from_numpy(synth.cond_index_batch(40, 2))
    inputs = ModelInputs(input_waveform=wav.cuda(), notes_batch=labels, cond_index=idx.cuda())
    out = m.model.generate(inputs, max_length=16, return_dict_in_generate=True, output_logprobs=True, **m._grammar_kwargs())
    b_ids = out.sequences.cpu().numpy()
    b_lp = np.concatenate([np.zeros((2, 1), dtype=np.float32), out.logprobs.cpu().numpy()], axis=1)
    _, b_conf = confidence.decode_with_confidence(TOK, b_ids, b_lp)
    flat = np.sort(np.concatenate(b_conf))
    print(f"labelled batch, grammar {grammar}: {len(flat)} notes")
    m.config.inference["min_note_confidence"] = float(flat[len(flat) // 2]) if len(flat) else 0.5
    try:
        b_kept, _ = confidence.decode_with_confidence(TOK, b_ids, b_lp, min_confidence=m.config.inference["min_note_confidence"])
        assert m.score_batch(inputs) == evaluation.evaluate_batch([numpy_to_midi(n) for n in labels], [numpy_to_midi(n) for n in b_kept])
    finally:
        del m.config.inference["min_note_confidence"]
