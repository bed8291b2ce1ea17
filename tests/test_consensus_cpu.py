"""CPU: the definition of the consensus selection (music2midi_amd.consensus) on hand-made inputs with the result worked out here;
what the device form (scoring.pairwise_note_counts / consensus_choice, csrc/consensus.hip) decides without a device - the header
against the binding, the refusals of its entry points, the ``ValueError``s of the Python layers, the config keys and the routing of
``Music2MIDI`` - and a seeded sanity check of the selection rule on synthetic candidates."""
import copy
import ctypes as C
import inspect
from pathlib import Path

import numpy as np
import pytest
import torch

import consensus_cases as cs
import note_metrics_cases as nc
from music2midi_amd import consensus, native, note_metrics, scoring
from music2midi_amd.config import DEFAULT_CONFIG, inference_consensus, load_config
from music2midi_amd.model import Music2MIDI, _decode_entry, _rows_per_clip
from music2midi_amd.transformer import T5Transformer

ROOT = Path(__file__).resolve().parents[1]
FAKE = 0x100000                          # a device address that is never dereferenced: every refusal comes first
TOK = nc.TOK


# ------------------------------------------------------------------------------------------------ the definition
def test_the_asymmetric_pair_in_both_orientations():
    # reference (0, 40, 60): 2 s long, tolerance max(0.2 * 2.0, 0.05) = 0.4 s, and the offsets are 8 steps = 0.4 s apart: a hit;
    # reference (0, 32, 60): 1.6 s long, tolerance 0.32 s < 0.4 s: a miss
    long_, short = nc.est_seconds([(0, 40, 60)]), nc.est_seconds([(0, 32, 60)])
    assert note_metrics.match_counts(long_, short)[0] == 1 and note_metrics.match_counts(short, long_)[0] == 0
    tp, n = consensus.pairwise_counts([long_, short])
    assert tp.dtype == np.int64 and n.dtype == np.int64
    assert tp.tolist() == [[1, 0], [1, 1]] and n.tolist() == [1, 1]          # tp[1, 0]: ref = candidate 0 (long), est = candidate 1
    tp, n = consensus.pairwise_counts([short, long_])
    assert tp.tolist() == [[1, 1], [0, 1]]
    tp, _ = consensus.pairwise_counts([long_, short], offset_ratio=None)
    assert tp.tolist() == [[1, 1], [1, 1]]


def test_the_augmenting_path_pair_in_both_orientations():
    labels, decoded, with_offsets, _ = nc.CRAFTED["augmenting path"]
    assert with_offsets == (2, 2, 2)
    est = nc.est_seconds(decoded)
    tp, n = consensus.pairwise_counts([est, labels])                         # tp[0, 1]: ref = the labels, est = the decoded notes
    assert tp[0, 1] == 2 and n.tolist() == [2, 2]
    # the other way round the decoded notes are the references: X = (1.00, 1.85), Y = (1.05, 2.10); A = (1.00, 2.00), B = (1.04, 1.80).
    # X: tolerance 0.17 - A is 0.15 off (hit), B 0.05 (hit); Y: tolerance 0.21 - A is 0.10 off (hit), B 0.30 (miss): X <- B, Y <- A
    assert tp[1, 0] == 2
    assert tp.tolist() == [[2, 2], [2, 2]]


def test_identical_candidates_agree_completely():
    est = nc.est_seconds([(0, 10, 60), (5, 9, 64), (20, 30, 60)])
    for K in (2, 3, 16):
        tp, n = consensus.pairwise_counts([est] * K)
        assert (tp == 3).all() and (n == 3).all()
        index, u = consensus.select(tp, n)
        assert index == 0 and u.tolist() == [1.0] * K and u.dtype == np.float64


def test_empty_candidates():
    empty = np.zeros((0, 4))
    tp, n = consensus.pairwise_counts([empty] * 4)
    assert not tp.any() and not n.any()
    index, u = consensus.select(tp, n)
    assert index == 0 and u.tolist() == [1.0] * 4                            # two silent candidates agree
    # one spurious candidate at index 0 among empty ones: it agrees with nobody, every empty one with the two other empty ones
    spurious = nc.est_seconds([(3, 9, 60), (4, 8, 62)])
    tp, n = consensus.pairwise_counts([spurious, empty, empty, empty])
    assert n.tolist() == [2, 0, 0, 0] and tp.tolist() == [[2, 0, 0, 0], [0] * 4, [0] * 4, [0] * 4]
    index, u = consensus.select(tp, n)
    assert u.tolist() == [0.0, (0.0 + 1.0 + 1.0) / 3, (0.0 + 1.0 + 1.0) / 3, (0.0 + 1.0 + 1.0) / 3] and index == 1
    # a note with end <= start does not exist
    tp, n = consensus.pairwise_counts([np.array([[1.0, 1.0, 60, 77.0]]), empty])
    assert n.tolist() == [0, 0] and consensus.select(tp, n)[0] == 0


def test_agreement_and_the_order_of_the_sum():
    assert consensus.agreement(0, 0, 0) == 1.0 and consensus.agreement(0, 3, 0) == 0.0 and consensus.agreement(2, 2, 2) == 1.0
    assert consensus.agreement(np.int64(1), np.int64(2), np.int64(1)) == 2 / 3 and type(consensus.agreement(1, 2, 1)) is float
    tp = np.array([[3, 1, 2, 1], [1, 7, 1, 3], [2, 1, 4, 0], [1, 3, 0, 6]])
    n = np.array([3, 7, 4, 6])
    u = consensus.expected_agreement(tp, n)
    assert u[0] == ((0.0 + 2 / 10) + 4 / 7 + 2 / 9) / 3 and u[3] == ((0.0 + 2 / 9) + 6 / 13 + 0 / 10) / 3
    assert consensus.select(tp, n)[0] == int(np.argmax(u))
    # K = 2: the two utilities are each other's only term; with offsets they may differ, a tie goes to candidate 0
    tp, n = np.array([[1, 1], [1, 1]]), np.array([1, 1])
    assert consensus.select(tp, n)[0] == 0 and consensus.expected_agreement(tp, n).tolist() == [1.0, 1.0]
    tp = np.array([[1, 0], [1, 1]])
    index, u = consensus.select(tp, n)
    assert u.tolist() == [0.0, 1.0] and index == 1
    for bad in (1, 17):
        with pytest.raises(ValueError, match="candidates out of range"):
            consensus.pairwise_counts([np.zeros((0, 4))] * bad)
    for bad in (None, "4", 4.0, True, 1, 17):
        with pytest.raises(ValueError, match="candidates out of range"):
            consensus.check_candidates(bad)
    assert consensus.check_candidates(np.int64(4)) == 4 and type(consensus.check_candidates(np.int64(4))) is int
    with pytest.raises(ValueError, match="tp of shape"):
        consensus.expected_agreement(np.zeros((3, 2)), np.zeros(3))


def test_onsets_only_is_symmetric():
    _, cands = cs.clips(5, 6, 7)
    some = 0
    for clip in cands:
        notes = [nc.est_seconds(c) for c in clip]
        tp, _ = consensus.pairwise_counts(notes, offset_ratio=None)
        assert np.array_equal(tp, tp.T)
        with_offsets, _ = consensus.pairwise_counts(notes)
        some += int(not np.array_equal(with_offsets, with_offsets.T))
        assert (with_offsets <= tp).all()
    assert some >= 1                                                         # with offsets the generator's clips are not all symmetric


# ------------------------------------------------------------------------------------------------ selection sanity
def _label_f1(label, candidate, ratio):
    tp, n_ref, n_est = note_metrics.match_counts(label, candidate, offset_ratio=ratio)
    return consensus.agreement(tp, n_est, n_ref)


@pytest.mark.parametrize("K,ratio", [(4, 0.2), (8, 0.2), (16, 0.2), (4, None), (8, None), (16, None)])
def test_the_selected_candidate_is_closer_to_the_hidden_label_than_the_average_one(K, ratio):
    """200 seeded clips (consensus_cases, seed 2024 + K): the mean label-F1 of the selected candidate against the mean label-F1 of all
    candidates, a condition with no margin.  This generator gives selected / mean
        with offsets   K = 4: 0.277 / 0.244    K = 8: 0.304 / 0.240    K = 16: 0.357 / 0.227
        onsets only    K = 4: 0.384 / 0.350    K = 8: 0.416 / 0.339    K = 16: 0.499 / 0.325."""
    labels, cands = cs.clips(2024 + K, 200, K)
    selected, everyone = [], []
    for label, clip in zip(labels, cands):
        notes = [nc.est_seconds(c) for c in clip]
        index, _ = consensus.select(*consensus.pairwise_counts(notes, offset_ratio=ratio))
        f1 = [_label_f1(label, c, ratio) for c in notes]
        selected.append(f1[index])
        everyone.append(float(np.mean(f1)))
    print(f"K={K} offset_ratio={ratio}: selected {np.mean(selected):.3f} / mean {np.mean(everyone):.3f}")
    assert np.mean(selected) > np.mean(everyone)


# ------------------------------------------------------------------------------------------------ header, binding, refusals
def test_header_declares_what_the_binding_binds():
    header = (ROOT / "include" / "music2midi_amd.h").read_text()
    for name, proto in [
            ("m2m_consensus_workspace_bytes", "int64_t m2m_consensus_workspace_bytes(int R, int L, int K);"),
            ("m2m_consensus_pairwise_counts", "int m2m_consensus_pairwise_counts(const int32_t* notes_dev, const int32_t* counts_dev, int R, int L, "
                                              "int K, double time_step,"),
            ("m2m_consensus_select", "int m2m_consensus_select(const int32_t* tp_dev, const int32_t* n_dev, int B, int K, int32_t* chosen_out_dev, "
                                     "double* utility_out_dev,")]:
        assert proto in header, name
        assert name in native.EXPORTED_SYMBOLS and hasattr(native.load(), name)
    assert header.index("int m2m_score_error_notes(") < header.index("int m2m_consensus_pairwise_counts(") < header.index("Audio ingest")
    assert "#define M2M_CONSENSUS_MAX_CANDIDATES 16" in header and scoring.MAX_CANDIDATES == 16 == consensus.MAX_CANDIDATES
    args = native._SIGNATURES["m2m_consensus_pairwise_counts"][1]
    assert len(args) == 14 and [i for i, a in enumerate(args) if a is C.c_double] == [5, 6, 7, 8] and args[10] is C.c_int64
    assert native._SIGNATURES["m2m_consensus_workspace_bytes"] == (C.c_int64, [C.c_int] * 3)
    assert native._SIGNATURES["m2m_consensus_select"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 3)
    lib = native.load()
    for R, L, K in ((2, 1, 2), (15, 7, 5), (128, 1024, 16), (48, 1023, 16), (6, 2048, 3)):
        NE, NP, arrays = R * L, R * (K - 1) * L, lambda per, count: (per * count + 7) // 8 * 8
        assert lib.m2m_consensus_workspace_bytes(R, L, K) == 3 * arrays(8, NE) + arrays(4, NE) + 4 * arrays(4, NP)
    assert lib.m2m_consensus_workspace_bytes(128, 1024, 16) == 28 * 128 * 1024 + 16 * 128 * 15 * 1024
    for bad in ((0, 1, 2), (65536, 1, 2), (2, 0, 2), (2, 2049, 2), (2, 8, 1), (17, 8, 17), (34, 8, 17), (5, 8, 2), (16, 8, 5)):
        assert lib.m2m_consensus_workspace_bytes(*bad) == -1


def _pairwise(R=6, L=40, K=3, ts=0.05, onset=0.05, ratio=0.2, floor=0.05, ws=FAKE, ws_bytes=None, notes=FAKE, counts=FAKE, tp=FAKE, n=FAKE):
    lib = native.load()
    if ws_bytes is None:
        ws_bytes = max(8, lib.m2m_consensus_workspace_bytes(R, L, K))
    st = lib.m2m_consensus_pairwise_counts(notes, counts, R, L, K, ts, onset, ratio, floor, ws, ws_bytes, tp, n, None)
    return st, lib.m2m_last_error().decode()


@pytest.mark.parametrize("kw,msg", [
    (dict(R=0), "0 rows out of range"),
    (dict(R=65536, K=2), "65536 rows out of range"),
    (dict(L=0), "L=0 out of range"),
    (dict(L=2049), "L=2049 out of range"),
    (dict(K=1), "1 candidates out of range"),
    (dict(R=17, K=17), "17 candidates out of range"),
    (dict(K=0), "0 candidates out of range"),
    (dict(R=7, K=3), "7 rows are not whole clips of 3 candidates"),
    (dict(R=16, K=5), "16 rows are not whole clips of 5 candidates"),
    (dict(ts=0.0), "time_step 0 out of range"),
    (dict(ts=float("nan")), "time_step nan out of range"),
    (dict(onset=-0.01), "onset_tolerance -0.01 out of range"),
    (dict(onset=float("nan")), "onset_tolerance nan out of range"),
    (dict(ratio=float("nan")), "offset_ratio nan out of range"),
    (dict(ratio=float("inf")), "offset_ratio inf out of range"),
    (dict(floor=-1.0), "offset_min_tolerance -1 out of range"),
    (dict(notes=None), "null notes"),
    (dict(counts=None), "null notes"),
    (dict(tp=None), "null notes"),
    (dict(n=None), "null notes"),
    (dict(ws=None), "null or misaligned workspace"),
    (dict(ws=FAKE + 4), "null or misaligned workspace"),
    (dict(ws_bytes=64), "workspace of 64 bytes"),
])
def test_pairwise_counts_refuses_on_the_arguments_alone(kw, msg):
    st, err = _pairwise(**kw)
    assert st == -1 and msg in err and "m2m_consensus_pairwise_counts" in err, err


@pytest.mark.parametrize("kw,msg", [
    (dict(B=0), "0 clips out of range"), (dict(B=65536), "65536 clips out of range"), (dict(K=1), "1 candidates out of range"),
    (dict(K=17), "17 candidates out of range"), (dict(tp=None), "null counts"), (dict(n=None), "null counts"),
    (dict(chosen=None), "null counts"), (dict(utility=None), "null counts"), (dict(utility=FAKE + 4), "misaligned utility"),
])
def test_select_refuses_on_the_arguments_alone(kw, msg):
    a = dict(tp=FAKE, n=FAKE, B=3, K=4, chosen=FAKE, utility=FAKE)
    a.update(kw)
    lib = native.load()
    st = lib.m2m_consensus_select(a["tp"], a["n"], a["B"], a["K"], a["chosen"], a["utility"], None)
    err = lib.m2m_last_error().decode()
    assert st == -1 and msg in err and "m2m_consensus_select" in err, err


def test_python_layer_refuses_before_the_library():
    ids = torch.zeros((6, 8), dtype=torch.long)
    for fn in (scoring.pairwise_note_counts, scoring.consensus_choice):
        for K in (1, 17, 0, 2.5, True, None, "3"):
            with pytest.raises(ValueError, match="candidates out of range"):
                fn(TOK, ids, K)
        with pytest.raises(ValueError, match="6 rows are not whole clips of 4 candidates"):
            fn(TOK, ids, 4)
        with pytest.raises(ValueError, match="int64 tensor"):
            fn(TOK, ids.int(), 3)
        with pytest.raises(ValueError, match="int64 tensor"):
            fn(TOK, ids[0], 3)
        for kw, what in ((dict(onset_tolerance=-0.1), "onset_tolerance"), (dict(offset_min_tolerance=float("nan")), "offset_min_tolerance"),
                         (dict(offset_ratio=-0.5), "offset_ratio"), (dict(offset_ratio=float("nan")), "offset_ratio")):
            with pytest.raises(ValueError, match=what):
                fn(TOK, ids, 3, **kw)


def test_ids_on_the_host_take_the_definition():
    _, cands = cs.clips(9, 3, 4)
    ids = torch.from_numpy(nc.id_rows([c for clip in cands for c in clip], 6 * 18 + 1))
    decoded = TOK.decode(ids)
    for ratio in (0.2, None):
        got = scoring.pairwise_note_counts(TOK, ids, 4, offset_ratio=ratio)
        chosen, utility = scoring.consensus_choice(TOK, ids, 4, offset_ratio=ratio)
        assert got.tp.shape == (3, 4, 4) and got.n.shape == (3, 4) and got.tp.dtype == np.int64
        assert chosen.dtype == torch.int32 and utility.dtype == torch.float64 and tuple(utility.shape) == (3, 4)
        for b in range(3):
            tp, n = consensus.pairwise_counts(decoded[4 * b:4 * b + 4], offset_ratio=ratio)
            assert np.array_equal(got.tp[b], tp) and np.array_equal(got.n[b], n)
            index, u = consensus.select(tp, n)
            assert int(chosen[b]) == index and np.array_equal(utility[b].numpy(), u)


# ------------------------------------------------------------------------------------------------ config, routing, refusals
def _config(**inference):
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["inference"].update(inference)
    return cfg


def test_config_keys():
    assert inference_consensus(load_config(DEFAULT_CONFIG)) == {}
    for off in (0, 1, None):
        assert inference_consensus(load_config(_config(consensus_samples=off))) == {}
    assert inference_consensus(load_config(_config(consensus_samples=4))) == {"num_samples": 4}
    full = load_config(_config(consensus_samples=16, consensus_temperature=2, consensus_top_k=0, consensus_top_p=0.9))
    assert inference_consensus(full) == {"num_samples": 16, "temperature": 2.0, "top_k": 0, "top_p": 0.9}
    assert inference_consensus(full, 3)["num_samples"] == 3 and inference_consensus(full, 1) == {} and inference_consensus(full, 0) == {}
    assert inference_consensus(load_config(DEFAULT_CONFIG), 5) == {"num_samples": 5}
    for bad in (-1, 17, 2.5, True, "4"):
        with pytest.raises(ValueError, match="consensus_samples"):
            inference_consensus(load_config(_config(consensus_samples=bad)))
    with pytest.raises(ValueError, match="num_beams"):
        inference_consensus(load_config(_config(consensus_samples=4, num_beams=2)))
    with pytest.raises(ValueError, match="num_beams"):
        inference_consensus(load_config(_config(num_beams=2)), 4)
    assert inference_consensus(load_config(_config(num_beams=2, consensus_samples=1))) == {}


def test_music2midi_routes_consensus_through_generate_consensus():
    m = Music2MIDI(_config())
    fn, kw = _decode_entry(m.model, m.config, m._grammar_kwargs())
    assert fn == m.model.generate and kw == {} and _rows_per_clip(kw) == 1
    fn, kw = _decode_entry(m.model, m.config, m._grammar_kwargs(), 3)
    assert fn == m.model.generate_consensus and kw == {"num_samples": 3} and _rows_per_clip(kw) == 3
    m = Music2MIDI(_config(consensus_samples=8, consensus_temperature=0.7, midi_grammar=True, batch_size=20))
    fn, kw = _decode_entry(m.model, m.config, m._grammar_kwargs())
    assert fn == m.model.generate_consensus and kw == {"num_samples": 8, "temperature": 0.7, "midi_grammar": True}
    assert _rows_per_clip(kw) == 8
    assert _decode_entry(m.model, m.config, m._grammar_kwargs(), 1)[0] == m.model.generate          # the keyword overrides the config
    for name in ("generate", "generate_notes", "sample_tokens", "sample_token_rows"):
        assert inspect.signature(getattr(Music2MIDI, name)).parameters["consensus"].default is None


def test_music2midi_chunks_by_batch_size_over_k():
    """Five segments, batch_size 7, K = 3: chunks of two segments; the stand-in returns one row per segment."""
    m = Music2MIDI(_config(batch_size=7))
    calls = []

    def fake(inputs, max_length, **kw):
        calls.append((int(inputs.input_waveform.shape[0]), max_length, kw))
        return torch.zeros((inputs.input_waveform.shape[0], 2), dtype=torch.long)
    m.model.generate_consensus = fake
    seg = m._segment_length()
    rows = m.sample_token_rows(torch.zeros(5 * seg), seg, consensus=3)
    assert len(rows) == 5 and calls == [(2, 1024, {"num_samples": 3}), (2, 1024, {"num_samples": 3}), (1, 1024, {"num_samples": 3})]
    notes = m.generate_notes(audio_y=np.zeros(2 * seg, dtype=np.float32), consensus=3)
    assert notes.shape == (0, 4) and calls[-1] == (2, 1024, {"num_samples": 3})


def test_music2midi_refusals():
    audio = np.zeros(16, dtype=np.float32)
    m = Music2MIDI(_config())
    for bad in (17, -1, 2.5):
        with pytest.raises(ValueError, match="consensus_samples"):
            m.generate_notes(audio_y=audio, consensus=bad)
    with pytest.raises(ValueError, match="consensus decoding does not combine with return_confidence"):
        m.generate_notes(audio_y=audio, consensus=3, return_confidence=True)
    with pytest.raises(ValueError, match="consensus decoding does not combine with"):
        m.generate_notes(audio_y=audio, consensus=3, min_confidence=0.5)
    with pytest.raises(ValueError, match="consensus decoding does not combine with confidence_velocity"):
        m.generate(audio_y=audio, consensus=3, confidence_velocity=True)
    with pytest.raises(ValueError, match="num_beams"):
        Music2MIDI(_config(num_beams=2)).generate_notes(audio_y=audio, consensus=3)
    configured = Music2MIDI(_config(consensus_samples=4))
    with pytest.raises(ValueError, match="consensus decoding does not combine with"):
        configured.generate_notes(audio_y=audio, return_confidence=True)
    with pytest.raises(ValueError, match="consensus decoding does not combine with"):
        configured.generate_notes(audio_y=audio, min_confidence=0.3)
    with pytest.raises(ValueError, match="consensus decoding does not combine with"):
        configured.sample_scored_rows(torch.zeros(16), 16)
    with pytest.raises(ValueError, match="consensus decoding does not combine with"):
        Music2MIDI(_config(consensus_samples=4, min_note_confidence=0.5)).generate_notes(audio_y=audio)


def test_generate_consensus_refusals():
    t = Music2MIDI(_config()).model
    for entry, first in ((t.generate_consensus, None), (t.generate_consensus_from_embeds, torch.zeros((1, 4, 8)))):
        for bad in (1, 17, 0, 2.5, True):
            with pytest.raises(ValueError, match="candidates out of range"):
                entry(first, bad)
        with pytest.raises(ValueError, match="num_beams"):
            entry(first, 4, num_beams=2)
        for name in ("do_sample", "num_return_sequences", "return_dict_in_generate", "output_logprobs"):
            with pytest.raises(ValueError, match=name):
                entry(first, 4, **{name: True})
    p = inspect.signature(T5Transformer.generate_consensus).parameters
    assert list(p)[:10] == ["self", "inputs", "num_samples", "max_length", "temperature", "top_k", "top_p", "midi_grammar",
                            "return_candidates", "processor_keywords"]
    assert (p["max_length"].default, p["temperature"].default, p["top_k"].default, p["top_p"].default) == (20, 1.0, 50, 1.0)
    assert p["midi_grammar"].default is False and p["return_candidates"].default is False


def test_generate_consensus_needs_one_rank(monkeypatch):
    t = Music2MIDI(_config()).model
    dist = torch.distributed
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(NotImplementedError, match="one GPU"):
        t.generate_consensus(None, 4)
