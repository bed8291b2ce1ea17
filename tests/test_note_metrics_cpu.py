"""CPU: the definition of the note-level metrics (music2midi_amd.note_metrics) against a brute force over every injective
assignment and on crafted cases with stated counts; what the device form (scoring.note_counts, csrc/note_match.hip) decides without a
device - the refusals of its entry point, the header against the binding, the ``ValueError``s of the Python layer - and the host
route of ``Music2MIDI.note_scores_batch`` / ``note_scores_recording`` for ids that are not on a GPU."""
import copy
import ctypes as C
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import confidence_cases as cc
import note_metrics_cases as nc
from music2midi_amd import confidence, evaluation, native, note_metrics, scoring
from music2midi_amd.config import DEFAULT_CONFIG, load_config
from music2midi_amd.input import ModelInputs
from music2midi_amd.model import Music2MIDI

ROOT = Path(__file__).resolve().parents[1]
FAKE = 0x100000                          # a device address that is never dereferenced: every refusal comes first
TOK = nc.TOK


# ------------------------------------------------------------------------------------------------ the definition
def _brute_force(hits: np.ndarray) -> int:
    """The largest number of label notes an injective assignment along hits can serve: every assignment is tried."""
    n_ref, n_est = hits.shape

    def best(u, used):
        if u == n_ref:
            return 0
        top = best(u + 1, used)                                # u stays alone
        for e in range(n_est):
            if hits[u, e] and not used >> e & 1:
                top = max(top, 1 + best(u + 1, used | 1 << e))
        return top
    return best(0, 0)


@pytest.mark.parametrize("ratio", [None, 0.2])
def test_definition_equals_brute_force_on_random_cases(ratio):
    rng = np.random.default_rng(11)
    sizes, nontrivial = 0, 0
    for _ in range(300):
        n, m = int(rng.integers(0, 7)), int(rng.integers(0, 7))
        on = rng.uniform(0.0, 0.25, n)                                       # off the grid
        labels = np.stack([on, on + rng.uniform(-0.05, 0.6, n), rng.integers(60, 62, n).astype(np.float64), np.full(n, 80.0)], axis=1)
        decoded = np.zeros((m, 4))                                           # on the 50 ms grid: near a label note, or anywhere
        for j in range(m):
            if n and rng.random() < 0.7:
                s, e, pitch, _ = labels[rng.integers(0, n)]
                a, b = int(round(s / 0.05)) + int(rng.integers(-1, 2)), int(round(e / 0.05)) + int(rng.integers(-2, 3))
            else:
                a, b, pitch = int(rng.integers(0, 6)), int(rng.integers(0, 16)), float(rng.integers(60, 62))
            decoded[j] = (a * 0.05, b * 0.05, pitch, 77.0)
        hits = note_metrics.hit_matrix(labels, decoded, offset_ratio=ratio)
        tp, n_ref, n_est = note_metrics.match_counts(labels, decoded, offset_ratio=ratio)
        assert all(type(v) is int for v in (tp, n_ref, n_est))
        assert (n_ref, n_est) == (int((labels[:, 1] > labels[:, 0]).sum()), int((decoded[:, 1] > decoded[:, 0]).sum())) == hits.shape
        want = _brute_force(hits)
        assert tp == want, (labels, decoded)
        sizes += want
        first_fit, used = 0, set()                             # the greedy answer, to know the cases are not all trivial
        for u in range(n_ref):
            e = next((e for e in range(n_est) if hits[u, e] and e not in used), None)
            if e is not None:
                used.add(e)
                first_fit += 1
        nontrivial += first_fit < want
    print(f"offset_ratio {ratio}: {sizes} pairs in all, first-fit short in {nontrivial} cases")
    assert sizes > 100 and nontrivial >= 1                     # the cases are not all empty, and not all trivial


@pytest.mark.parametrize("name", list(nc.CRAFTED))
def test_crafted_cases_have_the_stated_counts(name):
    labels, decoded, with_offsets, onsets_only = nc.CRAFTED[name]
    est = nc.est_seconds(decoded)
    assert note_metrics.match_counts(labels, est) == with_offsets
    assert note_metrics.match_counts(labels, est, offset_ratio=0.2, offset_min_tolerance=0.05, onset_tolerance=0.05) == with_offsets
    assert note_metrics.match_counts(labels, est, offset_ratio=None) == onsets_only
    assert np.array_equal(TOK.decode(nc.id_rows([decoded], 24))[0], est)     # the id rows of the GPU test decode to these notes


def test_crafted_details():
    # the onset that only the rounding makes a hit
    assert abs(1.0 - 21 * 0.05) == 0.050000000000000044 and abs(1.0 - 21 * 0.05) > 0.05
    # first-fit on the augmenting-path case finds one pair only
    labels, decoded, _, _ = nc.CRAFTED["augmenting path"]
    hits = note_metrics.hit_matrix(labels, nc.est_seconds(decoded))
    assert hits.tolist() == [[True, True], [True, False]]
    # decoded notes with end <= start are dropped as the labels' are
    est = np.array([[1.0, 1.5, 60, 77], [2.0, 2.0, 60, 77], [3.0, 2.9, 62, 77], [np.nan, 1.0, 60, 77]])
    assert note_metrics.match_counts(nc.ref((1.0, 1.5, 60), (2.0, 2.5, 60)), est) == (1, 2, 1)
    # int(pitch), on both sides
    assert note_metrics.match_counts(nc.ref((1.0, 1.5, 60.9)), np.array([[1.0, 1.5, 60.2, 77]])) == (1, 1, 1)
    # other tolerances
    assert note_metrics.match_counts(nc.ref((1.0, 1.5, 60)), nc.est_seconds([(22, 30, 60)]), onset_tolerance=0.1) == (1, 1, 1)
    assert note_metrics.match_counts(nc.ref((1.0, 2.0, 60)), nc.est_seconds([(20, 45, 60)]), offset_ratio=0.25) == (1, 1, 1)
    assert note_metrics.match_counts(nc.ref((1.0, 1.1, 60)), nc.est_seconds([(20, 24, 60)]), offset_min_tolerance=0.1) == (1, 1, 1)


def test_precision_recall_f1_edge_values():
    prf = note_metrics.precision_recall_f1
    assert prf(0, 0, 0) == (0.0, 0.0, 0.0) and prf(0, 5, 0) == (0.0, 0.0, 0.0) and prf(0, 0, 5) == (0.0, 0.0, 0.0)
    assert prf(0, 3, 4) == (0.0, 0.0, 0.0)                                    # p + r == 0
    assert prf(3, 3, 3) == (1.0, 1.0, 1.0)
    assert prf(1, 2, 4) == (0.25, 0.5, 2 * 0.25 * 0.5 / 0.75)
    assert prf(np.int64(2), np.int64(3), np.int64(7)) == (2 / 7, 2 / 3, 2 * (2 / 7) * (2 / 3) / (2 / 7 + 2 / 3))
    assert all(type(v) is float for v in prf(np.int64(2), np.int64(3), np.int64(7)))
    # NoteCounts micro-averages: the integers are summed first
    c = scoring.NoteCounts(np.array([[1, 0], [2, 0]]), np.array([[2, 0], [2, 3]]), np.array([[4, 4], [1, 1]]))
    assert c.precision.tolist() == [3 / 4, 0.0] and c.recall.tolist() == [3 / 5, 0.0] and c.f1.tolist() == [prf(3, 5, 4)[2], 0.0]
    assert c.per_timeline_f1.tolist() == [[prf(1, 4, 2)[2], 0.0], [prf(2, 1, 2)[2], 0.0]] and c.f1.dtype == np.float64
    d = evaluation.note_scores(c.tp, c.n_est, c.n_ref)
    assert d["tp"].tolist() == [3, 0] and d["n_est"].tolist() == [4, 3] and d["n_ref"].tolist() == [5, 5] and d["tp"].dtype == np.int64
    assert np.array_equal(d["f1"], c.f1) and np.array_equal(d["precision"], c.precision) and np.array_equal(d["recall"], c.recall)


# ------------------------------------------------------------------------------------------------ header, binding, refusals
def test_header_declares_what_the_binding_binds():
    header = (ROOT / "include" / "music2midi_amd.h").read_text()
    for name, proto in [
            ("m2m_score_note_counts", "int m2m_score_note_counts(const int32_t* notes_dev, const int32_t* counts_dev, const float* note_lp_dev, "
                                      "int R, int L, int sequential,"),
            ("m2m_score_note_workspace_bytes", "int64_t m2m_score_note_workspace_bytes(int R, int L, int n_labels, int n_thresholds);")]:
        assert proto in header, name
        assert name in native.EXPORTED_SYMBOLS and hasattr(native.load(), name)
    assert header.index("int m2m_score_chroma_counts(") < header.index("int m2m_score_note_counts(") < header.index("Audio ingest")
    assert "#define M2M_SCORE_MAX_THRESHOLDS 64" in header and scoring.MAX_THRESHOLDS == 64
    args = native._SIGNATURES["m2m_score_note_counts"][1]
    assert len(args) == 20 and [i for i, a in enumerate(args) if a is C.c_double] == [6, 11, 12, 13] and args[17] is C.c_int64
    assert native._SIGNATURES["m2m_score_note_workspace_bytes"] == (C.c_int64, [C.c_int] * 4)
    lib = native.load()
    for R, L, n, K in ((1, 1, 0, 1), (5, 64, 33, 1), (32, 1023, 8000, 16), (3, 7, 5, 64)):
        NE, arrays = R * L, lambda per, count: (per * count + 7) // 8 * 8
        want = 3 * arrays(8, n) + 2 * arrays(8, NE) + arrays(4, NE) + 3 * arrays(4, n) + arrays(4, NE) + 2 * arrays(4 * K, NE) + 2 * arrays(4 * K, n)
        assert lib.m2m_score_note_workspace_bytes(R, L, n, K) == want
    for bad in ((0, 1, 0, 1), (65536, 1, 0, 1), (1, 2049, 0, 1), (1, 1, -1, 1), (1, 1, 0, 0), (1, 1, 0, 65)):
        assert lib.m2m_score_note_workspace_bytes(*bad) == -1


def _call(R=4, L=72, seq=0, ts=0.05, labels=FAKE, offsets=FAKE, n_labels=10, T=None, onset=0.05, ratio=0.2, floor=0.05, thr=FAKE, K=3,
          lp=FAKE, ws=FAKE, ws_bytes=None, notes=FAKE, counts=FAKE, out=FAKE):
    lib = native.load()
    T = (1 if seq else R) if T is None else T
    if ws_bytes is None:
        ws_bytes = max(8, lib.m2m_score_note_workspace_bytes(R, L, n_labels, K))
    st = lib.m2m_score_note_counts(notes, counts, lp, R, L, seq, ts, labels, offsets, n_labels, T, onset, ratio, floor, thr, K, ws, ws_bytes,
                                   out, None)
    return st, lib.m2m_last_error().decode()


@pytest.mark.parametrize("kw,msg", [
    (dict(R=0, T=0), "0 rows out of range"),
    (dict(R=65536), "65536 rows out of range"),
    (dict(L=0), "L=0 out of range"),
    (dict(L=2049), "L=2049 out of range"),
    (dict(seq=2, T=1), "sequential must be 0 or 1"),
    (dict(R=4, T=3), "3 timelines for 4 rows"),
    (dict(R=4, seq=1, T=4), "4 timelines for 4 rows"),
    (dict(ts=0.0), "time_step 0 out of range"),
    (dict(ts=float("nan")), "time_step nan out of range"),
    (dict(ts=float("inf")), "time_step inf out of range"),
    (dict(n_labels=-1), "-1 label notes out of range"),
    (dict(n_labels=(1 << 24) + 1), "label notes out of range"),
    (dict(K=0), "0 thresholds out of range"),
    (dict(K=65), "65 thresholds out of range"),
    (dict(onset=-0.01), "onset_tolerance -0.01 out of range"),
    (dict(onset=float("nan")), "onset_tolerance nan out of range"),
    (dict(ratio=float("nan")), "offset_ratio nan out of range"),
    (dict(ratio=float("inf")), "offset_ratio inf out of range"),
    (dict(floor=-1.0), "offset_min_tolerance -1 out of range"),
    (dict(floor=float("nan")), "offset_min_tolerance nan out of range"),
    (dict(notes=None), "null notes"),
    (dict(counts=None), "null notes"),
    (dict(offsets=None), "null notes"),
    (dict(out=None), "null notes"),
    (dict(labels=None, n_labels=3), "null labels"),
    (dict(lp=None, K=3), "3 thresholds need the notes' log-probabilities"),
    (dict(thr=None, K=1), "null min_logprobs with log-probabilities"),
    (dict(ws=None), "null or misaligned workspace"),
    (dict(ws=FAKE + 4), "null or misaligned workspace"),
    (dict(ws_bytes=64), "workspace of 64 bytes"),
])
def test_note_counts_refuses_on_the_arguments_alone(kw, msg):
    st, err = _call(**kw)
    assert st == -1 and msg in err and "m2m_score_note_counts" in err, err


def test_python_layer_refuses_before_the_library():
    ids = torch.zeros((2, 8), dtype=torch.long)
    two = [np.zeros((0, 4))] * 2
    with pytest.raises(ValueError, match="need token_logprobs"):
        scoring.note_counts(TOK, ids, two, thresholds=[0.0, 0.5])
    with pytest.raises(ValueError, match="need token_logprobs"):
        evaluation.note_scores_tokens(TOK, ids, two, thresholds=[0.3])
    with pytest.raises(ValueError, match="CUDA int64"):                     # thresholds of at most 0 pass: the ids are looked at next
        scoring.note_counts(TOK, ids, two, thresholds=[0.0, -1.0])
    with pytest.raises(ValueError, match="min_confidence has to be a probability"):
        scoring.note_counts(TOK, ids, two, token_logprobs=torch.zeros((2, 8)), thresholds=[0.5, 1.5])
    with pytest.raises(ValueError, match="0 thresholds out of range"):
        scoring.note_counts(TOK, ids, two, thresholds=[])
    with pytest.raises(ValueError, match="65 thresholds out of range"):
        scoring.note_counts(TOK, ids, two, token_logprobs=torch.zeros((2, 8)), thresholds=[0.5] * 65)
    for kw, what in ((dict(onset_tolerance=-0.1), "onset_tolerance"), (dict(offset_min_tolerance=float("nan")), "offset_min_tolerance"),
                     (dict(offset_ratio=-0.5), "offset_ratio"), (dict(offset_ratio=float("nan")), "offset_ratio")):
        with pytest.raises(ValueError, match=what):
            scoring.note_counts(TOK, ids, two, **kw)
    with pytest.raises(ValueError, match="Invalid argument mode=both"):
        scoring.note_counts(TOK, ids, two, mode="both")
    assert scoring.threshold_logprobs(None, False).tolist() == [-np.inf] and scoring.threshold_logprobs(None, False).dtype == np.float32
    assert scoring.threshold_logprobs([0.0, 0.5, 1.0], True).tolist() == [-np.inf, float(np.float32(np.log(0.5))), 0.0]


def test_label_checks_of_the_python_layer(monkeypatch):
    """The number of label arrays and their eligibility are checked after the detokenise, which needs a device: it is replaced by a
    stand-in that returns the shapes a decode of these ids would have."""
    ids = torch.zeros((2, 8), dtype=torch.long)
    fake = scoring.DeviceNotes(torch.zeros((2, 8, 3), dtype=torch.int32), torch.zeros(2, dtype=torch.int32), "batched", 0.05, 80, 0)
    monkeypatch.setattr(scoring, "detokenize", lambda *a, **k: fake)
    good = np.array([[0.1, 0.5, 60, 80.0]])
    with pytest.raises(ValueError, match="3 label arrays for 2 timelines"):
        scoring.note_counts(TOK, ids, [good] * 3)
    with pytest.raises(ValueError, match="1 label arrays for 2 timelines"):
        scoring.note_counts(TOK, ids, [good])
    for bad, why in ((np.array([[0.1, 0.5, 128, 80.0]]), "a pitch outside 0..127"), (np.array([[0.1, 0.5, 60, 0.5]]), "a velocity below 1"),
                     (np.array([[-0.1, 0.5, 60, 80.0]]), "a negative start"), (np.zeros((2, 3)), "is not")):
        with pytest.raises(ValueError, match=f"note_counts: the labels are not eligible for the device path: timeline 1: .*{why}"):
            scoring.note_counts(TOK, ids, [good, bad])
        with pytest.raises(ValueError, match="not eligible"):
            evaluation.note_scores_tokens(TOK, ids, [good, bad])


def test_note_scores_tokens_is_exported_next_to_evaluate_tokens():
    import music2midi.evaluation as drop_in
    assert drop_in.note_scores_tokens is evaluation.note_scores_tokens


# ------------------------------------------------------------------------------------------------ Music2MIDI without a device
class _Host:
    """``Music2MIDI``'s inference methods over a stand-in model that "decodes" fixed CPU rows, two segments per call."""
    for _name in ("note_scores_batch", "note_scores_recording", "sample_scored_rows", "sample_token_rows", "_segment_chunks",
                  "_padded_segments", "_resolve_audio", "_segment_length", "_device_ingest", "_grammar_kwargs"):
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
        self.calls.append(dict(kw, max_length=max_length))
        lo, hi = self.next_row, self.next_row + inputs.input_waveform.shape[0]
        self.next_row = hi % len(self.ids)
        ids = self.ids[lo:hi]
        width = max(2, int((ids != 0).any(0).nonzero().max()) + 1)
        if not kw.get("return_dict_in_generate"):
            return ids[:, :width]
        return SimpleNamespace(sequences=ids[:, :width], logprobs=self.lp[lo:hi, 1:width])


def _same(got, want):
    assert set(got) == set(want) == {"precision", "recall", "f1", "tp", "n_est", "n_ref"}
    for name in want:
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (name, got[name], want[name])


def _definition(labels, decoded_per_threshold, ratio):
    """The dict from ``match_counts`` alone: per threshold, the integers summed over the timelines, then the three ratios."""
    sums = np.array([np.sum([note_metrics.match_counts(l, d, offset_ratio=ratio) for l, d in zip(labels, decoded)], axis=0)
                     for decoded in decoded_per_threshold], dtype=np.int64).reshape(-1, 3)
    prf = np.array([note_metrics.precision_recall_f1(*s) for s in sums.tolist()], dtype=np.float64).reshape(-1, 3)
    return {"precision": prf[:, 0], "recall": prf[:, 1], "f1": prf[:, 2], "tp": sums[:, 0], "n_ref": sums[:, 1], "n_est": sums[:, 2]}


def test_note_scores_batch_scores_cpu_ids_by_the_definition(monkeypatch):
    from music2midi_amd import model as model_mod
    monkeypatch.setattr(model_mod, "note_scores_tokens", lambda *a, **k: pytest.fail("the device path was taken for host ids"))
    labels, ids, lp = cc.fuzz(2, 64, 0.10, 22)
    ids[:, 0], lp[:, 0] = 0, 0.0
    labels = [TOK.decode(ids)[r][::2] + [0.012, 0.02, 0, 0] for r in range(2)]          # labels some decoded notes hit
    inputs = ModelInputs(input_waveform=torch.zeros(2, 8), notes_batch=tuple(labels), cond_index=None)
    budget = 4 * max(len(l) for l in labels)
    thresholds = [0.0, 0.5, 0.9]
    for ratio in (0.2, None):
        m = _Host(ids, lp, midi_grammar=True)
        got = m.note_scores_batch(inputs, thresholds=thresholds, offset_ratio=ratio)
        assert m.calls == [dict(return_dict_in_generate=True, output_logprobs=True, midi_grammar=True, max_length=budget)]
        kept = [confidence.decode_with_confidence(TOK, ids, lp, min_confidence=c)[0] for c in thresholds]
        _same(got, _definition(labels, kept, ratio))
        assert got["n_est"][0] > got["n_est"][1] > 0 and got["tp"][0] > 0 and got["n_ref"].tolist() == [sum(len(l) for l in labels)] * 3
        plain = _Host(ids, lp)
        _same(plain.note_scores_batch(inputs, offset_ratio=ratio), _definition(labels, [TOK.decode(ids)], ratio))
        assert plain.calls == [dict(max_length=budget)]                              # no log-probabilities without a positive threshold
        _same(plain.note_scores_batch(inputs, thresholds=[0.0, -2.0], offset_ratio=ratio), _definition(labels, [TOK.decode(ids)] * 2, ratio))
    with pytest.raises(ValueError, match="min_confidence has to be a probability"):
        _Host(ids, lp).note_scores_batch(inputs, thresholds=[0.5, 1.5])
    beams = _Host(ids, lp, num_beams=2)
    with pytest.raises(ValueError, match="num_beams > 1"):
        beams.note_scores_batch(inputs, thresholds=[0.5])
    assert beams.calls == []


def test_note_scores_batch_scores_ineligible_labels_by_the_definition(monkeypatch):
    from music2midi_amd import model as model_mod

    class OnGpu(torch.Tensor):
        is_cuda = True

    _, ids, lp = cc.fuzz(2, 64, 0.10, 22)
    decoded = TOK.decode(ids)
    good = [d[::2] + [0.012, 0.02, 0, 0] for d in decoded]
    bad = [good[0], np.concatenate([good[1], [[0.5, 1.0, 64, 0.5]]])]              # a velocity numpy_to_midi truncates to 0
    m = _Host(ids, lp)
    m.ids = m.ids.as_subclass(OnGpu)
    m._decode = lambda inputs, max_length, **kw: m.ids
    m.model.generate = m._decode
    taken = []
    monkeypatch.setattr(model_mod, "note_scores_tokens", lambda *a, **k: taken.append((a, k)) or "device")
    got = m.note_scores_batch(ModelInputs(input_waveform=torch.zeros(2, 8), notes_batch=tuple(bad), cond_index=None))
    assert not taken
    _same(got, _definition(bad, [decoded], 0.2))
    assert got["n_ref"].tolist() == [len(bad[0]) + len(bad[1])]                   # the definition keeps the note the device path refuses
    assert m.note_scores_batch(ModelInputs(input_waveform=torch.zeros(2, 8), notes_batch=tuple(good), cond_index=None)) == "device"
    assert len(taken) == 1 and taken[0][0][1] is m.ids and taken[0][1]["thresholds"] is None


def test_note_scores_recording_scores_cpu_ids_by_the_definition():
    _, ids, lp = cc.fuzz(3, 64, 0.10, 21)
    ids[2, 30:] = 0                                           # the second call returns fewer columns than the first
    ids[:, 0], lp[:, 0] = 0, 0.0
    audio = np.zeros(int(2.5 * 3 * 16000), dtype=np.float32)  # 2.5 segments of audio: three rows
    everything = TOK.decode(ids, mode="sequential", duration_per_batch=3)
    label = everything[::2] + [0.012, 0.02, 0, 0]
    thresholds = [0.0, 0.4, 1.0]
    for ratio in (0.2, None):
        m = _Host(ids, lp)
        got = m.note_scores_recording(label, audio_y=audio, thresholds=thresholds, offset_ratio=ratio)
        assert m.calls == [dict(return_dict_in_generate=True, output_logprobs=True, max_length=1024)] * 2
        kept = [[confidence.decode_with_confidence(TOK, ids, lp, "sequential", 3, c)[0]] for c in thresholds]
        _same(got, _definition([label], kept, ratio))
        assert got["n_est"][0] == len(everything) > got["n_est"][1] > got["n_est"][2] and got["tp"][0] > 0
        plain = _Host(ids, lp)
        _same(plain.note_scores_recording(label, audio_y=audio, offset_ratio=ratio), _definition([label], [[everything]], ratio))
        assert plain.calls == [dict(max_length=1024)] * 2
    beams = _Host(ids, lp, num_beams=2)
    with pytest.raises(ValueError, match="num_beams > 1"):
        beams.note_scores_recording(label, audio_y=audio, thresholds=[0.3])
    assert beams.calls == []
