"""GPU: note-level matching on the device (scoring.note_counts, csrc/note_match.hip) against its definition on the host
(music2midi_amd.note_metrics): the three integers are compared with ``==`` - on the crafted cases, on random batches, on long
augmenting chains, across the rows of a sequential decode, under a sweep of confidence thresholds, and end to end through
``Music2MIDI`` on random-init weights."""
import copy

import numpy as np
import pytest
import torch

import note_metrics_cases as nc
from music2midi_amd import confidence, evaluation, note_metrics, scoring, synth
from music2midi_amd.config import DEFAULT_CONFIG, T5Geometry

pytestmark = pytest.mark.gpu
TOK = nc.TOK
RATIOS = (None, 0.2)


def _want(labels, decoded, ratio):
    """[T, 3] (tp, n_est, n_ref) of the definition."""
    rows = [note_metrics.match_counts(l, d, offset_ratio=ratio) for l, d in zip(labels, decoded)]
    return np.asarray([(tp, n_est, n_ref) for tp, n_ref, n_est in rows], dtype=np.int64).reshape(-1, 3)


def _got(c, k=0):
    return np.stack([c.tp[:, k], c.n_est[:, k], c.n_ref[:, k]], axis=1)


def _check_batched(ids, labels, ratio):
    ids_dev = torch.from_numpy(ids).cuda()
    decoded = scoring.detokenize(TOK, ids_dev).to_numpy()
    assert all(np.array_equal(a, b) for a, b in zip(decoded, TOK.decode(ids)))
    c = scoring.note_counts(TOK, ids_dev, labels, offset_ratio=ratio)
    assert c.tp.dtype == np.int64 and c.tp.shape == c.n_est.shape == c.n_ref.shape == (len(ids), 1)
    want = _want(labels, decoded, ratio)
    assert np.array_equal(_got(c), want), (ratio, _got(c).tolist(), want.tolist())
    return c, want


def test_crafted_cases_through_the_kernel():
    names = list(nc.CRAFTED)
    ids = nc.id_rows([nc.CRAFTED[n][1] for n in names], 24)
    labels = [nc.CRAFTED[n][0] for n in names]
    for r, n in enumerate(names):                              # the rows decode to the notes the case states
        assert np.array_equal(TOK.decode(ids[r:r + 1])[0], nc.est_seconds(nc.CRAFTED[n][1])), n
    for ratio, col in ((0.2, 2), (None, 3)):
        c, _ = _check_batched(ids, labels, ratio)
        for r, n in enumerate(names):
            tp, n_ref, n_est = nc.CRAFTED[n][col]
            assert (int(c.tp[r, 0]), int(c.n_ref[r, 0]), int(c.n_est[r, 0])) == (tp, n_ref, n_est), (n, ratio)
    # one case alone (one row, one workgroup per pitch) and the micro-average of the batch
    c = scoring.note_counts(TOK, torch.from_numpy(ids[:1]).cuda(), labels[:1])
    assert (int(c.tp[0, 0]), int(c.n_ref[0, 0]), int(c.n_est[0, 0])) == nc.CRAFTED["augmenting path"][2]
    assert c.precision.tolist() == [1.0] and c.recall.tolist() == [1.0] and c.f1.tolist() == [1.0]
    c, want = _check_batched(ids, labels, 0.2)
    p, r, f = note_metrics.precision_recall_f1(want[:, 0].sum(), want[:, 2].sum(), want[:, 1].sum())
    assert (c.precision[0], c.recall[0], c.f1[0]) == (p, r, f) and c.per_timeline_f1.shape == (len(names), 1)
    scores = evaluation.note_scores_tokens(TOK, torch.from_numpy(ids).cuda(), labels)
    assert scores["f1"].tolist() == [f] and scores["tp"].tolist() == [want[:, 0].sum()] and scores["n_ref"].tolist() == [want[:, 2].sum()]


@pytest.mark.parametrize("seed", range(20))
def test_random_batches(seed):
    rng = np.random.default_rng(100 + seed)
    cases = [nc.random_case(rng) for _ in range(5)]
    ids = nc.tokenised([c[1] for c in cases], 64)
    labels = [c[0] for c in cases]
    for ratio in RATIOS:
        _, want = _check_batched(ids, labels, ratio)
    assert want[:, 1].sum() > 0


@pytest.mark.parametrize("seed", range(6))
def test_long_augmenting_chains(seed):
    """One pitch, 40 label notes 10 ms apart with varied durations, a decoded note on every grid step: every label note has two or
    three candidates by onset and the offsets decide which, so the matching is found through augmenting paths many notes long."""
    rng = np.random.default_rng(200 + seed)
    on = 0.30 + 0.01 * np.arange(40)
    labels = [np.stack([on, on + rng.uniform(0.08, 0.9, 40), np.full(40, 60.0), np.full(40, 80.0)], axis=1)]
    decoded = [(i, i + int(rng.integers(2, 20)), 60) for i in range(21)]
    ids = nc.id_rows([decoded], 128)
    assert np.array_equal(TOK.decode(ids)[0], nc.est_seconds(decoded))
    for ratio in RATIOS:
        _, want = _check_batched(ids, labels, ratio)
        print(f"chains, seed {seed}, offset_ratio {ratio}: tp {want[0, 0]} of {want[0, 1]} decoded / {want[0, 2]} label notes")
    assert want[0, 1] == 21 and want[0, 2] == 40


def _sequential_case(seed):
    rng = np.random.default_rng(300 + seed)
    labels, decoded = nc.random_case(rng, max_notes=24, span=8.5)
    # notes on both sides of the row boundaries at 3 s and 6 s, of one pitch: rows 0 and 1 (1 and 2) compete for the same labels
    labels = np.concatenate([labels, nc.ref((2.99, 3.40, 61), (3.01, 3.35, 61), (5.97, 6.50, 60), (6.02, 6.60, 60))])
    decoded = decoded + [(59, 68, 61), (60, 67, 61), (119, 130, 60), (120, 131, 60), (121, 133, 60)]
    rows = [[n for n in decoded if n[0] // 60 == r] for r in range(3)]
    return labels, nc.id_rows(rows, 6 * max(len(r) for r in rows) + 1, steps_per_row=60)


@pytest.mark.parametrize("seed", range(4))
def test_sequential_rows_are_one_timeline(seed):
    label, ids = _sequential_case(seed)
    ids_dev = torch.from_numpy(ids).cuda()
    decoded = scoring.detokenize(TOK, ids_dev, "sequential", 3).to_numpy()
    assert np.array_equal(decoded, TOK.decode(ids, mode="sequential", duration_per_batch=3)) and decoded[:, 0].max() >= 6.0
    for ratio in RATIOS:
        c = scoring.note_counts(TOK, ids_dev, label, mode="sequential", duration_per_batch=3, offset_ratio=ratio)
        want = _want([label], [decoded], ratio)
        assert c.tp.shape == (1, 1) and np.array_equal(_got(c), want), (ratio, _got(c).tolist(), want.tolist())
        assert want[0, 0] >= 4                                  # the boundary notes are matched, whichever row decoded them
    with pytest.raises(ValueError, match="2 label arrays for 3 timelines"):
        scoring.note_counts(TOK, ids_dev, [label] * 2)


def _threshold_case():
    """(labels, ids [4, 64], lp [4, 64]): closed groups of six ids per note, so every note has six tokens of its own; a NaN in the
    first note of row 0, -inf in its second."""
    rng = np.random.default_rng(7)
    cases = [nc.random_case(rng, max_notes=9) for _ in range(4)]
    cases = [(l, d[:10]) for l, d in cases]
    ids = nc.id_rows([c[1] for c in cases], 64)
    lp = (-rng.exponential(0.12, ids.shape)).astype(np.float32)
    assert len(cases[0][1]) >= 2
    lp[0, 2] = np.float32(np.nan)
    lp[0, 8] = np.float32(-np.inf)
    return [c[0] for c in cases], ids, lp


def test_threshold_sweep_in_one_launch():
    labels, ids, lp = _threshold_case()
    notes, conf = confidence.decode_with_confidence(TOK, ids, lp)
    assert np.isnan(conf[0][0]) and conf[0][1] == 0.0
    flat = np.sort(np.concatenate(conf))
    flat = flat[np.isfinite(flat) & (flat > 0)]
    own = float(flat[len(flat) // 2])                          # one note lies exactly on this threshold: it is kept
    totals = np.concatenate([confidence.total_logprob(confidence.note_logprobs(TOK, ids[r], lp[r])[1]) for r in range(4)])
    assert (totals == confidence.min_logprob(own)).sum() == 1
    thresholds = [0.0, 0.3, own, own * (1 + 1e-5), 1.0]
    ids_dev, lp_dev = torch.from_numpy(ids).cuda(), torch.from_numpy(lp).cuda()
    for ratio in RATIOS:
        c = scoring.note_counts(TOK, ids_dev, labels, token_logprobs=lp_dev, thresholds=thresholds, offset_ratio=ratio)
        assert c.tp.shape == (4, 5) and c.f1.shape == (5,) and c.per_timeline_f1.shape == (4, 5)
        for k, floor in enumerate(thresholds):
            kept, _ = confidence.decode_with_confidence(TOK, ids, lp, min_confidence=floor)
            want = _want(labels, kept, ratio)
            assert np.array_equal(_got(c, k), want), (ratio, floor, _got(c, k).tolist(), want.tolist())
        assert c.n_est[:, 0].sum() == sum(len(n) for n in notes)
        assert c.n_est[:, 2].sum() == c.n_est[:, 3].sum() + 1      # the note on the threshold leaves one step above it
        assert c.n_est[0, 4] == 1 and (c.n_est[1:, 4] == 0).all()  # only the NaN total survives a threshold of 1
        assert (np.diff(c.n_est.sum(axis=0)) <= 0).all() and (c.n_ref == c.n_ref[:, :1]).all()
        scores = evaluation.note_scores_tokens(TOK, ids_dev, labels, token_logprobs=lp_dev, thresholds=thresholds, offset_ratio=ratio)
        assert np.array_equal(scores["precision"], c.precision) and np.array_equal(scores["tp"], c.tp.sum(axis=0))
        # one threshold without log-probabilities is the threshold 0
        plain = scoring.note_counts(TOK, ids_dev, labels, offset_ratio=ratio)
        zero = scoring.note_counts(TOK, ids_dev, labels, token_logprobs=lp_dev, thresholds=[0.0], offset_ratio=ratio)
        assert np.array_equal(_got(plain), _got(c, 0)) and np.array_equal(_got(zero), _got(c, 0))
        assert np.array_equal(_got(scoring.note_counts(TOK, ids_dev, labels, thresholds=[0.0, -1.0], offset_ratio=ratio), 1), _got(c, 0))
    # 64 thresholds in one launch
    many = np.linspace(0.0, 1.0, 64).tolist()
    c = scoring.note_counts(TOK, ids_dev, labels, token_logprobs=lp_dev, thresholds=many)
    for k in (0, 17, 40, 63):
        kept, _ = confidence.decode_with_confidence(TOK, ids, lp, min_confidence=many[k])
        assert np.array_equal(_got(c, k), _want(labels, kept, 0.2)), k
    with pytest.raises(ValueError, match="65 thresholds out of range"):
        scoring.note_counts(TOK, ids_dev, labels, token_logprobs=lp_dev, thresholds=[0.5] * 65)


def test_bad_rows_and_no_side_effect_on_chroma_counts():
    labels, ids, lp = _threshold_case()
    ids_dev, lp_dev = torch.from_numpy(ids).cuda(), torch.from_numpy(lp).cuda()
    before = scoring.chroma_counts(TOK, ids_dev, labels)
    before_scored = scoring.chroma_counts(TOK, ids_dev, labels, token_logprobs=lp_dev, min_confidence=0.5)
    scoring.note_counts(TOK, ids_dev, labels, token_logprobs=lp_dev, thresholds=[0.0, 0.5, 0.9])
    scoring.note_counts(TOK, ids_dev, labels, offset_ratio=None)
    for was, call in ((before, lambda: scoring.chroma_counts(TOK, ids_dev, labels)),
                      (before_scored, lambda: scoring.chroma_counts(TOK, ids_dev, labels, token_logprobs=lp_dev, min_confidence=0.5))):
        now = call()
        for name in ("correct", "voiced", "frames"):
            assert np.array_equal(getattr(now, name), getattr(was, name)), name
        assert now.score == was.score
    assert np.array_equal(ids_dev.cpu().numpy(), ids)
    bad = ids.copy()
    bad[2, 5] = 400
    for kw in (dict(), dict(token_logprobs=lp_dev, thresholds=[0.0, 0.5])):
        with pytest.raises(ValueError, match="token row 2 holds an id outside"):
            scoring.note_counts(TOK, torch.from_numpy(bad).cuda(), labels, **kw)
    # the kernel's own answer for that call: tp = -1 for the timeline of the bad row, the others are unharmed
    dn = scoring.detokenize(TOK, torch.from_numpy(bad).cuda())
    packed, offsets, _ = scoring._pack_labels(labels)
    lab, off = torch.from_numpy(packed).cuda(), torch.from_numpy(offsets).cuda()
    from music2midi_amd import native
    lib = native.load()
    need = lib.m2m_score_note_workspace_bytes(4, 64, packed.shape[1], 1)
    ws = torch.empty(need // 8, dtype=torch.int64, device="cuda")
    out = torch.empty((4, 1, 3), dtype=torch.int32, device="cuda")
    native.check(lib.m2m_score_note_counts(dn.notes.data_ptr(), dn.counts.data_ptr(), None, 4, 64, 0, TOK.time_step, lab.data_ptr(),
                                           off.data_ptr(), packed.shape[1], 4, 0.05, 0.2, 0.05, None, 1, ws.data_ptr(), need,
                                           out.data_ptr(), native.stream_handle(out.device)), "m2m_score_note_counts")
    out = out.cpu().numpy()[:, 0]
    good = _got(scoring.note_counts(TOK, ids_dev, labels))
    assert out[2].tolist() == [-1, 0, 0] and np.array_equal(np.delete(out, 2, axis=0), np.delete(good, 2, axis=0))
    # no rows at all
    none = scoring.note_counts(TOK, torch.zeros((0, 5), dtype=torch.long).cuda(), [])
    assert none.tp.shape == (0, 1) and none.f1.tolist() == [0.0]


# ------------------------------------------------------------------------------------------------ Music2MIDI
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
    m = m.cuda().eval()
    m.config.inference["midi_grammar"] = True                  # random weights close notes only under the token grammar
    return m


def _recorded(m, call):
    """(the call's result, [(keywords, output)] of every ``model.generate`` it made)."""
    seen, real = [], m.model.generate

    def recording(*a, **kw):
        out = real(*a, **kw)
        seen.append((kw, out))
        return out
    m.model.generate = recording
    try:
        return call(), seen
    finally:
        m.model.generate = real


def _same(got, want):
    assert set(got) == set(want) == {"precision", "recall", "f1", "tp", "n_est", "n_ref"}
    for name in want:
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (name, got[name], want[name])


def test_music2midi_note_scores(random_init_model):
    from music2midi_amd.input import ModelInputs
    m = random_init_model
    # a labelled batch
    wav = torch.from_numpy(synth.waveform_batch(40, 2, 48000))
    idx = torch.from_numpy(synth.cond_index_batch(40, 2))
    probe = m.model.generate(ModelInputs(input_waveform=wav.cuda(), cond_index=idx.cuda()), max_length=48, midi_grammar=True)
    decoded = TOK.decode(probe.cpu().numpy())
    labels = tuple(np.concatenate([d[::2] + [0.013, 0.021, 0, 0], [[0.5, 2.5, 60, 80]] * (12 - len(d[::2]))])[:12] for d in decoded)
    assert all(len(l) == 12 for l in labels)                   # the budget of the decode: 4 * 12 = 48 ids
    inputs = ModelInputs(input_waveform=wav.cuda(), notes_batch=labels, cond_index=idx.cuda())
    plain, seen = _recorded(m, lambda: m.note_scores_batch(inputs))
    assert len(seen) == 1 and seen[0][0]["max_length"] == 48 and "output_logprobs" not in seen[0][0] and seen[0][0]["midi_grammar"] is True
    ids = seen[0][1].cpu().numpy()
    print(f"labelled batch: {[len(d) for d in TOK.decode(ids)]} notes decoded, {plain}")
    _same(plain, evaluation.note_scores_host(TOK, ids, labels))
    assert plain["n_ref"].tolist() == [24]
    for ratio in RATIOS:
        swept, seen = _recorded(m, lambda: m.note_scores_batch(inputs, thresholds=[0.0, 0.4, 0.8], offset_ratio=ratio))
        assert len(seen) == 1 and seen[0][0]["output_logprobs"] is True and seen[0][0]["max_length"] == 48
        s_ids = seen[0][1].sequences.cpu().numpy()
        s_lp = np.concatenate([np.zeros((2, 1), dtype=np.float32), seen[0][1].logprobs.cpu().numpy()], axis=1)
        _same(swept, evaluation.note_scores_host(TOK, s_ids, labels, token_logprobs=s_lp, thresholds=[0.0, 0.4, 0.8], offset_ratio=ratio))
    for name in plain:                                         # threshold 0 of the scored path is the plain path
        assert swept[name][0] == plain[name][0], name
    # a recording of three segments
    audio = synth.waveform(33, 7 * 16000)
    notes = m.generate_notes(audio_y=audio, cond_index=[4, 2])
    label = np.concatenate([notes[::2] + [0.013, 0.021, 0, 0], [[0.5, 2.5, 60, 80]]])
    plain, seen = _recorded(m, lambda: m.note_scores_recording(label, audio_y=audio, cond_index=[4, 2]))
    assert len(seen) == 1
    _same(plain, evaluation.note_scores_host(TOK, seen[0][1].cpu().numpy(), label, "sequential", 3))
    tp, n_ref, n_est = note_metrics.match_counts(label, notes)
    assert (plain["tp"].tolist(), plain["n_ref"].tolist(), plain["n_est"].tolist()) == ([tp], [n_ref], [n_est])
    swept, seen = _recorded(m, lambda: m.note_scores_recording(label, audio_y=audio, cond_index=[4, 2], thresholds=[0.0, 0.5, 1.0]))
    s_ids = seen[0][1].sequences.cpu().numpy()
    s_lp = np.concatenate([np.zeros((3, 1), dtype=np.float32), seen[0][1].logprobs.cpu().numpy()], axis=1)
    _same(swept, evaluation.note_scores_host(TOK, s_ids, label, "sequential", 3, token_logprobs=s_lp, thresholds=[0.0, 0.5, 1.0]))
    print(f"recording: {len(notes)} notes, {swept}")
    for name in plain:
        assert swept[name][0] == plain[name][0], name
    assert swept["n_est"][0] == len(notes) and (np.diff(swept["n_est"]) <= 0).all()
