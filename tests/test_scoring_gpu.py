"""GPU: the on-device scoring (music2midi_amd.scoring, csrc/score.hip) against the host functions it replaces -
``MidiTokenizer.decode``, ``numpy_to_midi`` and ``evaluation`` - which stay the definition.  Every comparison is exact
(``np.array_equal`` on the notes, ``==`` on the counts and on the float); every expected value is computed here from the host
functions."""
import copy

import numpy as np
import pytest
import torch

from music2midi_amd import evaluation, scoring, synth
from music2midi_amd.config import DEFAULT_CONFIG, T5Geometry, load_config
from music2midi_amd.input import ModelInputs
from music2midi_amd.tokenizer import BOS, EOS, OFFSET, ONSET, PAD, MidiTokenizer
from music2midi_amd.utils import numpy_to_midi

pytestmark = pytest.mark.gpu


def _tokenizer(**tok):
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["tokenizer"].update(tok)
    return MidiTokenizer(load_config(cfg))


TOK = _tokenizer()
P, T = TOK.pitch_token_offset, TOK.time_token_offset


def _pad_rows(rows, width=None):
    width = max(len(r) for r in rows) if width is None else width
    out = np.full((len(rows), width), PAD, dtype=np.int64)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return torch.from_numpy(out)


def _host_counts(label, decoded):
    """(correct, voiced, frames) of one timeline, recomputed from the host's melodies."""
    tm, om = evaluation.extract_midi_melody(numpy_to_midi(label), numpy_to_midi(decoded))
    both = (tm >= 0) & (om >= 0)
    return int((both & ((tm - om) % 12 == 0)).sum()), int((tm >= 0).sum()), len(tm)


def _host_score(labels, decoded):
    return evaluation.evaluate_batch([numpy_to_midi(n) for n in labels], [numpy_to_midi(n) for n in decoded])


def _check_batched(tok, ids, labels):
    """notes, counts per timeline and the float of a batched call against the host; returns the host's score."""
    decoded = tok.decode(ids, mode="batched")
    got = scoring.detokenize(tok, ids.cuda()).to_numpy()
    assert isinstance(got, list) and len(got) == len(decoded)
    for r, (g, w) in enumerate(zip(got, decoded)):
        assert g.dtype == np.float64 and g.shape == w.shape and np.array_equal(g, w), r
    counts = scoring.chroma_counts(tok, ids.cuda(), labels)
    want = np.array([_host_counts(l, d) for l, d in zip(labels, decoded)], dtype=np.int64).reshape(-1, 3)
    for name, col in (("correct", 0), ("voiced", 1), ("frames", 2)):
        g = getattr(counts, name)
        assert g.dtype == np.int64 and np.array_equal(g, want[:, col]), (name, g, want[:, col])
    host = _host_score(labels, decoded)
    assert counts.score == host and evaluation.evaluate_tokens(tok, ids.cuda(), labels) == host
    return host


# ------------------------------------------------------------------------------------------------ 1. one behaviour per row
def t(i):
    return T + i


def p(n):
    return P + n


HAND_ROWS = {
    # name: (tokens, closed notes the host must report - a check that the row shows the behaviour it is named for)
    "plain group": ([t(0), ONSET, p(60), p(64), t(10), OFFSET, p(60), p(64), EOS], 2),
    "pitch between time and ONSET": ([t(0), p(60), ONSET, p(62), t(5), OFFSET, p(60), p(62), EOS], 2),
    "pitch between time and OFFSET": ([t(0), ONSET, p(60), t(5), p(60), OFFSET, t(7), OFFSET, p(60), EOS], 1),
    "OFFSET closes two notes of one pitch": ([t(0), ONSET, p(60), t(2), ONSET, p(60), t(6), OFFSET, p(60), EOS], 2),
    "OFFSET at the onset's own index": ([t(3), ONSET, p(60), OFFSET, p(60), t(9), ONSET, p(61), EOS], 0),
    "OFFSET at the onset's own index, closed later": ([t(3), ONSET, p(60), OFFSET, p(60), t(9), OFFSET, p(60), EOS], 1),
    "time goes backwards": ([t(10), ONSET, p(60), t(4), ONSET, p(60), t(6), OFFSET, p(60), t(12), OFFSET, p(60), EOS], 2),
    "time goes backwards, the future note stays open": ([t(10), ONSET, p(60), t(4), ONSET, p(60), t(6), OFFSET, p(60), EOS], 1),
    "unclosed note": ([t(0), ONSET, p(60), p(61), t(5), OFFSET, p(61), EOS], 1),
    "tokens after EOS": ([t(0), ONSET, p(60), t(5), OFFSET, p(60), EOS, t(6), ONSET, p(70), t(9), OFFSET, p(70)], 1),
    "PAD and BOS inside": ([BOS, t(0), ONSET, PAD, p(60), t(5), PAD, OFFSET, BOS, p(60), EOS], 1),
    "unused ids are times": ([t(0), ONSET, p(60), 350, OFFSET, p(60), ONSET, p(61), 399, OFFSET, p(61), EOS], 2),
    "pitch and mode before the first time": ([ONSET, p(60), t(4), ONSET, p(62), t(8), OFFSET, p(60), p(62), EOS], 1),
    "empty row": ([PAD] * 8, 0),
    "EOS only": ([EOS] * 8, 0),
}


def test_hand_written_rows_decode_as_on_the_host():
    assert all(8 <= len(tokens) <= 24 for tokens, _ in HAND_ROWS.values())
    ids = _pad_rows([tokens for tokens, _ in HAND_ROWS.values()])
    want = TOK.decode(ids, mode="batched")
    got = scoring.detokenize(TOK, ids.cuda()).to_numpy()
    for (name, (_, n_closed)), g, w in zip(HAND_ROWS.items(), got, want):
        assert len(w) == n_closed, name                       # the host shows the behaviour
        assert g.dtype == np.float64 and g.shape == w.shape and np.array_equal(g, w), (name, g, w)
    unused = want[list(HAND_ROWS).index("unused ids are times")]
    assert unused[:, 1].max() >= 200 * TOK.time_step


# ------------------------------------------------------------------------------------------------ 2. fuzz
R_FUZZ, L_FUZZ = 64, 72


def _random_notes(rng, n=12, span=3.0):
    dur = rng.uniform(0.05, 1.0, n)
    start = rng.uniform(0.0, span - dur)
    pitch = rng.integers(40, 80, n)
    notes = np.stack([start, start + dur, pitch, np.full(n, 80.0)], axis=1)
    return notes[np.argsort(notes[:, 0], kind="stable")]


@pytest.fixture(scope="module")
def fuzz_base():
    """64 label arrays of 12 notes in 3 s and their token rows [64, 72] (12 notes: at most 24 groups of three ids)."""
    rng = np.random.default_rng(7)
    labels = [_random_notes(rng) for _ in range(R_FUZZ)]
    rows = [TOK._tokenize(n).numpy()[:L_FUZZ] for n in labels]
    return labels, _pad_rows(rows, L_FUZZ)


def _corrupt(ids, rate, seed):
    rng = np.random.default_rng(seed)
    repl = rng.integers(0, 400, ids.shape)
    repl[repl == EOS] = ONSET
    mask = rng.random(ids.shape) < rate
    return torch.from_numpy(np.where(mask, repl, ids.numpy()))


def test_fuzz_corrupted_rows(fuzz_base):
    from oracle import chroma
    labels, clean = fuzz_base
    ids = _corrupt(clean, 0.1, 7)
    decoded = TOK.decode(ids, mode="batched")
    host = _host_score(labels, decoded)
    mean_notes = float(np.mean([len(d) for d in decoded]))
    print(f"fuzz at 0.1: {mean_notes:.2f} decoded notes per row, host score {host:.4f}")
    assert mean_notes >= 4 and 0.1 < host < 0.9               # the set is not trivial
    assert _check_batched(TOK, ids, labels) == host
    assert evaluation.evaluate_tokens(TOK, ids.cuda(), labels) == pytest.approx(chroma.evaluate_batch(list(labels), list(decoded)), abs=1e-12)


@pytest.mark.parametrize("rate", [0.0, 0.25])
def test_fuzz_other_corruption_rates(fuzz_base, rate):
    labels, clean = fuzz_base
    _check_batched(TOK, _corrupt(clean, rate, 11), labels)


# ------------------------------------------------------------------------------------------------ 3. frame arithmetic
@pytest.mark.parametrize("ms", [10, 30, 50])
def test_frame_arithmetic_on_boundaries(ms):
    tok = _tokenizer(midi_quantize_ms=ms)
    rng = np.random.default_rng(ms)
    rows = [tok._tokenize(_random_notes(rng, 8, 199 * tok.time_step if ms == 10 else 3.0)).numpy() for _ in range(8)]
    ids = _pad_rows(rows)
    decoded = tok.decode(ids, mode="batched")
    longest = [float(d[:, 1].max()) for d in decoded]
    up, down = (lambda x: np.nextafter(x, np.inf)), (lambda x: np.nextafter(x, -np.inf))
    labels = [
        # ends exactly on, just under and just over a frame boundary; starts likewise
        np.array([[0.10, 0.50, 60, 80], [0.20, down(0.70), 64, 80], [0.30, up(0.90), 67, 80],
                  [down(1.00), 1.20, 70, 80], [up(1.10), 1.30, 72, 80], [1.25, 1.25, 99, 80]]),
        np.array([[0.00, longest[1] + 2.0, 50, 80]]),                       # the longest note is the label's
        np.array([[0.10, 0.20, 50, 80]]),                                   # the longest note is the output's
        np.array([[0.00, longest[3], 50, 80]]),                             # both end together
        np.array([[0.00, down(longest[4] + 1.0), 50, 80]]),                 # the label ends just under a frame boundary ...
        np.array([[0.00, up(longest[5] + 1.0), 50, 80]]),                   # ... and just over one
        np.array([[0.00, down(longest[6]), 50, 80]]),                       # a hair shorter than the output
        np.array([[0.00, up(longest[7]), 50, 80]]),                         # a hair longer
    ]
    _check_batched(tok, ids, labels)
    frames = scoring.chroma_counts(tok, ids.cuda(), labels).frames
    assert frames[1] == len(np.arange(0, longest[1] + 2.0, 1 / 100)) and frames[2] == len(np.arange(0, longest[2], 1 / 100))


# ------------------------------------------------------------------------------------------------ 4. edges
def test_one_row(fuzz_base):
    labels, clean = fuzz_base
    _check_batched(TOK, clean[:1], labels[:1])


def test_capacity_at_the_longest_row():
    """L = 2048: a row that opens a note with nearly every id and closes them all, and one that alternates onset and offset groups."""
    n_open = 1900
    dense = [t(0), ONSET] + [p(i % 100) for i in range(n_open)] + [t(1), OFFSET] + [p(i) for i in range(100)] + [EOS]
    alternating = []
    for k in range(2047 // 6):                                 # an onset group and an offset group per note: six ids each
        alternating += [t(2 * k % 200), ONSET, p(k % 128), t(2 * k % 200 + 1), OFFSET, p(k % 128)]
    half = []
    for k in range(2048 // 4):                                 # time, ONSET, pitch, pitch: two notes per four ids = L / 2 notes ...
        half += [t(k % 150), ONSET, p(k % 64), p(64 + k % 64)]
    half = half[:2048 - 130] + [t(199), OFFSET] + [p(i) for i in range(128)]   # ... closed by the last group
    ids = _pad_rows([dense, alternating, half], 2048)
    want = TOK.decode(ids, mode="batched")
    assert len(want[0]) == n_open and len(want[1]) == 2047 // 6 and len(want[2]) >= 2048 // 2 - 100
    got = scoring.detokenize(TOK, ids.cuda()).to_numpy()
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    labels = [np.array([[0.0, 0.04, 40, 80]]), np.array([[0.0, 9.0, 60, 80]]), np.array([[1.0, 8.0, 3, 80]])]
    _check_batched(TOK, ids, labels)


def test_strided_view_of_a_wider_tensor(fuzz_base):
    labels, clean = fuzz_base
    wide = torch.full((16, 100), 7, dtype=torch.long)
    wide[:, 10:10 + L_FUZZ] = clean[:16]
    view = wide.cuda()[:, 10:10 + L_FUZZ]
    assert view.stride() == (100, 1) and not view.is_contiguous()
    want = TOK.decode(clean[:16], mode="batched")
    got = scoring.detokenize(TOK, view).to_numpy()
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert evaluation.evaluate_tokens(TOK, view, labels[:16]) == _host_score(labels[:16], want)
    # a view whose inner stride is not 1 is copied first
    spread = torch.zeros((16, 2 * L_FUZZ), dtype=torch.long)
    spread[:, ::2] = clean[:16]
    got = scoring.detokenize(TOK, spread.cuda()[:, ::2]).to_numpy()
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_empty_outputs_and_empty_labels(fuzz_base):
    labels, clean = fuzz_base
    nothing = torch.zeros((4, 16), dtype=torch.long)
    assert _check_batched(TOK, nothing, labels[:4]) == 0.0     # nothing decoded: voiced frames, none correct
    empty = [np.zeros((0, 4))] * 4
    assert _check_batched(TOK, clean[:4], empty) == 0.0        # no label: no voiced frame
    assert _check_batched(TOK, nothing, empty) == 0.0          # neither: no frame at all
    assert np.array_equal(scoring.chroma_counts(TOK, nothing.cuda(), empty).frames, np.zeros(4, dtype=np.int64))
    mixed = [labels[0], np.zeros((0, 4)), np.array([[0.5, 0.5, 60, 80]]), labels[3]]
    _check_batched(TOK, torch.cat([clean[:2], nothing[:2, :1].expand(2, L_FUZZ)]), mixed)
    assert scoring.detokenize(TOK, torch.zeros((3, 0), dtype=torch.long).cuda()).to_numpy()[2].shape == (0, 4)
    assert scoring.detokenize(TOK, torch.zeros((0, 5), dtype=torch.long).cuda()).to_numpy() == []


@pytest.mark.parametrize("bad_id", [400, -1, 1 << 40])
def test_an_id_outside_the_vocabulary(fuzz_base, bad_id):
    labels, clean = fuzz_base
    ids = clean[:6].clone()
    ids[2, 30] = bad_id
    dn = scoring.detokenize(TOK, ids.cuda())
    with pytest.raises(ValueError, match="token row 2 holds an id outside"):
        dn.to_numpy()
    with pytest.raises(ValueError, match="token row 2 holds an id outside"):
        scoring.chroma_counts(TOK, ids.cuda(), labels[:6])
    counts, notes = dn.counts.cpu().numpy(), dn.notes.cpu().numpy()
    assert counts[2] == -1
    for r in (0, 1, 3, 4, 5):                                  # the other rows of that call are unharmed
        raw = TOK._decode_tokens(clean[r].numpy(), 0)
        raw = raw[raw[:, 1] != -1]
        assert counts[r] == len(raw) and np.array_equal(notes[r, :counts[r]], raw[:, :3].astype(np.int32))
    _check_batched(TOK, clean[:6], labels[:6])                 # and so is a second, valid call


# ------------------------------------------------------------------------------------------------ 5. sequential
def test_sequential_rows_of_one_recording(fuzz_base):
    labels, clean = fuzz_base
    rows = [TOK._tokenize(n).numpy() for n in labels[:5]]
    rows[2] = np.concatenate([rows[2][:-1], [t(59), ONSET, p(90), EOS]])       # a note left open at the end of row 2 ...
    rows[3] = np.concatenate([[t(1), OFFSET, p(90)], rows[3]])                 # ... that row 3 would close if the state leaked
    ids = _corrupt(_pad_rows(rows), 0.05, 5)
    ids[2, :len(rows[2])] = torch.from_numpy(rows[2])
    ids[3, :3] = torch.from_numpy(rows[3][:3])
    want = TOK.decode(ids, mode="sequential", duration_per_batch=3)
    assert want.ndim == 2 and not (want[:, 2] == 90).any() and want[:, 1].max() > 12.0
    dn = scoring.detokenize(TOK, ids.cuda(), mode="sequential", duration_per_batch=3)
    got = dn.to_numpy()
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == want.shape and np.array_equal(got, want)
    label = np.concatenate([n + [3.0 * i, 3.0 * i, 0, 0] for i, n in enumerate(labels[:5])])
    assert label[:, 1].max() > 12.0
    host = evaluation.evaluate_batch([numpy_to_midi(label)], [numpy_to_midi(want)])
    counts = scoring.chroma_counts(TOK, ids.cuda(), label, mode="sequential", duration_per_batch=3)
    assert (int(counts.correct[0]), int(counts.voiced[0]), int(counts.frames[0])) == _host_counts(label, want)
    assert len(counts.frames) == 1 and counts.score == host and 0.0 < host < 1.0
    assert evaluation.evaluate_tokens(TOK, ids.cuda(), label, mode="sequential", duration_per_batch=3) == host
    # a label that outlasts the output, and none at all
    for other in (np.concatenate([label, [[0.0, 21.0, 30, 80]]]), np.zeros((0, 4))):
        assert evaluation.evaluate_tokens(TOK, ids.cuda(), other, mode="sequential", duration_per_batch=3) == \
            evaluation.evaluate_batch([numpy_to_midi(other)], [numpy_to_midi(want)])


# ------------------------------------------------------------------------------------------------ 6. callers
def test_score_batch_validation_step_and_score_recording():
    from music2midi_amd.checkpoint import load_t5_state
    from music2midi_amd.model import Music2MIDI
    geom = T5Geometry(DEFAULT_CONFIG["model"]["t5"])
    sd = synth.t5_state_dict(geom, seed=0)
    synth.perturb_layer_norms(sd, 0)
    synth.force_eos_head(sd, geom, active=340, eos_scale=1.6)
    m = Music2MIDI(copy.deepcopy(DEFAULT_CONFIG))
    load_t5_state(m.model, sd, strict=False)
    m = m.cuda().eval()
    notes = (np.array([[0.10, 0.40, 60, 80], [0.50, 1.00, 64, 80], [1.20, 1.90, 67, 80], [2.00, 2.60, 72, 80]]),
             np.array([[0.05, 0.30, 50, 80], [0.70, 1.10, 55, 80]]),
             np.array([[0.00, 2.90, 40, 80], [0.30, 0.80, 76, 80], [1.00, 1.40, 77, 80], [1.50, 1.70, 79, 80], [2.00, 2.20, 81, 80],
                       [2.40, 2.80, 83, 80]]))
    B = len(notes)
    wav = torch.from_numpy(synth.waveform_batch(40, B, 48000))
    idx = torch.from_numpy(synth.cond_index_batch(40, B))
    inputs = ModelInputs(input_waveform=wav.cuda(), notes_batch=notes, cond_index=idx.cuda())
    want = m.evaluate_batch(inputs)[0]
    got = m.score_batch(inputs)
    assert isinstance(got, float) and got == want
    m.validation_step(inputs, 0)
    assert m.logged["val/score"] == want
    # a whole recording: 7 s are three segments, scored against one label array
    audio = synth.waveform(33, 7 * 16000)
    label = np.concatenate([n + [3.0 * i, 3.0 * i, 0, 0] for i, n in enumerate(notes)])[:-2]
    host = evaluation.evaluate_batch([numpy_to_midi(label)], [m.generate(audio_y=audio, cond_index=[4, 2])])
    assert m.score_recording(label, audio_y=audio, cond_index=[4, 2]) == host
