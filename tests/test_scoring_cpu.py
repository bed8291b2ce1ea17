"""CPU: what the on-device scoring (music2midi_amd.scoring, csrc/score.hip) decides without a device - the refusals of the two
entry points, the header against the binding, the eligibility rule of the labels, the host fallbacks of ``score_batch`` and the
frame-count formula the kernel evaluates against ``len(np.arange(...))``."""
import copy
import ctypes as C
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from music2midi_amd import evaluation, native, scoring
from music2midi_amd.config import DEFAULT_CONFIG, load_config
from music2midi_amd.input import ModelInputs
from music2midi_amd.tokenizer import MidiTokenizer
from music2midi_amd.utils import numpy_to_midi

ROOT = Path(__file__).resolve().parents[1]
FAKE = 0x100000                          # a device address that is never dereferenced: every refusal comes first


def _tokenizer(**tok):
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["tokenizer"].update(tok)
    return MidiTokenizer(load_config(cfg))


# ------------------------------------------------------------------------------------------------ header and binding
def test_header_declares_what_the_binding_binds():
    header = (ROOT / "include" / "music2midi_amd.h").read_text()
    for name, proto in [
            ("m2m_score_frame_count", "int64_t m2m_score_frame_count(double end_seconds);"),
            ("m2m_score_detokenize", "int m2m_score_detokenize(const int64_t* ids_dev, int R, int L, int64_t row_stride, int64_t steps_per_row, "
                                     "int pitch_offset,"),
            ("m2m_score_chroma_counts", "int m2m_score_chroma_counts(const int32_t* notes_dev, const int32_t* counts_dev, int R, int L, "
                                        "int sequential, double time_step,")]:
        assert proto in header, name
        assert name in native.EXPORTED_SYMBOLS and hasattr(native.load(), name)
    assert "#define M2M_ABI_VERSION 1" in header and native.load().m2m_abi_version() == 1
    assert len(native._SIGNATURES["m2m_score_detokenize"][1]) == 11
    assert len(native._SIGNATURES["m2m_score_chroma_counts"][1]) == 13
    assert native._SIGNATURES["m2m_score_chroma_counts"][1][5] is C.c_double
    assert native._SIGNATURES["m2m_score_frame_count"] == (C.c_int64, [C.c_double])
    for macro, value in [("M2M_SCORE_MAX_TOKENS 2048", scoring.MAX_TOKENS), ("M2M_SCORE_MAX_FRAMES (1 << 22)", scoring.MAX_FRAMES)]:
        assert f"#define {macro}" in header and value == eval(macro.split(" ", 1)[1])
    assert scoring.MAX_FRAMES >= 3600 * scoring.FS           # at least an hour of audio per timeline


# ------------------------------------------------------------------------------------------------ refusals without a device
def _detok(R=4, L=72, stride=None, steps=0, po=5, to=133, V=400, ids=FAKE, notes=FAKE, counts=FAKE):
    lib = native.load()
    st = lib.m2m_score_detokenize(ids, R, L, L if stride is None else stride, steps, po, to, V, notes, counts, None)
    return st, lib.m2m_last_error().decode()


@pytest.mark.parametrize("kw,msg", [
    (dict(R=0), "0 rows out of range"),
    (dict(R=65536), "65536 rows out of range"),
    (dict(L=0), "L=0 out of range"),
    (dict(L=2049), "L=2049 out of range"),
    (dict(L=72, stride=71), "row stride 71 below L=72"),
    (dict(V=0), "vocab_size 0 out of range"),
    (dict(V=4097), "vocab_size 4097 out of range"),
    (dict(po=4), "pitch_offset 4 below"),
    (dict(po=5, to=5), "0 pitch ids out of range"),
    (dict(po=5, to=134), "129 pitch ids out of range"),
    (dict(to=133, V=132), "time_offset 133 beyond vocab_size 132"),
    (dict(steps=-1), "steps_per_row -1 out of range"),
    (dict(R=65535, steps=40000), "does not fit in int32"),
    (dict(R=65535, L=2048, stride=40000), "does not fit in int32 elements"),
    (dict(ids=None), "null ids"),
    (dict(notes=None), "null ids"),
    (dict(counts=None), "null ids"),
])
def test_detokenize_refuses_on_the_arguments_alone(kw, msg):
    st, err = _detok(**kw)
    assert st == -1 and msg in err, err


def _counts(R=4, L=72, seq=0, ts=0.05, labels=FAKE, offsets=FAKE, n_labels=10, T=None, cap=2000, notes=FAKE, counts=FAKE, out=FAKE):
    lib = native.load()
    T = (1 if seq else R) if T is None else T
    st = lib.m2m_score_chroma_counts(notes, counts, R, L, seq, ts, labels, offsets, n_labels, T, cap, out, None)
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
    (dict(ts=-0.05), "time_step -0.05 out of range"),
    (dict(ts=float("nan")), "time_step nan out of range"),
    (dict(ts=float("inf")), "time_step inf out of range"),
    (dict(n_labels=-1), "-1 label notes out of range"),
    (dict(n_labels=(1 << 24) + 1), "label notes out of range"),
    (dict(cap=0), "frame_cap 0 out of range"),
    (dict(cap=(1 << 22) + 1), "frame_cap 4194305 out of range"),
    (dict(notes=None), "null notes"),
    (dict(counts=None), "null notes"),
    (dict(offsets=None), "null notes"),
    (dict(out=None), "null notes"),
    (dict(labels=None, n_labels=3), "null labels"),
])
def test_chroma_counts_refuses_on_the_arguments_alone(kw, msg):
    st, err = _counts(**kw)
    assert st == -1 and msg in err, err


def test_python_layer_refuses_before_the_library():
    tok = _tokenizer()
    ids = torch.zeros((2, 8), dtype=torch.long)
    with pytest.raises(ValueError, match="CUDA int64"):
        scoring.detokenize(tok, ids)
    with pytest.raises(ValueError, match="CUDA int64"):
        scoring.chroma_counts(tok, ids, [np.zeros((0, 4))] * 2)
    with pytest.raises(ValueError, match="Invalid argument mode=both"):
        scoring.detokenize(tok, ids, mode="both")
    with pytest.raises(ValueError, match="duration_per_batch is required"):
        scoring.detokenize(tok, ids, mode="sequential")
    for velocity in (0, -3):
        with pytest.raises(ValueError, match="default_velocity"):
            scoring.detokenize(_tokenizer(default_velocity=velocity), ids)
    assert tok.model_vocab_size == 400 and scoring._vocab_size(tok, None) == 400 and scoring._vocab_size(tok, 333) == 333
    assert scoring._vocab_size(SimpleNamespace(), None) == 4096
    assert scoring._steps_per_row(tok, "batched", None) == 0 and scoring._steps_per_row(tok, "sequential", 3) == 60


# ------------------------------------------------------------------------------------------------ eligibility
GOOD = [0.1, 0.5, 60, 80]


@pytest.mark.parametrize("rows,ok", [
    ([GOOD], True),
    ([], True),                                               # no notes at all
    ([[0.0, 0.5, 0, 1], [0.2, 0.9, 127, 127]], True),          # the corners of the rule
    ([[0.1, 0.5, 60.9, 80]], True),                            # int(pitch) = 60
    ([[0.1, 0.5, -0.5, 80]], True),                            # int(pitch) = 0
    ([[0.1, 0.5, 127.5, 80]], True),                           # int(pitch) = 127
    ([GOOD, [0.1, 0.5, 128, 80]], False),
    ([GOOD, [0.1, 0.5, -1, 80]], False),
    ([GOOD, [-0.01, 0.5, 60, 80]], False),                     # a negative start
    ([GOOD, [0.1, 0.5, 60, 0]], False),                        # velocity 0 sounds nowhere on the host
    ([GOOD, [0.1, 0.5, 60, -5]], False),
    ([GOOD, [0.1, 0.5, 60, 0.5]], False),                      # numpy_to_midi truncates it to 0
    ([GOOD, [0.1, np.inf, 60, 80]], False),
    ([GOOD, [0.1, 0.5, np.nan, 80]], False),
    ([GOOD, [0.1, 0.5, 60, np.nan]], False),
    ([GOOD, [0.1, 50000.0, 60, 80]], False),                   # beyond the frame cap (11.6 hours)
    ([GOOD, [0.1, 3600.0, 60, 80]], True),                     # an hour is within it
    # notes numpy_to_midi drops (end <= start, or a NaN in either) are not looked at
    ([GOOD, [0.5, 0.5, 300, -1]], True),
    ([GOOD, [0.7, 0.2, -4, 0]], True),
    ([GOOD, [-1.0, -2.0, 60, 80]], True),
    ([GOOD, [np.nan, 0.5, 999, 80]], True),
    ([GOOD, [0.1, np.nan, 999, 80]], True),
])
def test_eligibility_rule(rows, ok):
    notes = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
    assert scoring.labels_eligible([notes]) is ok
    assert scoring.labels_eligible([np.asarray([GOOD]), notes]) is ok
    if ok:
        packed, offsets, bound = scoring._pack_labels([notes])
        kept = notes[notes[:, 1] > notes[:, 0]]
        assert packed.shape == (3, len(kept)) and packed.dtype == np.float64 and offsets.tolist() == [0, len(kept)]
        assert np.array_equal(packed[:2], kept[:, :2].T) and np.array_equal(packed[2], np.trunc(kept[:, 2]))
        assert bound == (len(np.arange(0, kept[:, 1].max(), 1 / 100)) if len(kept) else 0)
    else:
        with pytest.raises(ValueError, match="not eligible"):
            scoring._pack_labels([notes])


def test_eligibility_of_other_shapes():
    assert not scoring.labels_eligible([np.zeros((2, 3))])
    assert not scoring.labels_eligible([np.zeros(4)])
    assert not scoring.labels_eligible([[["a", "b", "c", "d"]]])
    assert scoring.labels_eligible([[GOOD, GOOD]])             # a list of rows is an array
    assert scoring.labels_eligible([])


def test_pack_labels_lays_timelines_side_by_side():
    a = np.array([[0.1, 0.4, 60, 80], [0.5, 0.5, 61, 80], [0.6, 1.0, 62.7, 80]])
    b = np.zeros((0, 4))
    c = np.array([[0.0, 2.5, 40, 1]])
    packed, offsets, bound = scoring._pack_labels([a, b, c])
    assert offsets.dtype == np.int32 and offsets.tolist() == [0, 2, 2, 3]
    assert np.array_equal(packed, np.array([[0.1, 0.6, 0.0], [0.4, 1.0, 2.5], [60, 62, 40]]))
    assert packed.flags["C_CONTIGUOUS"] and bound == 250


# ------------------------------------------------------------------------------------------------ score_batch's fallbacks
def _stub(ids, calls):
    from music2midi_amd.model import Music2MIDI
    tok = _tokenizer()

    def generate(inputs, **kw):
        calls.append(kw)
        return ids
    stub = SimpleNamespace(model=SimpleNamespace(generate=generate, tokenizer=tok, geometry=SimpleNamespace(pad_token_id=0)),
                           config=SimpleNamespace(inference={}))
    stub._grammar_kwargs = lambda: Music2MIDI._grammar_kwargs(stub)
    return stub, tok


def test_score_batch_scores_cpu_ids_on_the_host(monkeypatch):
    """ids that are not on a GPU never reach the device path: one decode, the host pipeline, evaluate_batch's own float."""
    from music2midi_amd import model as model_mod
    from music2midi_amd.model import Music2MIDI
    labels = (np.array([[0.10, 0.40, 60, 80], [0.50, 1.00, 64, 80]]), np.array([[0.05, 0.30, 50, 80], [0.70, 1.10, 55, 80]]))
    shifted = (labels[0] + [0.05, 0.1, 12, 0], labels[1] + [0.0, 0.0, 5, 0])     # an octave up and late; a fourth up
    calls = []
    tok = _tokenizer()
    stub, tok = _stub(tok(shifted), calls)
    monkeypatch.setattr(model_mod, "evaluate_tokens", lambda *a, **k: pytest.fail("the device path was taken for host ids"))
    inputs = ModelInputs(input_waveform=torch.zeros(2, 8), notes_batch=labels, cond_index=None)
    got = Music2MIDI.score_batch(stub, inputs)
    want = Music2MIDI.evaluate_batch(stub, inputs)[0]
    assert isinstance(got, float) and got == want and 0.0 < got < 1.0
    assert got == evaluation.evaluate_batch([numpy_to_midi(n) for n in labels], [numpy_to_midi(n) for n in tok.decode(tok(shifted))])
    assert calls == [dict(max_length=8)] * 2                  # one decode per call, the budget of evaluate_batch


def test_score_batch_scores_ineligible_labels_on_the_host(monkeypatch):
    """Labels the device path does not take go to the host even for ids on a GPU (the stand-in below claims to be on one)."""
    from music2midi_amd import model as model_mod
    from music2midi_amd.model import Music2MIDI

    class OnGpu(torch.Tensor):
        is_cuda = True

    good = np.array([[0.10, 0.40, 60, 80], [0.50, 1.00, 64, 80]])
    bad = np.array([[0.10, 0.40, 60, 80], [0.50, 1.00, 64, 0.5]])               # a velocity numpy_to_midi truncates to 0
    tok = _tokenizer()
    other = np.array([[0.10, 0.40, 61, 80], [0.50, 1.00, 64, 80]])              # what the second clip "decodes" to: a semitone off
    ids = tok((good, other)).as_subclass(OnGpu)
    assert ids.is_cuda and model_mod._on_device_scorable(ids, (good, good)) and not model_mod._on_device_scorable(ids, (good, bad))
    assert not model_mod._on_device_scorable(tok((good, good)), (good, good))
    stub, tok = _stub(ids, [])
    taken = []
    monkeypatch.setattr(model_mod, "evaluate_tokens", lambda *a, **k: taken.append(a) or 0.25)
    inputs = ModelInputs(input_waveform=torch.zeros(2, 8), notes_batch=(good, bad), cond_index=None)
    got = Music2MIDI.score_batch(stub, inputs)
    assert not taken and got == Music2MIDI.evaluate_batch(stub, inputs)[0] and 0.0 < got < 1.0
    # the same ids with eligible labels do take the device path
    assert Music2MIDI.score_batch(stub, ModelInputs(input_waveform=torch.zeros(2, 8), notes_batch=(good, good), cond_index=None)) == 0.25
    assert len(taken) == 1 and taken[0][1] is ids


def test_evaluate_tokens_is_exported_next_to_evaluate_batch():
    import music2midi.evaluation as drop_in
    assert drop_in.evaluate_tokens is evaluation.evaluate_tokens and drop_in.evaluate_batch is evaluation.evaluate_batch


# ------------------------------------------------------------------------------------------------ the frame-count formula
def _arange_len(x):
    return len(np.arange(0, x, 1 / 100))


def test_frame_count_formula_equals_arange_length_on_random_doubles():
    """n_frames = len(np.arange(0, x, 1 / 100)) on the host; the kernel computes ceil(x / (1.0 / 100.0)) in double."""
    rng = np.random.default_rng(3)
    xs = np.concatenate([rng.uniform(0.0, 30.0, 3000), rng.uniform(0.0, 4000.0, 1000), np.arange(0, 400) / 100.0,
                         np.nextafter(np.arange(1, 400) / 100.0, 0), np.nextafter(np.arange(1, 400) / 100.0, 1e9), [0.0, 1e-300, 41943.04]])
    lib = native.load()
    for x in xs.tolist():
        want = _arange_len(x)
        assert int(np.ceil(x / (1 / 100))) == want, x
        assert lib.m2m_score_frame_count(x) == want, x        # the library's own arithmetic, compiled for the host
    assert lib.m2m_score_frame_count(-1.0) == 0 and lib.m2m_score_frame_count(float("nan")) == 0


@pytest.mark.parametrize("ms", [50, 10, 30])
def test_frame_count_formula_on_every_time_the_vocabulary_can_produce(ms):
    tok = _tokenizer(midi_quantize_ms=ms)
    lib = native.load()
    top = 4096 + 60 * 64                                      # every index of a 4096-id vocabulary, and of 64 sequential rows
    off = 0
    for idx in range(top):
        x = idx * tok.time_step
        want = _arange_len(x)
        assert int(np.ceil(x / (1 / 100))) == want and lib.m2m_score_frame_count(x) == want, idx
        off += want != (ms // 10) * idx
    if ms == 50:
        assert off > 0                                        # the products are not exact: 5 * idx is NOT the formula
