"""CPU: what the on-device tokeniser (music2midi_amd.tokenize, csrc/tokenize.hip) decides without a device - the header against the
binding, the quantisation the kernel evaluates against ``MidiTokenizer._quantize``, the row bound against the host tokeniser's
rows, the eligibility rule of the notes, the refusals of the entry point and the host path of ``_labels`` with the key absent."""
import copy
import ctypes as C
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from music2midi_amd import native, tokenize
from music2midi_amd.config import DEFAULT_CONFIG, load_config
from music2midi_amd.tokenizer import MidiTokenizer

ROOT = Path(__file__).resolve().parents[1]
FAKE = 0x100000                          # a device address that is never dereferenced: every refusal comes first


def _tokenizer(ms=50, n_time=200, **vocab):
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["tokenizer"]["midi_quantize_ms"] = ms
    cfg["tokenizer"]["vocab_size"].update(time=n_time, **vocab)
    return MidiTokenizer(load_config(cfg))


# ------------------------------------------------------------------------------------------------ header and binding
def test_header_declares_what_the_binding_binds():
    header = (ROOT / "include" / "music2midi_amd.h").read_text()
    for name, proto in [
            ("m2m_tokenize_quantize", "int m2m_tokenize_quantize(double seconds, double time_step, int n_time);"),
            ("m2m_tokenize_row_bound", "int64_t m2m_tokenize_row_bound(int n_notes, int n_time);"),
            ("m2m_tokenize_notes", "int m2m_tokenize_notes(const double* notes_dev, const int32_t* offsets_dev, int n_notes, int B, "
                                   "double time_step, int pitch_offset,")]:
        assert proto in header, name
        assert name in native.EXPORTED_SYMBOLS and hasattr(native.load(), name)
    assert "#define M2M_ABI_VERSION 1" in header and native.load().m2m_abi_version() == 1
    args = native._SIGNATURES["m2m_tokenize_notes"][1]
    assert len(args) == 18 and args[4] is C.c_double and args[9] is C.c_double and args[10] is C.c_int64 and args[12] is C.c_int64
    assert native._SIGNATURES["m2m_tokenize_quantize"] == (C.c_int, [C.c_double, C.c_double, C.c_int])
    assert native._SIGNATURES["m2m_tokenize_row_bound"] == (C.c_int64, [C.c_int, C.c_int])
    for macro, value in [("M2M_TOKENIZE_MAX_NOTES 1024", tokenize.MAX_NOTES), ("M2M_TOKENIZE_MAX_TIME 4096", tokenize.MAX_TIME),
                         ("M2M_TOKENIZE_MAX_ROWS 65535", tokenize.MAX_ROWS)]:
        assert f"#define {macro}" in header and value == int(macro.split(" ", 1)[1])


# ------------------------------------------------------------------------------------------------ the quantisation
def _both(tok, xs):
    lib = native.load()
    n_time = tok.config.vocab_size.time
    got = np.array([lib.m2m_tokenize_quantize(float(x), tok.time_step, n_time) for x in xs])
    with np.errstate(over="ignore"):                          # 1.8e308 / step overflows to inf on purpose
        return got, tok._quantize(np.asarray(xs, dtype=np.float64))


def test_quantize_on_every_millisecond_of_ten_seconds_at_the_reference_step():
    tok = _tokenizer()
    xs = np.arange(10001) / 1000.0
    q = xs / tok.time_step
    assert int((q - np.floor(q) == 0.5).sum()) == 133         # the exact .5 quotients the nextafter is about
    got, want = _both(tok, xs)
    assert np.array_equal(got, want)
    assert got[25] == 1 and np.rint(q[25]) == 0               # ties go up: 0.025 s -> 1, where rint alone gives 0
    assert [tokenize.quantize(tok, x) for x in (0.0, 0.025, 9.95, 10.0)] == [0, 1, 199, 199]


@pytest.mark.parametrize("ms,n_time", [(10, 1000), (30, 200), (30, 4096), (50, 1)])
def test_quantize_at_steps_that_are_no_binary_fraction(ms, n_time):
    tok = _tokenizer(ms, n_time)
    xs = np.arange(10001) / 1000.0
    got, want = _both(tok, xs)
    assert np.array_equal(got, want)
    rng = np.random.default_rng(ms)
    got, want = _both(tok, rng.uniform(0.0, 1.2 * n_time * tok.time_step, 4000))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("ms,n_time", [(50, 200), (10, 1000), (30, 200)])
def test_quantize_at_the_ends_of_its_domain(ms, n_time):
    tok = _tokenizer(ms, n_time)
    top = (n_time - 1) * tok.time_step
    xs = [0.0, -0.0, 5e-324, top, np.nextafter(top, 0), np.nextafter(top, 1e9), n_time * tok.time_step, 1e6, 1e17, 1e300,
          1.7976931348623157e308, float("inf")]              # 1.8e308 / step overflows to inf: the minimum comes first
    got, want = _both(tok, xs)
    assert np.array_equal(got, want) and got[0] == 0 and got[3] == n_time - 1 and (got[6:] == n_time - 1).all()
    lib = native.load()
    for seconds, step, n in [(-1e-9, 0.05, 200), (float("nan"), 0.05, 200), (1.0, 0.0, 200), (1.0, -0.05, 200), (1.0, float("nan"), 200),
                             (1.0, 3600.5, 200), (1.0, 0.05, 0), (1.0, 0.05, 4097)]:
        assert lib.m2m_tokenize_quantize(seconds, step, n) == -1


# ------------------------------------------------------------------------------------------------ the row bound
def _random_clip(rng, n, duration=3.0, sort=False):
    on = rng.uniform(0.0, duration, n)
    notes = np.stack([on, on + rng.uniform(-0.05, 0.6, n), rng.integers(21, 109, n).astype(np.float64), np.full(n, 80.0)], axis=1)
    return notes[np.argsort(on)] if sort else notes


def test_row_bound_holds_on_random_clips_and_is_met_when_every_index_is_distinct():
    assert tokenize.row_bound(90, 200) == 541 and tokenize.row_bound(0, 200) == 1 and tokenize.row_bound(1024, 4096) == 6 * 1024 + 1
    assert tokenize.row_bound(1024, 200) == 1 + 2048 + 200 + 400
    assert native.load().m2m_tokenize_row_bound(-1, 200) == -1 and native.load().m2m_tokenize_row_bound(3, 0) == -1
    rng = np.random.default_rng(11)
    for ms, n_time in [(50, 200), (10, 1000), (50, 7)]:
        tok = _tokenizer(ms, n_time)
        for n in (1, 2, 5, 45, 90, 250, 600):
            for duration in (0.2, 3.0, 12.0):
                row = tok._tokenize(_random_clip(rng, n, duration))
                assert len(row) <= tokenize.row_bound(n, n_time), (ms, n_time, n, duration)
    # every onset and every offset on an index of its own: 6k + 1, and the bound's other arm when the indices run out
    tok = _tokenizer(50, 200)
    k = 90
    distinct = np.stack([np.arange(k) * 0.1, np.arange(k) * 0.1 + 0.05, np.full(k, 60.0), np.full(k, 80.0)], axis=1)
    assert len(tok._tokenize(distinct)) == 6 * k + 1 == tokenize.row_bound(k, 200)
    k = 300                                                   # all 200 indices taken: one short of 1 + 2k + T + 2T (no offset falls on index 0)
    dense = np.stack([(np.arange(k) % 200) * 0.05, ((np.arange(k) + 1) % 200) * 0.05, np.full(k, 60.0), np.full(k, 80.0)], axis=1)
    dense[dense[:, 1] < dense[:, 0], 1] = 9.95
    assert len(tok._tokenize(dense)) == tokenize.row_bound(k, 200) - 1 == 600 + 200 + 400


# ------------------------------------------------------------------------------------------------ eligibility
GOOD = [0.1, 0.5, 60, 80]


@pytest.mark.parametrize("rows,ok", [
    ([GOOD], True),
    ([], True),                                               # no notes at all
    ([[0.0, 0.0, -32768, 0], [0.2, 0.1, 32768, -5]], True),    # the corners of the rule; the velocity is not read
    ([[0.1, 0.5, 60.5, 80]], True),
    ([[0.1, -7.0, 60, 80]], True),                             # an offset before the onset is lifted to onset + step
    ([GOOD, [1e300, 1e300, 60, 80]], True),                    # finite: clips to the last index
    ([GOOD, [-1e-9, 0.5, 60, 80]], False),                     # a negative onset
    ([GOOD, [np.nan, 0.5, 60, 80]], False),
    ([GOOD, [0.1, np.inf, 60, 80]], False),
    ([GOOD, [0.1, 0.5, np.nan, 80]], False),
    ([GOOD, [0.1, 0.5, 60, np.inf]], False),                   # every value has to be finite
    ([GOOD, [0.1, 0.5, 32769, 80]], False),
    ([GOOD, [0.1, 0.5, -32768.5, 80]], False),
])
def test_eligibility_rule(rows, ok):
    tok = _tokenizer()
    notes = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
    assert tokenize.notes_eligible(tok, [notes]) is ok
    assert tokenize.notes_eligible(tok, [np.asarray([GOOD]), notes, np.zeros((0, 4))]) is ok
    if not ok:
        with pytest.raises(ValueError, match="not eligible"):
            tokenize.tokenize(tok, [notes])


def test_eligibility_of_other_shapes_sizes_and_vocabularies():
    tok = _tokenizer()
    assert not tokenize.notes_eligible(tok, [np.zeros((2, 3))])
    assert not tokenize.notes_eligible(tok, [np.zeros((2, 5))])
    assert not tokenize.notes_eligible(tok, [np.zeros(4)])
    assert not tokenize.notes_eligible(tok, [[["a", "b", "c", "d"]]])
    assert not tokenize.notes_eligible(tok, 5)
    assert tokenize.notes_eligible(tok, [[GOOD, GOOD]])        # a list of rows is an array
    assert tokenize.notes_eligible(tok, [])
    assert tokenize.notes_eligible(tok, [[], np.zeros((0, 4)), np.zeros(0), np.zeros((0, 3))])    # empty clips of any shape
    assert tokenize.notes_eligible(tok, [np.tile(GOOD, (1024, 1))])
    assert not tokenize.notes_eligible(tok, [np.asarray([GOOD]), np.tile(GOOD, (1025, 1))])
    assert tokenize.notes_eligible(_tokenizer(10, 4096), [[GOOD]]) and not tokenize.notes_eligible(_tokenizer(10, 4097), [[GOOD]])
    assert not tokenize.notes_eligible(_tokenizer(50, 0), [[GOOD]])
    assert not tokenize.notes_eligible(_tokenizer(special=4), [[GOOD]])
    assert not tokenize.notes_eligible(_tokenizer(0), [[GOOD]]) and not tokenize.notes_eligible(_tokenizer(3600001), [[GOOD]])
    assert not tokenize.notes_eligible(SimpleNamespace(), [[GOOD]])


def test_pack_lays_the_clips_side_by_side_with_their_offsets_behind():
    a = np.array([[0.1, 0.4, 60, 80], [0.5, 0.5, 61, 80], [0.6, 1.0, 62.7, 80]])
    c = np.array([[0.0, 2.5, 40, 1]])
    flat, per_clip = tokenize._flat_notes([a, [], c])
    assert per_clip.tolist() == [3, 0, 1]
    buf = tokenize._pack(flat, per_clip)
    assert buf.dtype == np.float64 and buf.flags["C_CONTIGUOUS"] and len(buf) == 12 + 2
    assert np.array_equal(buf[:12].reshape(3, 4), np.array([[0.1, 0.5, 0.6, 0.0], [0.4, 0.5, 1.0, 2.5], [60, 61, 62.7, 40]]))
    assert buf[12:].view(np.int32).tolist() == [0, 3, 3, 4]
    flat, per_clip = tokenize._flat_notes([[], []])
    assert tokenize._pack(flat, per_clip).view(np.int32).tolist()[:3] == [0, 0, 0]


# ------------------------------------------------------------------------------------------------ refusals without a device
def _call(notes=FAKE, offsets=FAKE, n=10, B=4, step=0.05, po=5, to=133, n_time=200, has_cutoff=0, cutoff=0.0, fill=0, labels=0, pad=0,
          ids=FAKE, width=64, stride=None, lengths=FAKE):
    lib = native.load()
    st = lib.m2m_tokenize_notes(notes, offsets, n, B, step, po, to, n_time, has_cutoff, cutoff, fill, labels, pad, ids, width,
                                width if stride is None else stride, lengths, None)
    return st, lib.m2m_last_error().decode()


@pytest.mark.parametrize("kw,msg", [
    (dict(B=0), "0 clips out of range"),
    (dict(B=65536), "65536 clips out of range"),
    (dict(n=-1), "-1 notes out of range"),
    (dict(n=4 * 1024 + 1), "4097 notes out of range"),
    (dict(step=0.0), "time_step 0 out of range"),
    (dict(step=-0.05), "time_step -0.05 out of range"),
    (dict(step=3600.5), "time_step 3600.5 out of range"),
    (dict(step=float("nan")), "time_step nan out of range"),
    (dict(step=float("inf")), "time_step inf out of range"),
    (dict(n_time=0), "0 time ids out of range"),
    (dict(n_time=4097), "4097 time ids out of range"),
    (dict(po=4), "pitch_offset 4 below"),
    (dict(po=5, to=4), "time_offset 4 out of range"),
    (dict(to=(1 << 30) + 1), "time_offset 1073741825 out of range"),
    (dict(has_cutoff=2), "has_cutoff must be 0 or 1"),
    (dict(labels=-1), "labels must be 0 or 1"),
    (dict(width=0), "width 0 below 1"),
    (dict(width=64, stride=63), "row stride 63 below width 64"),
    (dict(notes=None), "null notes"),
    (dict(offsets=None), "null notes"),
    (dict(ids=None), "null notes"),
    (dict(lengths=None), "null notes"),
])
def test_tokenize_notes_refuses_on_the_arguments_alone(kw, msg):
    st, err = _call(**kw)
    assert st == -1 and msg in err, err


def test_python_layer_refuses_before_the_library():
    tok = _tokenizer()
    with pytest.raises(ValueError, match="not eligible.*clip 1: 1025 notes"):
        tokenize.tokenize(tok, [[GOOD], np.tile(GOOD, (1025, 1))])
    with pytest.raises(ValueError, match="bucket=0"):
        tokenize.tokenize(tok, [[GOOD]], bucket=0)
    with pytest.raises(ValueError, match="width=0"):
        tokenize.tokenize(tok, [[GOOD]], width=0)
    if not torch.cuda.is_available():
        with pytest.raises(native.NativeError, match="no HIP device"):       # no fallback in the module
            tokenize.tokenize(tok, [[GOOD]])
    with pytest.raises(ValueError, match="cannot be placed"):
        tokenize._raise_for_rows(np.array([5, -1, 7]), 8)
    with pytest.raises(ValueError, match="clip 2 gives 9 ids, more than width=8"):
        tokenize._raise_for_rows(np.array([5, 8, 9]), 8)
    tokenize._raise_for_rows(np.array([1, 8]), 8)
    # the caller's helper hands the batch back to the host instead of raising
    cpu = torch.device("cpu")
    assert tokenize.training_labels(tok, [[GOOD]], cpu, 0, 16, None) is None


# ------------------------------------------------------------------------------------------------ _labels with the key absent
def _labels_stub(config, device_labels):
    from music2midi_amd.model import Music2MIDI
    tok = _tokenizer()
    t5 = SimpleNamespace(tokenizer=tok, geometry=SimpleNamespace(pad_token_id=0), device_labels=device_labels)
    return SimpleNamespace(model=t5, config=load_config(config), LABEL_BUCKET=Music2MIDI.LABEL_BUCKET), tok, Music2MIDI


def test_labels_with_the_key_absent_is_the_host_tensor():
    rng = np.random.default_rng(5)
    batch = (_random_clip(rng, 7), np.zeros((0, 4)), _random_clip(rng, 31))
    asked = []
    for config in (DEFAULT_CONFIG, {"trainer": {"device_labels": False}}, {}):
        stub, tok, Music2MIDI = _labels_stub(config, lambda *a, **k: asked.append(a) or pytest.fail("the device path was asked"))
        got = Music2MIDI._labels(stub, batch)
        want = tok(batch)
        want[want == 0] = -100
        assert not got.is_cuda and got.dtype == torch.int64 and got.shape[1] % 16 == 0 and got.shape[1] - want.shape[1] < 16
        assert torch.equal(got[:, :want.shape[1]], want) and (got[:, want.shape[1]:] == -100).all()
    assert not asked and "device_labels" not in DEFAULT_CONFIG["trainer"]


def test_labels_with_the_key_set_asks_the_device_path_and_keeps_the_host_path_behind_it():
    batch = (np.asarray([GOOD]),)
    asked = []
    marker = torch.zeros((1, 16), dtype=torch.int64)
    stub, tok, Music2MIDI = _labels_stub({"trainer": {"device_labels": True}}, lambda notes, **k: asked.append(k) or marker)
    assert Music2MIDI._labels(stub, batch) is marker and asked == [dict(bucket=16, enabled=True)]
    # a batch the device path does not take (None) is tokenised on the host as before
    stub, tok, Music2MIDI = _labels_stub({"trainer": {"device_labels": True}}, lambda notes, **k: None)
    got = Music2MIDI._labels(stub, batch)
    assert got.shape == (1, 16) and got[0, :7].tolist() == [135, 3, 65, 143, 4, 65, 2] and (got[0, 7:] == -100).all()


def test_transformer_helper_is_off_without_the_key_or_a_gpu():
    from music2midi_amd.transformer import T5Transformer
    t5 = T5Transformer(copy.deepcopy(DEFAULT_CONFIG))
    assert t5.device_labels([np.asarray([GOOD])]) is None                       # key absent
    t5.config.trainer.device_labels = True
    assert t5.transformer.device.type == "cpu" and t5.device_labels([np.asarray([GOOD])]) is None and t5._label_stream is None
