"""The MIDI token grammar (music2midi_amd/grammar.py) against the tokenizer that defines its language, its restatement as a logits
processor (tests/grammar_ref.py) against the installed transformers classes, and the keyword / ABI surface.  No GPU."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from music2midi_amd import native
from music2midi_amd.config import DEFAULT_CONFIG, load_config
from music2midi_amd.generation import GenerateConfig, ProcessConfig, resolve_generate_kwargs
from music2midi_amd.grammar import (EOS, OFFSET, OFFSET_LIST, ONSET, ONSET_LIST, ONSET_OPEN, START, TIME, GrammarState,
                                    MidiGrammar)
from music2midi_amd.tokenizer import MidiTokenizer

import grammar_ref as gref

TOK = MidiTokenizer(load_config(DEFAULT_CONFIG))
GR = TOK.grammar
STEP = TOK.time_step                    # 0.05 s
P0, T0 = GR.pitch_offset, GR.time_offset


def _notes(rng, n, n_steps, n_pitch=128, max_len=40):
    """n notes (onset_s, offset_s, pitch, velocity) on the time grid, at most one sounding note per pitch at any time: a pitch is
    struck again at the earliest at the step its last note ends (the decoder closes every earlier open note of a pitch at that
    pitch's first OFFSET, so two notes of one pitch sounding together are not in the language: see the module docstring of
    grammar.py and test_two_sounding_notes_of_one_pitch).  No duplicated (onset step, pitch) pair follows from that."""
    free_from = {}
    rows = []
    for _ in range(n):
        p = rng.randrange(n_pitch)
        lo = free_from.get(p, 0)
        if lo >= n_steps - 1:
            continue
        on = rng.randrange(lo, min(lo + 30, n_steps - 1))
        off = on + 1 + rng.randrange(max_len)
        free_from[p] = off
        rows.append((on * STEP, off * STEP, p, 80))
    rng.shuffle(rows)
    return np.asarray(rows, dtype=np.float64).reshape(-1, 4)


def test_the_tokenizer_writes_the_grammar():
    rng = random.Random(0)
    assert GR.accepts([1] + TOK._tokenize(np.zeros((0, 4))).tolist())            # the empty array: EOS alone
    n_groups = n_restrike = n_clipped = n_cut = 0
    for case in range(300):
        # every third case runs past the last time id (offsets are clipped to it), every fourth is cut off
        notes = _notes(rng, rng.randrange(1, 60), GR.n_time - 1 if case % 3 == 0 else 150, max_len=400 if case % 3 == 0 else 40)
        cutoff = 4 if case % 4 == 0 else None
        ids = TOK._tokenize(notes, cutoff).tolist()
        assert GR.accepts([1] + ids), (case, TOK.to_string(ids))
        assert ids[-1] == EOS
        n_groups += sum(1 for i in ids if i >= T0)
        n_clipped += int((notes[:, 1] / STEP > GR.n_time).any() and T0 + GR.n_time - 1 in ids)
        n_cut += int(cutoff is not None and (notes[:, 0] >= cutoff).any())
        # a pitch struck again in the group that ends its earlier note: ONSET p and OFFSET p after one time id
        for a, b in zip([i for i, t in enumerate(ids) if t >= T0], [i for i, t in enumerate(ids) if t >= T0][1:] + [len(ids)]):
            grp = ids[a:b]
            if OFFSET in grp and ONSET in grp:
                n_restrike += bool(set(grp[grp.index(ONSET) + 1: grp.index(OFFSET)]) & set(grp[grp.index(OFFSET) + 1:]))
    assert n_groups > 3000 and n_restrike > 20 and n_clipped > 20 and n_cut > 20


def test_restrikes_of_one_pitch():
    """a pitch struck again while its earlier note still sounds up to that very step (the overlap the open_old / open_new split is
    for): legato re-strikes, a chain of them, and two pitches crossing"""
    for notes in ([(0.0, 0.5, 60, 80), (0.5, 1.0, 60, 80)],
                  [(0.0, 0.5, 60, 80), (0.5, 1.0, 60, 80), (1.0, 1.5, 60, 80), (1.5, 2.0, 60, 80)],
                  [(0.0, 0.5, 60, 80), (0.5, 1.0, 60, 80), (0.25, 0.5, 61, 80), (0.5, 0.75, 61, 80)],
                  [(0.0, 0.5, 60, 80), (0.0, 12.0, 61, 80), (0.5, 11.0, 60, 80)]):
        arr = np.asarray(notes, dtype=np.float64)
        ids = TOK._tokenize(arr).tolist()
        assert GR.accepts([1] + ids), TOK.to_string(ids)
        back = TOK.decode([np.asarray(ids)])[0]
        assert len(back) == len(arr)


def test_two_sounding_notes_of_one_pitch():
    """Two notes of one pitch that sound at the same time are ONE sounding pitch to ``_decode_tokens``: its first OFFSET closes
    both, and the second OFFSET the tokenizer writes is discarded.  The grammar bans what the decoder discards, so it stops at that
    second OFFSET (the pitch is silent there): this input is outside the language, by the same rule as 'OFFSET of a silent pitch'."""
    arr = np.asarray([(0.0, 0.5, 60, 80), (0.25, 0.75, 60, 80)], dtype=np.float64)
    ids = TOK._tokenize(arr).tolist()
    assert TOK.to_string(ids) == ["time_0", "ONSET", "note_60", "time_5", "ONSET", "note_60", "time_10", "OFFSET", "note_60",
                                  "time_15", "OFFSET", "note_60", "EOS"]
    back = TOK.decode([np.asarray(ids)])[0]
    assert back[:, 1].tolist() == [0.5, 0.5]               # both closed by the first OFFSET: the second changed nothing
    assert GR.accepts([1] + ids[:10]) and not GR.accepts([1] + ids[:11])
    assert OFFSET not in GR.allowed(GR.state_of([1] + ids[:10]))


def _pick(gr, rng, state):
    """one id out of ``allowed(state)`` (never empty, ascending, inside the tokenizer's vocabulary): mostly list entries and short
    time jumps, so a sequence lasts, now and then EOS"""
    allowed = gr.allowed(state)
    assert allowed, state
    assert allowed == sorted(set(allowed))
    assert all(i in (EOS, ONSET, OFFSET) or gr.pitch_offset <= i < gr.end for i in allowed)
    times = [i for i in allowed if i >= gr.time_offset]
    rest = [i for i in allowed if i < gr.time_offset and i != EOS]
    if EOS in allowed and rng.random() < 0.01:
        return EOS
    if rest and (not times or rng.random() < 0.7):
        return rng.choice(rest)
    if times:
        return times[min(len(times) - 1, rng.randrange(3))]
    return EOS


def _walk(gr, rng, steps):
    """``steps`` picks; EOS ends a sequence and the next one starts.  -> the sequences (start token first, the last one open)"""
    seqs, state, ids = [], gr.start(), [1]
    for _ in range(steps):
        tok = _pick(gr, rng, state)
        ids.append(tok)
        state = gr.step(state, tok)
        if tok == EOS:
            seqs.append(ids)
            state, ids = gr.start(), [1]
    assert gr.state_of(ids) == state
    return seqs + [ids]


@pytest.mark.parametrize("sizes", [(5, 128, 200), (5, 100, 1900), (7, 128, 3900), (5, 3, 2)])
def test_allowed_is_never_empty_and_walks_decode(sizes):
    gr = MidiGrammar(*sizes)
    cfg = load_config(DEFAULT_CONFIG)
    cfg.tokenizer.vocab_size = dict(special=sizes[0], pitch=sizes[1], time=sizes[2])
    tok = MidiTokenizer(cfg)
    assert (tok.grammar.pitch_offset, tok.grammar.time_offset, tok.grammar.end) == (gr.pitch_offset, gr.time_offset, gr.end)
    total_on = total_off = 0
    for seed in range(4):
        for ids in _walk(gr, random.Random(seed), 2000):
            assert gr.accepts(ids)
            # every ONSET pitch becomes a note or a still-open onset: the decoder drops none of them
            raw = tok._decode_tokens(np.asarray(ids), 0)
            n_onsets = n_offsets = 0
            mode = None
            for t in ids[1:]:
                mode = t if t in (ONSET, OFFSET) else (None if t >= gr.time_offset else mode)
                n_onsets += int(gr.pitch_offset <= t < gr.time_offset and mode == ONSET)
                n_offsets += int(gr.pitch_offset <= t < gr.time_offset and mode == OFFSET)
            assert len(raw) == n_onsets
            # ... and every OFFSET pitch closed at least one note (a pitch struck again while it sounds is closed together with
            # its earlier note): the distinct (offset step, pitch) pairs of the closed notes are the OFFSET pitches
            closed = raw[raw[:, 1] != -1]
            assert len({(int(r[1]), int(r[2])) for r in closed}) == n_offsets
            assert len(tok.decode([np.asarray(ids)])[0]) == len(closed)
            total_on += n_onsets
            total_off += n_offsets
    assert total_on > 500 and total_off > 500


def test_hand_written_rejects():
    t = lambda i: T0 + i        # noqa: E731
    p = lambda i: P0 + i        # noqa: E731
    ok = [1, t(0), ONSET, p(60), p(64), t(4), ONSET, p(60), OFFSET, p(60), p(64), t(9), OFFSET, p(60), EOS]
    assert GR.accepts(ok)
    assert TOK.decode([np.asarray(ok)])[0].shape == (3, 4)
    bad = {
        "time not increasing": [1, t(3), ONSET, p(60), t(3), OFFSET, p(60), EOS],
        "time going back": [1, t(3), ONSET, p(60), t(2), OFFSET, p(60), EOS],
        "pitch after time": [1, t(0), p(60), EOS],
        "pitch at the start": [1, p(60), EOS],
        "OFFSET of a silent pitch": [1, t(0), ONSET, p(60), t(2), OFFSET, p(61), EOS],
        "OFFSET with nothing sounding": [1, t(0), OFFSET, p(60), EOS],
        "OFFSET of a pitch struck in the same group": [1, t(0), ONSET, p(60), t(1), ONSET, p(61), OFFSET, p(61), EOS],
        "ONSET after OFFSET in a group": [1, t(0), ONSET, p(60), t(2), OFFSET, p(60), ONSET, p(62), EOS],
        "the same pitch twice in an ONSET list": [1, t(0), ONSET, p(60), p(60), EOS],
        "an empty group": [1, t(0), t(1), ONSET, p(60), EOS],
        "EOS after a mode token": [1, t(0), ONSET, EOS],
        "id 333": [1, t(0), ONSET, p(60), 333, EOS],
        "id 399": [1, 399],
        "PAD before EOS": [1, t(0), ONSET, p(60), 0, EOS],
        "BOS again": [1, 1, EOS],
    }
    for name, ids in bad.items():
        assert not GR.accepts(ids), name
    assert GR.accepts([1, EOS, 333, 7]) and GR.accepts([1, t(0), ONSET, p(1), EOS, 0, 0])     # nothing after EOS is looked at
    assert GR.accepts([1, t(0), ONSET, p(1)])                                                   # a prefix (max_length cut it)


def test_transitions_are_total():
    rng = random.Random(3)
    state = GR.start()
    assert state == GrammarState(START, -1, frozenset(), frozenset())
    for _ in range(3000):                                   # any id at all, allowed or not: the state stays a state
        state = GR.step(state, rng.randrange(400))
        assert 0 <= state.phase <= OFFSET_LIST and -1 <= state.last_time < GR.n_time
        assert all(0 <= q < GR.n_pitch for q in state.open_old | state.open_new)
    s = GR.state_of([1, T0 + 5, ONSET, P0 + 9])
    assert s == GrammarState(ONSET_LIST, 5, frozenset(), frozenset({9}))
    assert GR.step(s, T0 + 7) == GrammarState(TIME, 7, frozenset({9}), frozenset())
    for inert in (0, 1, EOS, 333, 399):
        assert GR.step(s, inert) == s
    assert GR.step(GR.start(), P0 + 3) == GR.start() and GR.step(GrammarState(TIME, 2), P0 + 3) == GrammarState(TIME, 2)
    assert GR.step(s, ONSET).phase == ONSET_OPEN
    with pytest.raises(ValueError):
        MidiGrammar(4, 128, 200)
    with pytest.raises(ValueError):
        MidiGrammar(5, 0, 200)


# ------------------------------------------------------------------ the processor, against transformers
@pytest.fixture(scope="module")
def lp():
    return pytest.importorskip("transformers.generation.logits_process")


def _prefixes(rng, B, cur):
    """B grammatical prefixes of cur ids (walks, padded by walking on)"""
    rows = []
    while len(rows) < B:
        ids = _walk(GR, rng, cur - 1)[0]
        if len(ids) == cur and EOS not in ids:
            rows.append(ids)
    return torch.tensor(rows)


def test_grammar_ref_matches_hf_prefix_constrained_processor(lp):
    V, L = 400, 24
    rng = random.Random(5)
    fn = GR.prefix_allowed_tokens_fn()
    for cur in (1, 2, 3, 4, 9, 17, 23):
        ids = _prefixes(rng, 6, cur)
        s = torch.randn(6, V, generator=torch.Generator().manual_seed(cur)) * 3
        # the grammar alone
        want = lp.PrefixConstrainedLogitsProcessor(fn, 1)(ids, s.clone())
        got = gref.process(ids, s, None, EOS, L, GR)
        assert torch.equal(got, want), cur
        assert torch.equal(torch.isfinite(got), gref.grammar_mask(ids, V, GR) == 0)
        assert torch.equal(got[torch.isfinite(got)], s[torch.isfinite(got)])
        # 4.34's chain: min length, min new tokens, THE GRAMMAR, forced BOS (an id the grammar bans at cur = 1: the forced id wins)
        for forced in (333, P0 + 3, T0 + 1):
            pc = ProcessConfig(min_length=20, min_new_tokens=18, forced_bos_token_id=forced, suppress_tokens=(T0 + 2,))
            want = s.clone()
            for proc in (lp.MinLengthLogitsProcessor(20, EOS), lp.MinNewTokensLengthLogitsProcessor(1, 18, EOS),
                         lp.PrefixConstrainedLogitsProcessor(fn, 1), lp.ForcedBOSTokenLogitsProcessor(forced),
                         lp.SuppressTokensLogitsProcessor([T0 + 2])):
                want = proc(ids, want)
            got = gref.process(ids, s, pc, EOS, L, GR)
            assert torch.equal(got, want), (cur, forced)
            if cur == 1:
                assert forced not in GR.allowed(GR.start()) or forced >= T0
                assert got.argmax(-1).eq(forced).all() and bool((got[:, forced] == 0).all())
            elif cur < 19:
                assert not torch.isfinite(got[:, EOS]).any()                  # the two EOS bans hold under the grammar
    # without a grammar it is process_ref.process
    pc = ProcessConfig(repetition_penalty=1.3, min_length=5)
    assert torch.equal(gref.process(ids, s, pc, EOS, L, None), gref.pr.process(ids, s, pc, EOS, L))


def test_a_forced_id_outside_the_grammar_leaves_a_defined_state():
    """forced BOS = 333 (never allowed): the id is emitted, the state does not move, and the next step is masked from START"""
    s1 = GR.state_of([1, 333])
    assert s1 == GR.start()
    assert GR.allowed(s1)[0] == EOS and GR.allowed(s1)[1] == T0
    s2 = GR.state_of([1, ONSET])                            # forced ONSET at the start: ONSET_OPEN with every pitch allowed
    assert s2.phase == ONSET_OPEN and len(GR.allowed(s2)) == GR.n_pitch


# ------------------------------------------------------------------ keywords and the ABI
def test_keyword_resolution():
    assert resolve_generate_kwargs({}).midi_grammar is False and GenerateConfig().midi_grammar is False
    cfg = resolve_generate_kwargs({"midi_grammar": True, "max_length": 64}, vocab_size=400, grammar=GR)
    assert cfg.midi_grammar is True and cfg.process is None and not cfg.do_sample       # a field of GenerateConfig, not a processor
    assert resolve_generate_kwargs({"midi_grammar": False}, vocab_size=400) == resolve_generate_kwargs({}, vocab_size=400)
    cfg = resolve_generate_kwargs(dict(midi_grammar=True, do_sample=True, temperature=1.5, top_k=0, min_length=9,
                                       return_dict_in_generate=True, output_scores=True, output_logprobs=True), vocab_size=400, grammar=GR)
    assert cfg.midi_grammar and cfg.do_sample and cfg.process == ProcessConfig(min_length=9) and cfg.output_scores and cfg.output_logprobs
    assert not hasattr(ProcessConfig(), "midi_grammar")
    for bad in (1, 0, None, "yes", [True]):
        with pytest.raises(ValueError, match="midi_grammar"):
            resolve_generate_kwargs({"midi_grammar": bad})
    with pytest.raises(ValueError, match="max_length"):
        resolve_generate_kwargs({"midi_grammar": True, "max_length": 2049}, vocab_size=400, grammar=GR)
    resolve_generate_kwargs({"midi_grammar": True, "max_length": 2048}, vocab_size=400, grammar=GR)
    with pytest.raises(ValueError, match="max_length"):
        resolve_generate_kwargs({"midi_grammar": True, "max_new_tokens": 2048}, vocab_size=400, grammar=GR)
    with pytest.raises(ValueError, match="pitch"):
        resolve_generate_kwargs({"midi_grammar": True}, vocab_size=400, grammar=MidiGrammar(5, 129, 200))
    with pytest.raises(ValueError, match="vocab_size"):
        resolve_generate_kwargs({"midi_grammar": True}, vocab_size=332, grammar=GR)          # special + pitch + time = 333 > V
    resolve_generate_kwargs({"midi_grammar": True}, vocab_size=333, grammar=GR)
    with pytest.raises(ValueError, match="4096"):
        resolve_generate_kwargs({"midi_grammar": True}, vocab_size=4097, grammar=MidiGrammar(5, 128, 3900))
    resolve_generate_kwargs({"midi_grammar": True}, vocab_size=4096, grammar=MidiGrammar(7, 128, 3900))
    with pytest.raises(NotImplementedError):
        resolve_generate_kwargs({"midi_grammar": True, "num_beams": 2}, vocab_size=400, grammar=GR)
    # the limits are the grammar's own, whoever asks
    GR.check_device_limits(400)
    with pytest.raises(ValueError):
        MidiGrammar(5, 129, 10).check_device_limits(400)


def test_beam_search_does_not_take_the_keyword():
    import inspect
    from music2midi_amd.transformer import T5Transformer
    assert "midi_grammar" not in inspect.signature(T5Transformer.beam_search).parameters
    assert "midi_grammar" not in inspect.signature(T5Transformer.beam_search_from_embeds).parameters


def test_the_export_and_its_parameter_block():
    assert "m2m_generate_grammar" in native.EXPORTED_SYMBOLS
    res, args = native._SIGNATURES["m2m_generate_grammar"]
    assert res is C.c_int
    assert args == [C.c_void_p, C.c_int, C.POINTER(native.GrammarParams), C.POINTER(native.ProcessParams),
                    C.POINTER(native.SampleParams), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]
    assert C.sizeof(native.GrammarParams) == 12
    assert [f[0] for f in native.GrammarParams._fields_] == ["pitch_offset", "n_pitch", "n_time"]
    # m2m_generate_scored's arguments with the grammar block in front of the processors
    assert args[:2] + args[3:] == native._SIGNATURES["m2m_generate_scored"][1]


def test_the_model_config_key_reaches_generate():
    from music2midi_amd.model import Music2MIDI
    seen = []

    class Stub:
        config = load_config(DEFAULT_CONFIG)
        _grammar_kwargs = Music2MIDI._grammar_kwargs

    assert Stub()._grammar_kwargs() == {}                   # absent by default: generate is called as before
    Stub.config.inference["midi_grammar"] = True
    assert Stub()._grammar_kwargs() == {"midi_grammar": True}
    Stub.config.inference["midi_grammar"] = False
    assert Stub()._grammar_kwargs() == {}

    from music2midi_amd import distributed as D
    from music2midi_amd.input import ModelInputs

    def fake(inputs, **kw):
        seen.append(kw)
        return torch.zeros((1, 3), dtype=torch.long)
    inp = ModelInputs(input_waveform=torch.zeros(1, 8), cond_index=None)
    D.generate_sharded(fake, inp, max_length=3, midi_grammar=True)
    D.generate_sharded(fake, inp, max_length=3)
    assert seen == [{"max_length": 3, "midi_grammar": True}, {"max_length": 3}]


def test_evaluate_batch_still_decodes_without_autograd():
    """``evaluate_batch`` runs under ``torch.no_grad()`` as it did before the config key (training_step and validation_step call it
    with autograd on, and ``encoder_inputs`` reads a trainable embedding); the helper that builds the keyword carries no decorator."""
    from types import SimpleNamespace

    from music2midi_amd.model import Music2MIDI

    class Stop(Exception):
        pass

    seen = {}

    def generate(inputs, **kw):
        seen.update(grad=torch.is_grad_enabled(), kw=kw)
        raise Stop

    for key, want in (({}, {}), ({"midi_grammar": True}, {"midi_grammar": True})):
        stub = SimpleNamespace(model=SimpleNamespace(generate=generate), config=SimpleNamespace(inference=key))
        stub._grammar_kwargs = lambda stub=stub: Music2MIDI._grammar_kwargs(stub)
        with torch.enable_grad(), pytest.raises(Stop):
            Music2MIDI.evaluate_batch(stub, SimpleNamespace(notes_batch=[np.zeros((3, 4)), np.zeros((5, 4))]))
        assert seen["grad"] is False and seen["kw"] == dict(max_length=20, **want)
    assert not hasattr(Music2MIDI._grammar_kwargs, "__wrapped__")
