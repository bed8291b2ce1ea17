"""Beam search under the token grammar and the logits processors, without a GPU: the restatement (tests/beam_process_ref.py) against
beam_ref and a brute-force enumeration, the language property, the keyword surface, the config switch, the export and its blocks."""
import ctypes as C
import copy
import inspect
import itertools
import math
from pathlib import Path

import pytest
import torch

from music2midi_amd import native
from music2midi_amd.config import DEFAULT_CONFIG, inference_beams, load_config
from music2midi_amd.generation import ProcessConfig, resolve_beam_process_kwargs
from music2midi_amd.grammar import EOS, MidiGrammar

import beam_process_cases as bc
import beam_process_ref as bpr
import beam_ref
from test_beam_gpu import FP32_CASES as PLAIN_CASES

GR = MidiGrammar(5, 128, 200)
NEG = -float("inf")


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("case", [PLAIN_CASES[0], PLAIN_CASES[1]], ids=lambda c: "-".join(map(str, c)))
def test_neutral_hook_is_beam_ref(case):
    name, eos, B, S, nb, n, lp, es, L, seed = case
    assert name == "tiny"
    orc, g = bc.oracle(bc.tiny_config(), "fp32", eos=eos)
    x = bc.embeds(B, S, g.d_model, seed=seed)
    want = beam_ref.oracle_beam_search(orc, x, nb, L, lp, es, n)
    got = bpr.oracle_beam_search(orc, x, nb, L, lp, es, n)                      # pc = None, grammar = None
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2] == want[2]
    got = bpr.oracle_beam_search(orc, x, nb, L, lp, es, n, pc=ProcessConfig())    # the neutral block
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2] == want[2]


@pytest.fixture(scope="module")
def grammar_run():
    name, eos, B, S, nb, n, lp, es, L, seed, gram, kw = bc.FP32_CASES[1]
    assert gram and not kw
    orc, g = bc.oracle(bc.tiny_config(), "fp32", eos=eos)
    x = bc.embeds(B, S, g.d_model, seed=seed)
    return orc, x, bpr.oracle_beam_search(orc, x, nb, L, lp, es, n, grammar=GR), (nb, L, lp, es, n)


def test_grammar_rows_of_finite_score_walk_inside_the_language(grammar_run):
    orc, x, (ids, scores, gap), (nb, L, lp, es, n) = grammar_run
    finite = [r for r, s in zip(ids.tolist(), scores.tolist()) if math.isfinite(s)]
    assert finite
    for row in finite:
        assert bc.walks_inside(GR, row), row
        assert GR.accepts(row)
    plain = beam_ref.oracle_beam_search(orc, x, nb, L, lp, es, n)[0]
    assert not all(bc.walks_inside(GR, r) for r in plain.tolist())             # the unconstrained beams are not MIDI


# V = 8, nb = 2, three steps of logits that depend on the step alone; ids 0 pad, 2 EOS.  The model never prefers EOS.
_TABLE = [[0.0, 1.5, -3.0, 2.0, 0.5, -1.0, 0.2, -0.4],
          [0.3, -0.2, -2.5, 0.1, 1.7, 0.9, -1.1, 0.6],
          [1.1, 0.4, -4.0, -0.3, 0.2, 2.2, 0.8, -0.9]]


def _table_step(tokens, t, beam_idx):
    return torch.tensor(_TABLE[t], dtype=torch.float32).expand(tokens.shape[0], -1).clone()


def test_forced_eos_fills_the_beams_from_candidates_at_minus_inf():
    """max_length = 4, forced_eos_token_id at cur_len 3 (the last step): brute force over every path of the table.  With
    length_penalty = 0 a score is the sum of the path's log-probabilities, the forced EOS counting 0."""
    V, nb, L, eos = 8, 2, 4, 2
    pc = ProcessConfig(forced_eos_token_id=eos)
    ids, scores, _ = bpr.beam_search(_table_step, 1, nb, V, L, 0.0, False, 2, eos=eos, pad=0, start=0, pc=pc)
    lp = [torch.log_softmax(torch.tensor(r, dtype=torch.float32), -1) for r in _TABLE]
    # the two best two-token paths that hold no EOS (exact beam search finds them: the logits do not depend on the prefix, so the
    # best pairs extend the best first tokens), each then forced to EOS at step 2
    paths = sorted(((float(lp[0][a] + lp[1][b]), [0, a, b]) for a, b in itertools.product(range(V), repeat=2) if eos not in (a, b)),
                   key=lambda p: -p[0])[:2]
    # the hypotheses: the two forced EOS (added at the last step) are the only finite ones; the running beams of the last step
    # come from candidates at -inf - the lowest flat indices that are not EOS: beam 0's ids 0 and 1 - and finalize offers them at
    # -inf, which does not beat the two kept hypotheses
    assert ids.tolist() == [p[1] + [eos] for p in paths]
    assert torch.allclose(scores, torch.tensor([p[0] for p in paths]), rtol=0, atol=1e-6)
    # with n = nb and a hypothesis store that is not yet full the -inf beams themselves come back: one forced EOS only, nb = 2
    pc1 = ProcessConfig(forced_eos_token_id=eos, suppress_tokens=tuple(range(3, V)))        # ids 0, 1 (and EOS) stay
    ids1, scores1, _ = bpr.beam_search(_table_step, 1, nb, V, L, 0.0, False, 2, eos=eos, pad=0, start=0, pc=pc1)
    want = sorted(((float(lp[0][a] + lp[1][b]), [0, a, b, eos]) for a, b in itertools.product((0, 1), repeat=2)), key=lambda p: -p[0])[:2]
    assert ids1.tolist() == [w[1] for w in want]
    assert torch.allclose(scores1, torch.tensor([w[0] for w in want]), rtol=0, atol=1e-6)


def test_beams_at_minus_inf_are_returned_as_such():
    """from the second step on the hook bans every id: all candidates are at -inf and rank by the flat index alone - beam 0's ids 0
    and 1 become the beams (its EOS, id 2, has rank 2 >= nb and is dropped), finalize adds both running beams at -inf and returns
    the later-added first.  Nothing is NaN, the gap bookkeeping skips the -inf pairs."""
    V, nb, L, eos = 8, 2, 4, 2

    def hook(ids_rows, logp):
        return logp if ids_rows.shape[1] == 1 else torch.full_like(logp, NEG)

    ids, scores, gap = bpr.beam_search(_table_step, 1, nb, V, L, 1.0, False, 2, eos=eos, pad=0, start=0, hook=hook)
    assert ids.tolist() == [[0, 3, 0, 1], [0, 3, 0, 0]]             # step 0: ids 3 and 1; both later beams descend from beam 0
    assert scores.tolist() == [NEG, NEG]
    assert gap == gap and 0 < gap < math.inf                         # the finite gaps of step 0


# ---------------------------------------------------------------------------------------------- keywords
@pytest.mark.parametrize("kw", [dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2), dict(bad_words_ids=[[5], [7, 9]]),
                                dict(min_length=4, repetition_penalty=0.5)])
def test_history_processors_raise_not_implemented(kw):
    with pytest.raises(NotImplementedError, match="history"):
        resolve_beam_process_kwargs(kw, 400, GR)


def test_resolve_beam_process_kwargs():
    assert resolve_beam_process_kwargs({}, 400, GR) == (None, False)
    assert resolve_beam_process_kwargs({"midi_grammar": True}, 400, GR) == (None, True)
    pc, gram = resolve_beam_process_kwargs(dict(bc.ALL_KW, midi_grammar=True), 400, GR)
    assert gram is True and pc.min_length == 12 and pc.forced_eos_token_id == EOS and pc.bad_words_ids == ((66,),)
    assert pc.forced_bos_token_id == 3 and pc.begin_index == 2 and pc.repetition_penalty == 1.0 and pc.no_repeat_ngram_size == 0
    kw = {"repetition_penalty": 1.0, "no_repeat_ngram_size": 0, "min_length": 3}                # neutral values are absent processors
    assert resolve_beam_process_kwargs(kw, 400, GR)[0] == ProcessConfig(min_length=3)
    assert kw == {"repetition_penalty": 1.0, "no_repeat_ngram_size": 0, "min_length": 3}       # not modified
    with pytest.raises(ValueError, match="bool"):
        resolve_beam_process_kwargs({"midi_grammar": 1}, 400, GR)
    with pytest.raises(ValueError, match="vocabulary"):
        resolve_beam_process_kwargs({"suppress_tokens": [400]}, 400, GR)
    with pytest.raises(ValueError, match="4096"):
        resolve_beam_process_kwargs({"min_length": 3}, 4097, None)
    with pytest.raises(ValueError, match="pitch"):
        resolve_beam_process_kwargs({"midi_grammar": True}, 400, MidiGrammar(5, 129, 200))
    with pytest.raises(ValueError, match="vocab_size"):
        resolve_beam_process_kwargs({"midi_grammar": True}, 332, GR)
    with pytest.raises(ValueError, match="2048"):
        resolve_beam_process_kwargs({"midi_grammar": True}, 400, GR, max_length=2049)
    resolve_beam_process_kwargs({"midi_grammar": True}, 400, GR, max_length=2048)
    with pytest.raises(NotImplementedError, match="do_sample"):
        resolve_beam_process_kwargs({"do_sample": True}, 400, GR)


def test_entry_points_and_the_unchanged_ones():
    from music2midi_amd.transformer import T5Transformer
    for name in ("beam_search_processed", "beam_search_processed_from_embeds"):
        p = inspect.signature(getattr(T5Transformer, name)).parameters
        assert list(p)[2:9] == ["num_beams", "max_length", "length_penalty", "early_stopping", "num_return_sequences", "return_scores",
                                "midi_grammar"]
        assert p["midi_grammar"].default is False and p["max_length"].default == 20
        assert any(q.kind is inspect.Parameter.VAR_KEYWORD for q in p.values())
    p = inspect.signature(T5Transformer.beam_search).parameters
    assert "midi_grammar" not in p and not any(q.kind is inspect.Parameter.VAR_KEYWORD for q in p.values())


def test_config_switch():
    assert inference_beams(load_config(DEFAULT_CONFIG)) == {}
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["inference"]["num_beams"] = 1
    assert inference_beams(load_config(cfg)) == {}
    cfg["inference"]["num_beams"] = 4
    assert inference_beams(load_config(cfg)) == {"num_beams": 4, "length_penalty": 1.0, "early_stopping": False}
    cfg["inference"].update(length_penalty=2, early_stopping="never")
    assert inference_beams(load_config(cfg)) == {"num_beams": 4, "length_penalty": 2.0, "early_stopping": "never"}
    for bad in (0, -2, 2.5, True):
        cfg["inference"]["num_beams"] = bad
        with pytest.raises(ValueError, match="num_beams"):
            inference_beams(load_config(cfg))


def test_music2midi_routes_beams_through_the_processed_entry_point():
    from music2midi_amd.model import Music2MIDI, _decode_entry
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    m = Music2MIDI(cfg)
    fn, kw = _decode_entry(m.model, m.config, m._grammar_kwargs())
    assert fn == m.model.generate and kw == {}
    cfg["inference"].update(num_beams=2, midi_grammar=True, batch_size=7)
    m = Music2MIDI(cfg)
    fn, kw = _decode_entry(m.model, m.config, m._grammar_kwargs())
    assert fn == m.model.beam_search_processed
    assert kw == {"num_beams": 2, "length_penalty": 1.0, "early_stopping": False, "num_return_sequences": 1, "midi_grammar": True}


# ---------------------------------------------------------------------------------------------- the ABI
def test_the_export_and_its_parameter_blocks():
    assert "m2m_generate_beam_processed" in native.EXPORTED_SYMBOLS
    res, args = native._SIGNATURES["m2m_generate_beam_processed"]
    assert res is C.c_int
    assert args == [C.c_void_p, C.c_int, C.POINTER(native.BeamParams), C.POINTER(native.GrammarParams), C.POINTER(native.ProcessParams),
                    C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]
    header = (Path(__file__).resolve().parents[1] / "include" / "music2midi_amd.h").read_text()
    assert ("int m2m_generate_beam_processed(m2m_session* s, int max_length, const m2m_beam_params* p, const m2m_grammar_params* grammar,"
            in header)
    assert "no logits processors apply" not in header

    def offsets(struct):
        return [(n, getattr(struct, n).offset) for n, _ in struct._fields_]

    assert C.sizeof(native.BeamParams) == 16
    assert offsets(native.BeamParams) == [("num_beams", 0), ("length_penalty", 4), ("early_stopping", 8), ("num_return_sequences", 12)]
    assert C.sizeof(native.GrammarParams) == 12
    assert offsets(native.GrammarParams) == [("pitch_offset", 0), ("n_pitch", 4), ("n_time", 8)]
    assert C.sizeof(native.ProcessParams) == 80
    assert offsets(native.ProcessParams) == [
        ("repetition_penalty", 0), ("no_repeat_ngram_size", 4), ("min_length", 8), ("min_new_tokens", 12), ("forced_bos_token_id", 16),
        ("forced_eos_token_id", 20), ("suppress_tokens", 24), ("n_suppress_tokens", 32), ("begin_suppress_tokens", 40),
        ("n_begin_suppress_tokens", 48), ("bad_words_ids", 56), ("bad_words_lengths", 64), ("n_bad_words", 72)]
    if native.library_path().exists():
        assert hasattr(native.load(), "m2m_generate_beam_processed")


def test_evaluate_batch_chunks_a_beam_decode_by_batch_size():
    """inference.batch_size 4, num_beams 2: five labelled clips are decoded two at a time (4 rows a call), the ids padded to one width"""
    from types import SimpleNamespace

    import numpy as np

    from music2midi_amd.input import ModelInputs
    from music2midi_amd.model import Music2MIDI

    class Stop(Exception):
        pass

    calls, seen = [], {}

    def beam_search_processed(inputs, **kw):
        n = inputs.input_waveform.shape[0]
        calls.append((n, len(inputs.notes_batch), tuple(inputs.cond_index.shape), kw, torch.is_grad_enabled()))
        return torch.full((n, 3 + len(calls)), 7, dtype=torch.long)

    def decode(token_ids, mode):
        seen["ids"] = token_ids
        raise Stop

    model = SimpleNamespace(beam_search_processed=beam_search_processed, geometry=SimpleNamespace(pad_token_id=0),
                            tokenizer=SimpleNamespace(decode=decode))
    stub = SimpleNamespace(model=model, config=SimpleNamespace(inference={"num_beams": 2, "batch_size": 4, "midi_grammar": True}))
    stub._grammar_kwargs = lambda: Music2MIDI._grammar_kwargs(stub)
    inputs = ModelInputs(input_waveform=torch.zeros(5, 8), notes_batch=tuple(np.zeros((2, 4)) for _ in range(5)),
                         cond_index=torch.zeros(5, 2, dtype=torch.long))
    with torch.enable_grad(), pytest.raises(Stop):
        Music2MIDI.evaluate_batch(stub, inputs)
    assert [c[:3] for c in calls] == [(2, 2, (2, 2)), (2, 2, (2, 2)), (1, 1, (1, 2))]
    assert all(c[3] == dict(max_length=8, num_beams=2, length_penalty=1.0, early_stopping=False, num_return_sequences=1,
                            midi_grammar=True) and c[4] is False for c in calls)
    assert seen["ids"].shape == (5, 6) and bool((seen["ids"][:2, 4:] == 0).all()) and bool((seen["ids"][4] == 7).all())
