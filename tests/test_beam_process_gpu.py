"""Beam search under the token grammar and the logits processors on the GPU (T5Transformer.beam_search_processed /
m2m_generate_beam_processed) against the restatement (tests/beam_process_ref.py: beam_ref's transformers 4.34 beam search with the
processors applied to the log-softmax before the beam scores are added).  fp32 ids must be equal and the scores agree to
test_beam_gpu's derived bar; rows at -inf must be -inf exactly.  The cases and their seeds are in tests/beam_process_cases.py."""
import copy
import ctypes as C
import math

import pytest
import torch

from music2midi_amd import native, synth
from music2midi_amd.config import DEFAULT_CONFIG

import beam_process_cases as bc
import beam_process_ref as bpr
from test_beam_gpu import _assert_ids_equal, _hyp_len
from test_t5_gpu import build, embeds, tiny_config

pytestmark = pytest.mark.gpu
M2M_ERR_INVALID = -1
NEG = -float("inf")


def _beam(model, x, nb, L, lp=1.0, es=False, n=1, gram=False, **kw):
    ids, scores = model.beam_search_processed_from_embeds(x.cuda(), nb, max_length=L, length_penalty=lp, early_stopping=es,
                                                          num_return_sequences=n, return_scores=True, midi_grammar=gram, **kw)
    return ids.cpu(), scores.cpu()


def _check_against_the_restatement(tag, got, want, lp, eos):
    (ids, scores), (want_ids, want_scores, gap) = got, want
    inf = torch.isinf(want_scores)
    fin = ~inf
    # test_beam_gpu's bar: the sums are held to 5e-5 relative plus 5e-7 per term (one fp32 log-softmax term per step; see there)
    lens = torch.tensor([_hyp_len(r, eos) for r in want_ids], dtype=torch.float64)
    d_sum = ((scores.double() - want_scores.double()).abs() * lens ** lp)[fin]
    bar = (5e-5 * (want_scores.double().abs() * lens ** lp) + 5e-7 * lens)[fin]
    worst = float((d_sum / bar).max()) if fin.any() else 0.0
    print(f"beam processed fp32 {tag}: ids {tuple(ids.shape)} min decision gap {gap:.3e} | -inf rows {int(inf.sum())} of {len(inf)} | "
          f"sum err / bar max {worst:.2f}")
    assert gap > 1e-4, "a near-tie in the restatement: choose another seed"
    _assert_ids_equal(ids, want_ids, eos)
    assert torch.equal(torch.isinf(scores), inf) and bool((scores[inf] == NEG).all())
    assert not torch.isnan(scores).any()
    assert torch.all(d_sum <= bar)


@pytest.mark.parametrize("case", bc.FP32_CASES, ids=lambda c: c[0])
def test_fp32_equals_the_restatement(case):
    name, eos, B, S, nb, n, lp, es, L, seed, gram, kw = case
    model, orc, g = build(tiny_config(), "fp32", eos=eos)
    x = embeds(B, S, g.d_model, seed=seed)
    want = bpr.oracle_beam_search(orc, x, nb, L, lp, es, n, pc=bc.process_config(kw, g.vocab_size),
                                  grammar=model.tokenizer.grammar if gram else None)
    got = _beam(model, x, nb, L, lp, es, n, gram, **kw)
    _check_against_the_restatement(name, got, want, lp, g.eos_token_id)
    if name == "minus-inf":
        assert bool(torch.isinf(want[1]).any())
    if name == "grammar-all":      # the forced id wins over the grammar, and every row ends with the forced EOS at max_length - 1
        assert bool((got[0][:, 1] == kw["forced_bos_token_id"]).all()) and bool((got[0][:, L - 1] == g.eos_token_id).all())


@pytest.mark.parametrize("V,sizes,seed", bc.BAND_CASES, ids=lambda v: str(v))
def test_vocabulary_bands_fp32(V, sizes, seed):
    """NPL = 8, 32, 64 logits per lane (test_grammar_gpu.test_vocabulary_bands_fp32's shapes): the class boundaries fall inside a
    lane's ids and an unused tail exists"""
    cfg = bc.band_config(V, sizes)
    model, orc, g = build(cfg, "fp32")
    gr = model.tokenizer.grammar
    assert (gr.pitch_offset, gr.n_pitch, gr.n_time) == sizes and gr.end < V
    sh = bc.BAND_SHAPE
    x = embeds(sh["B"], sh["S"], g.d_model, seed=seed)
    want = bpr.oracle_beam_search(orc, x, sh["nb"], sh["L"], 1.0, False, sh["n"], grammar=gr)
    got = _beam(model, x, sh["nb"], sh["L"], n=sh["n"], gram=True)
    _check_against_the_restatement(f"V={V}", got, want, 1.0, g.eos_token_id)
    assert int(got[0].max()) < gr.end
    assert all(bc.walks_inside(gr, r) for r in got[0].tolist())


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_returned_rows_walk_inside_the_grammar(precision):
    B, S, nb, n, L = 3, 30, 4, 4, 40
    for eos in (False, True):
        model, _, g = build(tiny_config(), precision, eos=eos)
        gr = model.tokenizer.grammar
        x = embeds(B, S, g.d_model, seed=8)
        ids, scores = _beam(model, x, nb, L, n=n, gram=True)
        finite = [r for r, s in zip(ids.tolist(), scores.tolist()) if math.isfinite(s)]
        assert finite and all(bc.walks_inside(gr, r) for r in finite)
        plain = model.beam_search_from_embeds(x.cuda(), nb, max_length=L, num_return_sequences=n).cpu()
        assert not all(bc.walks_inside(gr, r) for r in plain.tolist())       # random-init beams mean nothing as MIDI


def test_bf16_tracks_the_bf16_restatement():
    """the pattern of test_beam_gpu.test_bf16_beam_tracks_the_bf16_restatement: equal ids, or a restatement gap below its 5e-2"""
    B, S, nb, n, L = 3, 30, 4, 2, 32
    model, orc, g = build(tiny_config(), "bf16", eos=True)
    x = embeds(B, S, g.d_model)
    want_ids, want_scores, gap = bpr.oracle_beam_search(orc, x, nb, L, 1.0, False, n, grammar=model.tokenizer.grammar)
    ids, scores = _beam(model, x, nb, L, n=n, gram=True)
    same = ids.shape == want_ids.shape and torch.equal(ids, want_ids)
    print(f"beam processed bf16: equal={same} min decision gap {gap:.3e} | scores {scores.tolist()} vs {want_scores.tolist()}")
    if same:
        assert torch.allclose(scores, want_scores, rtol=2e-2, atol=2e-2)
    else:
        assert gap < 5e-2


def _abi_call(model, x, L, bp, gp=None, pp=None, rows=None, session_rows=None):
    """m2m_generate_beam_processed on a fresh encode -> (status, the whole token buffer, the score buffer, out_len)"""
    lib = native.load()
    sess, _ = model._encode(x, L, rows=session_rows or x.shape[0] * bp.num_beams)
    rows = rows or x.shape[0] * bp.num_return_sequences
    tokens = torch.full((rows, L), -7, dtype=torch.long, device=x.device)
    scores = torch.full((rows,), 7.0, dtype=torch.float32, device=x.device)
    n = C.c_int(0)
    rc = lib.m2m_generate_beam_processed(sess, L, C.byref(bp), C.byref(gp) if gp is not None else None,
                                         C.byref(pp) if pp is not None else None, tokens.data_ptr(), scores.data_ptr(), C.byref(n),
                                         native.stream_handle(x.device))
    torch.cuda.synchronize()
    return rc, tokens.cpu(), scores.cpu(), n.value


def test_the_neutral_call_is_beam_search_bit_for_bit():
    B, S, nb, n, L = 3, 30, 4, 2, 32
    model, _, g = build(tiny_config(), "fp32", eos=True)
    x = embeds(B, S, g.d_model).cuda()
    want_ids, want_scores = model.beam_search_from_embeds(x, nb, max_length=L, num_return_sequences=n, return_scores=True)
    want_ids, want_scores = want_ids.cpu(), want_scores.cpu()
    ids, scores = _beam(model, x, nb, L, n=n)                                # no processor, midi_grammar=False: both blocks NULL
    assert torch.equal(ids, want_ids) and torch.equal(scores, want_scores)
    ids, scores = _beam(model, x, nb, L, n=n, repetition_penalty=1.0, min_length=0)     # neutral values: still no processor
    assert torch.equal(ids, want_ids) and torch.equal(scores, want_scores)
    bp = native.BeamParams(nb, 1.0, 0, n)
    rc, tok, sc, w = _abi_call(model, x, L, bp)                              # both pointers NULL
    assert rc == 0 and torch.equal(tok[:, :w], want_ids) and torch.equal(sc, want_scores)
    neutral = native.ProcessParams(1.0, 0, 0, 0, -1, -1, None, 0, None, 0, None, None, 0)
    rc, tok, sc, w = _abi_call(model, x, L, bp, pp=neutral)                  # the processed head over a neutral block, enable = 0
    assert rc == 0 and torch.equal(tok[:, :w], want_ids) and torch.equal(sc, want_scores)
    ids, scores = _beam(model, x, nb, L, n=n, gram=True)                     # and the grammar does change the beams
    assert not torch.equal(ids, want_ids)
    again = model.beam_search_from_embeds(x, nb, max_length=L, num_return_sequences=n).cpu()
    assert torch.equal(again, want_ids)                                      # the head mode does not outlive its call


def _beam_with_env(monkeypatch, cfg, precision, x, env, nb, L, **kw):
    for k, v in env.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    model, _, _ = build(cfg, precision, eos=True)        # M2M_DA_CLIPS is latched when the session is created: a model per leg
    out = _beam(model, x, nb, L, gram=True, **kw)
    for k in env:
        monkeypatch.delenv(k, raising=False)
    return out


@pytest.mark.parametrize("large", [False, True])
def test_kernel_forms_give_identical_beams_under_the_grammar(monkeypatch, large):
    """the shapes and the environment of test_beam_gpu.test_kernel_forms_give_identical_beams; two_chains splits the rows (and so
    the per-row grammar states) over two chains"""
    if large:
        cfg, precision, B, S, nb, L = DEFAULT_CONFIG, "bf16", 12, 864, 4, 16
    else:
        cfg, precision, B, S, nb, L = tiny_config(), "fp32", 6, 30, 4, 32
    from music2midi_amd.config import T5Geometry, load_config
    d = T5Geometry(load_config(cfg).model.t5).d_model
    x = embeds(B, S, d).cuda()
    legs = {
        "policy": {},
        "clips1": {"M2M_DA_CLIPS": "1"},
        "clips2": {"M2M_DA_CLIPS": "2"},
        "clips4": {"M2M_DA_CLIPS": "4"},
        "two_chains": {"M2M_GROUP_ROWS": str(B * nb // 2)},
        "no_graph": {"M2M_NO_GRAPH": "1"},
    }
    base = None
    for name, env in legs.items():
        env = {k: env.get(k) for k in ("M2M_DA_CLIPS", "M2M_GROUP_ROWS", "M2M_NO_GRAPH")}
        ids, scores = _beam_with_env(monkeypatch, cfg, precision, x, env, nb, L, n=2)
        print(f"beam processed forms {'large' if large else 'small'} {name}: ids {tuple(ids.shape)}")
        if base is None:
            base = (ids, scores)
        else:
            assert torch.equal(ids, base[0]), name
            assert torch.equal(scores, base[1]), name


def test_session_reuse_beam_grammar_greedy_grammar_beam_beam_grammar():
    """one session: beam + grammar, greedy + grammar, plain beam, beam + grammar - each equal to its fresh-session result (the state
    reset, and the region the per-clip and the per-row states share)"""
    B, S, nb, n, L = 3, 30, 4, 2, 40

    def run(model, what):
        x = embeds(B, S, model.geometry.d_model).cuda()
        if what == "beam+grammar":
            return _beam(model, x, nb, L, n=n, gram=True, min_length=6)
        if what == "greedy+grammar":
            return (model.generate_from_embeds(x, max_length=L, midi_grammar=True).cpu(),)
        ids, scores = model.beam_search_from_embeds(x, nb, max_length=L, num_return_sequences=n, return_scores=True)
        return ids.cpu(), scores.cpu()

    order = ["beam+grammar", "greedy+grammar", "beam", "beam+grammar"]
    fresh = {}
    for what in set(order):
        model, _, _ = build(tiny_config(), "fp32", eos=True)
        fresh[what] = run(model, what)
    model, _, _ = build(tiny_config(), "fp32", eos=True)
    _beam(model, embeds(B, S, model.geometry.d_model).cuda(), nb, L)          # the session is sized for B * nb rows from the start
    for what in order:
        got = run(model, what)
        assert len(got) == len(fresh[what]) and all(torch.equal(a, b) for a, b in zip(got, fresh[what])), what


def test_c_abi_invalid_blocks_launch_nothing():
    B, S, nb, L = 2, 19, 2, 16
    model, _, g = build(tiny_config(), "fp32")
    x = embeds(B, S, g.d_model).cuda()
    ok = _beam(model, x, nb, L, gram=True, min_length=4)                      # the session: max_batch = B * nb = 4
    lib = native.load()
    G, P, BP = native.GrammarParams, native.ProcessParams, native.BeamParams

    def proc(**kw):
        d = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, min_new_tokens=0, forced_bos_token_id=-1,
                 forced_eos_token_id=-1)
        d.update(kw)
        return P(d["repetition_penalty"], d["no_repeat_ngram_size"], d["min_length"], d["min_new_tokens"], d["forced_bos_token_id"],
                 d["forced_eos_token_id"], None, 0, None, 0, d.get("bad"), d.get("bad_len"), d.get("n_bad", 0))

    bad_ids, bad_len = (C.c_int32 * 2)(7, 9), (C.c_int32 * 1)(2)
    good_b, good_g, good_p = BP(nb, 1.0, 0, 1), G(5, 128, 200), proc(min_length=4)
    cases = [
        # every invalid case of m2m_generate_beam
        (BP(33, 1.0, 0, 1), good_g, good_p, "num_beams"), (BP(2, 1.0, 0, 3), good_g, good_p, "num_return_sequences"),
        (BP(4, 1.0, 0, 1), good_g, good_p, "max_batch"), (BP(2, 1.0, 3, 1), good_g, good_p, "early_stopping"),
        (BP(2, math.inf, 0, 1), good_g, good_p, "length_penalty"),
        # ... of the grammar block
        (good_b, G(5, 129, 200), good_p, "n_pitch"), (good_b, G(5, 128, 268), good_p, "vocab_size"), (good_b, G(4, 128, 200), good_p, "pitch_offset"),
        (good_b, G(5, 0, 200), None, "n_pitch"), (good_b, G(5, 128, 0), None, "n_time"),
        # ... of the process block, and the processors that read a row's history
        (good_b, good_g, proc(min_length=-1), "min_length"), (good_b, None, proc(forced_eos_token_id=400), "forced_eos_token_id"),
        (good_b, good_g, proc(repetition_penalty=1.5), "history"), (good_b, None, proc(no_repeat_ngram_size=2), "history"),
        (good_b, good_g, proc(bad=bad_ids, bad_len=bad_len, n_bad=1), "history"),
    ]
    for bp, gp, pp, what in cases:
        rc, tok, sc, _ = _abi_call(model, x, L, bp, gp, pp, rows=B * 32, session_rows=B * nb)
        msg = lib.m2m_last_error().decode()
        print(f"m2m_generate_beam_processed {what}: {rc} {msg}")
        assert rc == M2M_ERR_INVALID and what in msg and "m2m_generate_beam_processed" in msg
        assert bool((tok == -7).all()) and bool((sc == 7.0).all())               # the output buffers are untouched
    # max_length above the processed head's 2048 (and, here, above the session's max_dec: either check refuses the call)
    sess, _ = model._encode(x, L, rows=B * nb)
    n = C.c_int(0)
    out = torch.full((B, 8), -7, dtype=torch.long, device=x.device)
    rc = lib.m2m_generate_beam_processed(sess, 2049, C.byref(good_b), C.byref(good_g), None, out.data_ptr(), None, C.byref(n),
                                         native.stream_handle(x.device))
    assert rc == M2M_ERR_INVALID and bool((out == -7).all())
    rc = lib.m2m_generate_beam_processed(sess, L, None, C.byref(good_g), None, out.data_ptr(), None, C.byref(n), native.stream_handle(x.device))
    assert rc == M2M_ERR_INVALID and "null" in lib.m2m_last_error().decode()
    torch.cuda.synchronize()
    again = _beam(model, x, nb, L, gram=True, min_length=4)                   # nothing faulted: the session still decodes the same
    assert torch.equal(ok[0], again[0]) and torch.equal(ok[1], again[1])
    with pytest.raises(NotImplementedError):
        model.beam_search_processed_from_embeds(x, nb, max_length=L, repetition_penalty=1.3)
    with pytest.raises(ValueError):
        model.beam_search_processed_from_embeds(x, 1, max_length=L, midi_grammar=True)
    ids = model.beam_search_processed_from_embeds(x, nb, max_new_tokens=L - 1, midi_grammar=True, min_length=4).cpu()
    assert torch.equal(ids, ok[0])


def test_music2midi_decodes_with_beams_under_the_grammar():
    from music2midi_amd.model import Music2MIDI
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["inference"].update(num_beams=2, midi_grammar=True)
    m = Music2MIDI(cfg).cuda().eval()
    seen = []
    decode = m.model.beam_search_processed

    def spy(inputs, **kw):
        out = decode(inputs, **kw)
        seen.append((kw, out.cpu()))
        return out
    m.model.beam_search_processed = spy
    from music2midi_amd.grammar import EOS as gr_eos
    audio = synth.waveform_batch(3, 1, 2 * int(m.config.model.sample_rate))[0]          # 2 s: one zero-padded segment
    notes = m.generate_notes(audio_y=audio, cond_index=[4, 2])
    assert notes.ndim == 2 and notes.shape[1] == 4
    assert seen and all(kw.get("midi_grammar") is True and kw.get("num_beams") == 2 and kw.get("num_return_sequences") == 1
                        for kw, _ in seen)
    gr = m.model.tokenizer.grammar
    tok = m.model.tokenizer
    n_tokens = 0
    for _, ids in seen:
        for row in ids.tolist():
            assert bc.walks_inside(gr, row)
            # MidiTokenizer.decode drops no token: every ONSET pitch is a note of the decoder's table (closed or still open), every
            # OFFSET pitch closes one (a distinct (pitch, time) among the closed notes), no pitch stands outside a list, no id is unused
            body = row[1: row.index(gr_eos, 1)] if gr_eos in row[1:] else row[1:]
            mode, n_on, n_off, stray = -1, 0, 0, 0
            for t in body:
                if t >= gr.end or t in (0, 1):
                    stray += 1
                elif t >= gr.time_offset:
                    mode = -1
                elif t >= gr.pitch_offset:
                    n_on, n_off, stray = n_on + (mode == 1), n_off + (mode == 0), stray + (mode == -1)
                else:
                    mode = 1 if t == 3 else 0
            notes = tok._decode_tokens(torch.tensor(row).numpy(), 0)
            closed = notes[notes[:, 1] != -1]
            assert stray == 0 and len(notes) == n_on, (row, n_on, len(notes))
            assert len({(int(p), int(e)) for _, e, p, _ in closed}) == n_off, (row, n_off)
            n_tokens += len(body)
    assert n_tokens > 0
