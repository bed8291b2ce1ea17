"""generate(midi_grammar=True) (m2m_generate_grammar) on the GPU against the oracle restatement (tests/grammar_ref.py: the processed
oracle decode with the token grammar's mask at PrefixConstrainedLogitsProcessor's place): fp32 ids exactly, bf16 along the device's
own ids, sampled ids inside the language, the scores' -inf pattern, the C ABI's checks."""
import copy
import ctypes as C

import pytest
import torch

from music2midi_amd import native, synth
from music2midi_amd.config import DEFAULT_CONFIG
from music2midi_amd.generation import resolve_generate_kwargs
from music2midi_amd.grammar import EOS, MidiGrammar

import grammar_ref as gref
from forced_check import BF16_ARGMAX_MARGIN_CAP
from test_process_gpu import _KW
from test_sampling_gpu import build_ragged
from test_t5_gpu import build, embeds, tiny_config

pytestmark = pytest.mark.gpu
M2M_ERR_INVALID = -1
NEG = -float("inf")
SELF_LOGPROB_BOUND = 1e-4      # DESIGN.md section 16's bar for logprobs against the float64 log_softmax of the device's own rows


def _pc(kw, V=400):
    kw = {k: v for k, v in kw.items() if k != "midi_grammar"}
    return resolve_generate_kwargs(kw, vocab_size=V).process if kw else None


def _gen(model, x, L, **kw):
    return model.generate_from_embeds(x.cuda(), max_length=L, **kw).cpu()


def _accepted(grammar, ids):
    return all(grammar.accepts(row) for row in ids.tolist())


@pytest.fixture(scope="module")
def tiny():
    model, orc, g = build(tiny_config(), "fp32")
    return model, orc, g, embeds(5, 19, g.d_model, seed=5)


def test_fp32_tiny_equals_the_oracle_and_stays_in_the_language(tiny):
    model, orc, g, x = tiny
    L, gr = 40, model.tokenizer.grammar
    got = _gen(model, x, L, midi_grammar=True)
    want = gref.oracle_generate(orc, x, L, None, gr)
    assert torch.equal(got, want)
    assert _accepted(gr, got)
    plain = _gen(model, x, L)
    assert not torch.equal(got, plain) and not _accepted(gr, plain)      # random-init greedy ids mean nothing as MIDI
    assert torch.equal(_gen(model, x, L, midi_grammar=False), plain)


def test_fp32_tiny_with_every_processor(tiny):
    model, orc, g, x = tiny
    L, kw = 40, _KW["all"]
    got = _gen(model, x, L, midi_grammar=True, **kw)
    assert torch.equal(got, gref.oracle_generate(orc, x, L, _pc(kw), model.tokenizer.grammar))
    assert bool((got[:, 1] == kw["forced_bos_token_id"]).all())          # an id the grammar bans at the start: the forced id wins
    assert not torch.equal(got, _gen(model, x, L, **kw))


@pytest.fixture(scope="module")
def ragged_reference():
    return {}


@pytest.mark.parametrize("compact", ["0", "1"])
def test_fp32_ragged_default_config(monkeypatch, ragged_reference, compact):
    """rows end at different steps (the re-packing runs with M2M_COMPACT=1): the state follows the clip, not the slot, and a second
    call starts from fresh states"""
    monkeypatch.setenv("M2M_COMPACT", compact)
    model, orc, g = build_ragged("fp32")
    x = embeds(40, 40, g.d_model, seed=6)
    L, gr = 140, model.tokenizer.grammar
    got = _gen(model, x, L, midi_grammar=True)
    if compact == "1":
        assert model.repack_stats()[1] > 0
    if "want" not in ragged_reference:                                    # the oracle decode once for both settings
        ragged_reference["want"] = gref.oracle_generate(orc, x, L, None, gr)
    assert torch.equal(got, ragged_reference["want"])
    assert _accepted(gr, got)
    assert torch.equal(_gen(model, x, L, midi_grammar=True), got)         # the states were reset


def test_large_chains_fp32():
    """128 clips: two chains of 64"""
    model, orc, g = build(DEFAULT_CONFIG, "fp32")
    x = embeds(128, 24, g.d_model, seed=8)
    got = _gen(model, x, 40, midi_grammar=True)
    assert torch.equal(got, gref.oracle_generate(orc, x, 40, None, model.tokenizer.grammar))


@pytest.mark.parametrize("V,sizes", [(400, (5, 128, 200)), (2048, (5, 100, 1900)), (4096, (7, 128, 3900))])
def test_vocabulary_bands_fp32(V, sizes):
    """NPL = 8, 32, 64 logits per lane: the class boundaries (5 | 133 | 333, 5 | 105 | 2005, 7 | 135 | 4035) fall inside a lane's
    ids, the time compare runs across lanes, and an unused tail (67, 43, 61 ids) exists"""
    cfg = copy.deepcopy(tiny_config())
    cfg["model"]["t5"]["vocab_size"] = V
    cfg["tokenizer"]["vocab_size"] = dict(special=sizes[0], pitch=sizes[1], time=sizes[2])
    model, orc, g = build(cfg, "fp32")
    gr = model.tokenizer.grammar
    assert (gr.pitch_offset, gr.n_pitch, gr.n_time) == sizes and gr.end < V
    x = embeds(4, 19, g.d_model, seed=12)
    got = _gen(model, x, 48, midi_grammar=True)
    assert torch.equal(got, gref.oracle_generate(orc, x, 48, None, gr))
    assert _accepted(gr, got)
    assert int(got.max()) < gr.end and not torch.equal(got, _gen(model, x, 48))


def _sample(model, x, L, seed, **kw):
    torch.manual_seed(seed)
    return model.generate_from_embeds(x.cuda(), max_length=L, do_sample=True, midi_grammar=True, **kw).cpu()


def test_sampling_stays_in_the_language(tiny):
    model, _, g, _ = tiny
    gr = model.tokenizer.grammar
    x = embeds(8, 19, g.d_model, seed=13)
    L = 64
    runs = [_sample(model, x, L, seed, temperature=1.5, top_k=0) for seed in (1, 2)]
    for ids, seed in zip(runs, (1, 2)):
        assert _accepted(gr, ids)
        assert torch.equal(_sample(model, x, L, seed, temperature=1.5, top_k=0), ids)
    assert not torch.equal(runs[0][:, : min(r.shape[1] for r in runs)], runs[1][:, : min(r.shape[1] for r in runs)])
    assert torch.equal(_sample(model, x, L, 3, top_k=1), _gen(model, x, L, midi_grammar=True))


def _scored(model, x, L, **kw):
    out = model.generate_from_embeds(x.cuda(), max_length=L, return_dict_in_generate=True, output_scores=True, output_logprobs=True, **kw)
    ids = out.sequences.cpu()
    return ids, torch.stack(out.scores).cpu(), out.logprobs.cpu()


def test_scores_are_minus_inf_exactly_outside_the_allowed_set(tiny):
    model, _, g, x = tiny
    L, gr, V = 40, model.tokenizer.grammar, g.vocab_size
    ids, scores, logprobs = _scored(model, x, L, midi_grammar=True)
    assert torch.equal(ids, _gen(model, x, L, midi_grammar=True))
    done = (ids[:, 1:] == EOS).cumsum(1) > 0
    live = torch.cat([torch.ones_like(done[:, :1]), ~done[:, :-1]], dim=1)             # [B, T]
    rows = scores.permute(1, 0, 2)                                                       # [B, T, V]
    n_inf = 0
    for t in range(ids.shape[1] - 1):
        mask = gref.grammar_mask(ids[:, : t + 1], V, gr)[live[:, t]]
        got = rows[:, t][live[:, t]]
        assert torch.equal(got == NEG, mask == NEG), t
        n_inf += int((mask == NEG).sum())
    assert n_inf > 0
    assert bool((rows[~live] == 0).all()) and bool((logprobs[~live] == 0).all())
    # inside the allowed set the row is the unconstrained call's row, as long as both calls have decoded the same prefix
    # (teacher-forced common prefix: step 0 and every step up to the first differing id)
    pids, pscores, _ = _scored(model, x, L)
    n_same = 0
    for b in range(ids.shape[0]):
        T = min(ids.shape[1], pids.shape[1]) - 1
        diff = (ids[b, 1: T + 1] != pids[b, 1: T + 1]).nonzero()
        first = int(diff[0]) if len(diff) else T                                        # steps 0 .. first share their prefix
        for t in range(min(first + 1, T)):
            if not live[b, t]:
                break
            fin = torch.isfinite(rows[b, t])
            assert torch.equal(rows[b, t][fin], pscores[t, b][fin]), (b, t)
            n_same += 1
    assert n_same >= ids.shape[0]
    # logprobs against the float64 log_softmax of the device's own rows
    want = torch.log_softmax(rows[live].double(), -1).gather(1, ids[:, 1:][live][:, None])[:, 0]
    err = float((logprobs[live].double() - want).abs().max())
    print(f"constrained logprobs vs float64 log_softmax of the device scores: max err {err:.3e} over {int(live.sum())} positions")
    assert err <= SELF_LOGPROB_BOUND


def test_bf16_tokens_are_the_constrained_argmax_along_the_device_ids():
    """The method of test_process_gpu.test_bf16_tokens_are_the_processed_argmax_along_the_device_ids.  On the CPU the bf16-emulating
    oracle, decoding this seed along its OWN constrained ids, ends its four rows after 44, 28, 28 and 23 tokens (ids [4, 45]) and
    has a top-2 margin >= BF16_ARGMAX_MARGIN_CAP at 116 of its 123 live positions: 64 % of the 180 ids, against the quarter asked
    for here.  (min_length = max_length, as the processed test uses, is not added: once a row has used the last time id and closed
    its notes the grammar allows EOS alone, and banning that too leaves the row no id at all.)"""
    model, orc, g = build(DEFAULT_CONFIG, "bf16")
    gr = model.tokenizer.grammar
    x = embeds(4, 64, g.d_model, seed=9)
    L = 64
    ids = _gen(model, x, L, midi_grammar=True)
    assert _accepted(gr, ids)
    labels = torch.cat([ids[:, 1:], torch.zeros_like(ids[:, :1])], dim=1)
    logits = orc.forward(x, labels)[1]
    done = (ids[:, 1:] == EOS).cumsum(1) > 0
    checked = 0
    for t in range(ids.shape[1] - 1):
        s = gref.process(ids[:, : t + 1], logits[:, t], None, g.eos_token_id, L, gr)
        top2 = torch.topk(s, 2, dim=-1)
        for b in range(ids.shape[0]):
            if t > 0 and done[b, t - 1]:
                continue
            if top2.values[b, 0] - top2.values[b, 1] >= BF16_ARGMAX_MARGIN_CAP:
                checked += 1
                assert ids[b, t + 1] == top2.indices[b, 0], (b, t)
    print(f"bf16 constrained ids: {checked} of {ids.numel()} positions checked")
    assert checked >= ids.numel() // 4


def test_c_abi():
    model, _, g = build(tiny_config(), "fp32")
    x = embeds(2, 12, g.d_model).cuda()
    lib = native.load()
    L, V = 8, g.vocab_size
    tokens = torch.empty((2, L), dtype=torch.long, device=x.device)
    n = C.c_int(0)
    st = native.stream_handle(x.device)

    def call(gp, scores=None, logprobs=None, max_length=L):
        sess, _ = model._encode(x, L)
        return lib.m2m_generate_grammar(sess, max_length, C.byref(gp) if gp is not None else None, None, None, tokens.data_ptr(),
                                        scores.data_ptr() if scores is not None else None,
                                        logprobs.data_ptr() if logprobs is not None else None, C.byref(n), st)

    G = native.GrammarParams
    processed = model.generate_from_embeds(x, max_length=L, min_length=3).cpu()
    for i, gp in enumerate([G(5, 129, 200), G(5, 128, 268), G(273, 128, 1), G(5, 0, 200), G(5, 128, 0), G(-1, 128, 200), G(5, -1, 200),
                            G(5, 128, -3), G(4, 128, 200), G(401, 1, 1)]):
        assert call(gp) == M2M_ERR_INVALID, i
        assert b"m2m_generate_grammar" in lib.m2m_last_error()
    assert call(G(5, 128, 200), max_length=L + 1) == M2M_ERR_INVALID
    assert call(G(5, 128, 267)) == 0                                      # the time ids run to the last id of the vocabulary
    # grammar = NULL is m2m_generate_scored
    scores = torch.full((L - 1, 2, V), 7.0, device=x.device)
    logprobs = torch.full((2, L - 1), 7.0, device=x.device)
    assert call(None, scores, logprobs) == 0
    ids = tokens[:, : n.value].cpu().clone()
    sess, _ = model._encode(x, L)
    s2, l2 = torch.full_like(scores, 7.0), torch.full_like(logprobs, 7.0)
    assert lib.m2m_generate_scored(sess, L, None, None, tokens.data_ptr(), s2.data_ptr(), l2.data_ptr(), C.byref(n), st) == 0
    assert torch.equal(tokens[:, : n.value].cpu(), ids) and torch.equal(s2, scores) and torch.equal(l2, logprobs)
    assert torch.equal(ids, model.generate_from_embeds(x, max_length=L).cpu())
    # the grammar through the ABI is the keyword, and the flag does not outlive its call
    assert call(G(5, 128, 200)) == 0
    assert torch.equal(tokens[:, : n.value].cpu(), model.generate_from_embeds(x, max_length=L, midi_grammar=True).cpu())
    assert torch.equal(model.generate_from_embeds(x, max_length=L, min_length=3).cpu(), processed)
    assert call(None) == 0 and torch.equal(tokens[:, : n.value].cpu(), ids)


def test_music2midi_decodes_constrained_from_a_waveform():
    from music2midi_amd.model import Music2MIDI
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["inference"]["midi_grammar"] = True
    m = Music2MIDI(cfg).cuda().eval()
    seen = []
    generate = m.model.generate

    def spy(inputs, **kw):
        out = generate(inputs, **kw)
        seen.append((kw, out.cpu()))
        return out
    m.model.generate = spy
    audio = synth.waveform_batch(3, 1, 2 * int(m.config.model.sample_rate))[0]          # 2 s: one zero-padded segment
    notes = m.generate_notes(audio_y=audio, cond_index=[4, 2])
    assert notes.ndim == 2 and notes.shape[1] == 4
    assert seen and all(kw.get("midi_grammar") is True for kw, _ in seen)
    gr = m.model.tokenizer.grammar
    assert all(_accepted(gr, ids) for _, ids in seen)
