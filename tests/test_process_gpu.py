"""Logits processors (generate(repetition_penalty=..., no_repeat_ngram_size=..., ...)) on the GPU against the oracle restatement
(tests/process_ref.py): fp32 ids exactly, bf16 along the device's own ids, sampled ids inside the processed support."""
import ctypes as C
import os

import pytest
import torch

from music2midi_amd import native, synth
from music2midi_amd.config import DEFAULT_CONFIG
from music2midi_amd.generation import ProcessConfig
from music2midi_amd.input import ModelInputs

import process_ref as pr
from forced_check import BF16_ARGMAX_MARGIN_CAP
from test_sampling_gpu import build_ragged
from test_t5_gpu import build, embeds, tiny_config

pytestmark = pytest.mark.gpu
M2M_ERR_INVALID = -1

_KW = {
    "repetition": dict(repetition_penalty=1.8),
    "penalty_below_1": dict(repetition_penalty=0.6),
    "ngram2": dict(no_repeat_ngram_size=2),
    "ngram4": dict(no_repeat_ngram_size=4),
    "bad_words": dict(bad_words_ids=[[1], [5], [7, 9], [3, 3, 3]]),
    "min_length": dict(min_length=30),
    "min_new_tokens": dict(min_new_tokens=25),
    "forced_bos": dict(forced_bos_token_id=11),
    "forced_eos": dict(forced_eos_token_id=1),
    "suppress": dict(suppress_tokens=[0, 2, 4, 6, 8]),
    "begin_suppress": dict(begin_suppress_tokens=[1, 2, 3], forced_bos_token_id=5),
    "all": dict(repetition_penalty=1.2, no_repeat_ngram_size=3, bad_words_ids=[[1], [2, 2]], min_length=12, min_new_tokens=8,
                forced_bos_token_id=3, forced_eos_token_id=1, suppress_tokens=[4, 9], begin_suppress_tokens=[6]),
}


def _pc(kw, V=400):
    from music2midi_amd.generation import resolve_generate_kwargs
    return resolve_generate_kwargs(kw, vocab_size=V).process


def _gen(model, x, L, **kw):
    return model.generate_from_embeds(x.cuda(), max_length=L, **kw).cpu()


@pytest.mark.parametrize("name", list(_KW))
def test_each_processor_fp32_tiny_equals_the_oracle(name):
    model, orc, g = build(tiny_config(), "fp32")
    x = embeds(5, 19, g.d_model, seed=5)
    L = 40
    got = _gen(model, x, L, **_KW[name])
    want = pr.oracle_generate(orc, x, L, _pc(_KW[name]))
    assert torch.equal(got, want), name
    if name in ("repetition", "ngram2", "ngram4", "all"):    # random-init greedy loops: these processors change the ids
        assert not torch.equal(got, _gen(model, x, L)), name


@pytest.mark.parametrize("compact", ["0", "1"])
def test_all_processors_fp32_ragged_default_config(monkeypatch, compact):
    """rows end at different steps (the re-packing runs with M2M_COMPACT=1): the history follows the clip, not the slot"""
    monkeypatch.setenv("M2M_COMPACT", compact)
    model, orc, g = build_ragged("fp32")
    x = embeds(40, 40, g.d_model, seed=6)
    L = 140
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=4, min_length=20, bad_words_ids=[[7, 8]], suppress_tokens=[3])
    got = _gen(model, x, L, **kw)
    if compact == "1":
        assert model.repack_stats()[1] > 0
    want = pr.oracle_generate(orc, x, L, _pc(kw))
    assert torch.equal(got, want)
    assert not torch.equal(got, _gen(model, x, L))


def test_large_chains_fp32():
    """128 clips: two chains of 64 (the multi-clip attention of four clips and the four-slice feed-forward)"""
    model, orc, g = build(DEFAULT_CONFIG, "fp32")
    x = embeds(128, 24, g.d_model, seed=8)
    kw = dict(repetition_penalty=1.25, no_repeat_ngram_size=3, min_length=16)
    got = _gen(model, x, 40, **kw)
    assert torch.equal(got, pr.oracle_generate(orc, x, 40, _pc(kw)))


def test_bf16_tokens_are_the_processed_argmax_along_the_device_ids():
    model, orc, g = build(DEFAULT_CONFIG, "bf16")
    x = embeds(4, 64, g.d_model, seed=9)
    L = 64
    kw = dict(repetition_penalty=1.2, no_repeat_ngram_size=4, min_length=64)
    pc = _pc(kw)
    ids = _gen(model, x, L, **kw)
    labels = torch.cat([ids[:, 1:], torch.zeros_like(ids[:, :1])], dim=1)
    logits = orc.forward(x, labels)[1]
    checked = 0
    for t in range(ids.shape[1] - 1):
        s = pr.process(ids[:, : t + 1], logits[:, t], pc, g.eos_token_id, L)
        top2 = torch.topk(s, 2, dim=-1)
        for b in range(ids.shape[0]):
            assert ids[b, t + 1] != g.eos_token_id       # min_length = max_length: EOS never allowed
            if top2.values[b, 0] - top2.values[b, 1] >= BF16_ARGMAX_MARGIN_CAP:
                checked += 1
                assert ids[b, t + 1] == top2.indices[b, 0], (b, t)
    assert checked >= ids.numel() // 4


def _sample(model, x, L, seed, **kw):
    torch.manual_seed(seed)
    return model.generate_from_embeds(x.cuda(), max_length=L, do_sample=True, **kw).cpu()


def test_sampled_tokens_respect_the_bans():
    model, _, g = build_ragged("fp32")
    x = embeds(24, 40, g.d_model, seed=10)
    L, n = 60, 3
    kw = dict(no_repeat_ngram_size=n, suppress_tokens=[5, 6], min_length=20, forced_eos_token_id=g.eos_token_id,
              temperature=3.0, top_k=0)
    ids = _sample(model, x, L, 1, **kw)
    for row in ids.tolist():
        end = row.index(g.eos_token_id, 1) if g.eos_token_id in row[1:] else len(row)
        gen = row[: end + 1]
        assert end >= 20, row                                    # no EOS while cur_len < 20
        assert not ({5, 6} & set(gen[1:])), row
        grams = [tuple(gen[i:i + n]) for i in range(len(gen) - n + 1)]
        assert len(grams) == len(set(grams)), row
        if end == len(row):
            pytest.fail("a row ran past max_length - 1 without the forced EOS")
    assert ids.shape[1] <= L


def test_top_k_1_is_processed_greedy_and_seeds_reproduce(monkeypatch):
    model, _, g = build_ragged("fp32")
    x = embeds(40, 40, g.d_model, seed=4)
    kw = dict(repetition_penalty=1.4, no_repeat_ngram_size=3)
    greedy = _gen(model, x, 120, **kw)
    assert torch.equal(_sample(model, x, 120, 2, top_k=1, **kw), greedy)
    skw = dict(kw, temperature=1.5, top_k=40, top_p=0.95)
    monkeypatch.setenv("M2M_COMPACT", "1")
    a = _sample(model, x, 120, 11, **skw)
    monkeypatch.setenv("M2M_COMPACT", "0")
    assert torch.equal(_sample(model, x, 120, 11, **skw), a)
    monkeypatch.setenv("M2M_GROUP_ROWS", "8")
    assert torch.equal(_sample(model, x, 120, 11, **skw), a)
    monkeypatch.delenv("M2M_GROUP_ROWS")
    monkeypatch.setenv("M2M_DA_CLIPS", "4")
    m2, _, _ = build_ragged("fp32")
    assert torch.equal(_sample(m2, x, 120, 11, **skw), a)


def test_session_state_after_a_processed_call():
    model, _, g = build_ragged("fp32")
    x = embeds(40, 40, g.d_model, seed=6)
    greedy = _gen(model, x, 140)
    stats = model.repack_stats()
    sampled = _sample(model, x, 140, 3, temperature=1.5, top_k=40)
    _gen(model, x, 140, repetition_penalty=1.3, no_repeat_ngram_size=2)
    assert model.repack_stats()[1] > 0
    assert torch.equal(_gen(model, x, 140), greedy)
    assert model.repack_stats() == stats
    assert torch.equal(_sample(model, x, 140, 3, temperature=1.5, top_k=40), sampled)


def test_c_abi_rejects_invalid_parameters():
    model, _, g = build(tiny_config(), "fp32")
    x = embeds(2, 12, g.d_model).cuda()
    lib = native.load()
    sess, _ = model._encode(x, 8)
    tokens = torch.empty((2, 8), dtype=torch.long, device=x.device)
    n = C.c_int(0)
    ids = (C.c_int32 * 4)(1, 2, 3, 400)
    lens = (C.c_int32 * 2)(2, 0)
    none = C.POINTER(C.c_int32)()

    def P(**kw):
        f = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, min_new_tokens=0, forced_bos_token_id=-1,
                 forced_eos_token_id=-1, suppress_tokens=none, n_suppress_tokens=0, begin_suppress_tokens=none,
                 n_begin_suppress_tokens=0, bad_words_ids=none, bad_words_lengths=none, n_bad_words=0)
        f.update(kw)
        return native.ProcessParams(**f)

    def call(p, L=8, sp=None):
        return lib.m2m_generate_processed(sess, L, C.byref(p), C.byref(sp) if sp else None, tokens.data_ptr(), C.byref(n),
                                          native.stream_handle(x.device))

    bad = [P(repetition_penalty=0.0), P(repetition_penalty=-1.0), P(repetition_penalty=float("inf")),
           P(repetition_penalty=float("nan")), P(no_repeat_ngram_size=-1), P(min_length=-1), P(min_new_tokens=-2),
           P(forced_bos_token_id=400), P(forced_bos_token_id=-2), P(forced_eos_token_id=400),
           P(suppress_tokens=ids, n_suppress_tokens=4), P(suppress_tokens=none, n_suppress_tokens=1), P(n_suppress_tokens=-1),
           P(begin_suppress_tokens=ids, n_begin_suppress_tokens=4), P(n_begin_suppress_tokens=-1),
           P(bad_words_ids=ids, bad_words_lengths=lens, n_bad_words=2), P(bad_words_ids=ids, bad_words_lengths=none, n_bad_words=1),
           P(n_bad_words=-1)]
    for i, p in enumerate(bad):
        assert call(p) == M2M_ERR_INVALID, i
    for sp in (native.SampleParams(0.0, 50, 1.0, 1), native.SampleParams(1.0, -1, 1.0, 1), native.SampleParams(1.0, 50, 1.5, 1)):
        assert call(P(repetition_penalty=1.2), sp=sp) == M2M_ERR_INVALID
    many = (C.c_int32 * 130)(*([2] * 130))
    two = (C.c_int32 * 65)(*([2] * 65))
    assert call(P(bad_words_ids=many, bad_words_lengths=two, n_bad_words=65)) == M2M_ERR_INVALID   # > 64 sequences
    assert call(P(repetition_penalty=1.2), L=9) == M2M_ERR_INVALID                                  # max_length > session
    assert lib.m2m_generate_processed(sess, 8, None, None, tokens.data_ptr(), C.byref(n), native.stream_handle(x.device)) \
        == M2M_ERR_INVALID
    # nothing active through the processed head = plain greedy
    assert call(P()) == 0
    assert torch.equal(tokens[:, :n.value].cpu(), model.generate_from_embeds(x, max_length=8).cpu())


def test_generate_from_the_waveform():
    model, _, g = build(DEFAULT_CONFIG, "fp32")
    wav = torch.from_numpy(synth.waveform_batch(2, 2, 16000))
    idx = torch.from_numpy(synth.cond_index_batch(2, 2))
    inputs = ModelInputs(input_waveform=wav.cuda(), cond_index=idx.cuda())
    plain = model.generate(inputs, max_length=40).cpu()
    got = model.generate(inputs, max_length=40, repetition_penalty=1.3).cpu()
    x = model.encoder_inputs(inputs)
    assert torch.equal(got, model.generate_from_embeds(x, max_length=40, repetition_penalty=1.3).cpu())
    assert got[:, 0].eq(g.decoder_start_token_id).all() and got.shape[0] == 2
    assert not torch.equal(got, plain)
    assert model.generate(inputs, max_new_tokens=9, min_new_tokens=9).shape[1] == 10
    with pytest.raises(NotImplementedError):
        model.generate(inputs, num_beams=2, repetition_penalty=1.3)
