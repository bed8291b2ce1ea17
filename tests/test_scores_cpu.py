"""Per-token scores of generate: the keyword resolution (music2midi_amd/generation.py) and compute_transition_scores, the torch
restatement of transformers 4.34's function for the non-beam case.  No GPU."""
import pytest
import torch

from music2midi_amd import native
from music2midi_amd.generation import GenerateConfig, resolve_generate_kwargs
from music2midi_amd.transformer import T5Transformer


def test_defaults_are_a_plain_call():
    cfg = resolve_generate_kwargs({})
    assert (cfg.return_dict, cfg.output_scores, cfg.output_logprobs) == (False, False, False)
    assert cfg == GenerateConfig()
    assert resolve_generate_kwargs({"return_dict_in_generate": False, "output_scores": False, "output_logprobs": False}) == cfg


def test_return_dict_selects_the_outputs():
    cfg = resolve_generate_kwargs({"return_dict_in_generate": True})
    assert (cfg.return_dict, cfg.output_scores, cfg.output_logprobs) == (True, False, False)
    cfg = resolve_generate_kwargs({"return_dict_in_generate": True, "output_scores": True, "max_length": 9})
    assert (cfg.return_dict, cfg.output_scores, cfg.output_logprobs, cfg.max_length) == (True, True, False, 9)
    cfg = resolve_generate_kwargs({"return_dict_in_generate": True, "output_logprobs": True, "do_sample": True, "top_k": 7,
                                   "num_return_sequences": 3, "repetition_penalty": 1.2})
    assert (cfg.return_dict, cfg.output_scores, cfg.output_logprobs) == (True, False, True)
    assert cfg.do_sample and cfg.top_k == 7 and cfg.num_return_sequences == 3 and cfg.process.repetition_penalty == 1.2
    with pytest.raises(NotImplementedError, match="beam_search"):          # beams keep their own entry point
        resolve_generate_kwargs({"return_dict_in_generate": True, "output_scores": True, "num_beams": 2})


def test_output_scores_without_return_dict_is_a_plain_call():
    """4.34: generate returns the tensor unless return_dict_in_generate=True, whatever output_scores says"""
    assert resolve_generate_kwargs({"output_scores": True}) == GenerateConfig()
    assert resolve_generate_kwargs({"output_scores": True, "return_dict_in_generate": False, "max_length": 7}) == GenerateConfig(max_length=7)


def test_output_logprobs_needs_return_dict():
    with pytest.raises(ValueError, match="return_dict_in_generate"):
        resolve_generate_kwargs({"output_logprobs": True})
    with pytest.raises(ValueError, match="return_dict_in_generate"):
        resolve_generate_kwargs({"output_logprobs": True, "output_scores": True, "return_dict_in_generate": False})


def test_scores_need_a_vocabulary_the_head_holds():
    with pytest.raises(ValueError, match="4096"):
        resolve_generate_kwargs({"return_dict_in_generate": True, "output_scores": True}, vocab_size=4097)
    with pytest.raises(ValueError, match="4096"):
        resolve_generate_kwargs({"return_dict_in_generate": True, "output_logprobs": True}, vocab_size=4097)
    assert resolve_generate_kwargs({"return_dict_in_generate": True}, vocab_size=4097).return_dict


@pytest.mark.parametrize("kw", [dict(output_attentions=True), dict(output_hidden_states=True), dict(renormalize_logits=True),
                                dict(penalty_alpha=0.5), dict(output_score=True)])
def test_other_keywords_still_raise(kw):
    """... and the message names the keyword that is not supported, not the three that now are"""
    with pytest.raises(NotImplementedError) as e:
        resolve_generate_kwargs(dict(kw, return_dict_in_generate=True, output_scores=True, output_logprobs=True))
    assert str(sorted(kw)) in str(e.value)
    with pytest.raises(NotImplementedError):
        resolve_generate_kwargs(kw)


def test_the_export_is_declared():
    assert "m2m_generate_scored" in native.EXPORTED_SYMBOLS
    _, args = native._SIGNATURES["m2m_generate_scored"]
    assert len(args) == 9      # session, max_length, proc, sample, tokens, scores, logprobs, out_len, stream


def _random_scores(T, B, V, seed):
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(T, B, V, generator=g) * 4
    s[torch.rand(T, B, V, generator=g) < 0.3] = -float("inf")
    seq = torch.randint(0, V, (B, T + 1), generator=g)
    for t in range(T):          # the selected entry is finite, as in a real decode
        s[t, torch.arange(B), seq[:, t + 1]] = torch.randn(B, generator=g)
    return s, seq


@pytest.mark.parametrize("T,B,V", [(1, 1, 2), (7, 3, 50), (12, 5, 400)])
def test_compute_transition_scores_is_a_gather(T, B, V):
    s, seq = _random_scores(T, B, V, T)
    scores = tuple(s.unbind(0))
    assert (s == -float("inf")).any() or V == 2
    want = torch.stack([s[t, torch.arange(B), seq[:, t + 1]] for t in range(T)], dim=1)
    got = T5Transformer.compute_transition_scores(seq, scores)
    assert got.shape == (B, T) and torch.equal(got, want)
    ls = torch.log_softmax(s, dim=-1)
    want_n = torch.stack([ls[t, torch.arange(B), seq[:, t + 1]] for t in range(T)], dim=1)
    got_n = T5Transformer.compute_transition_scores(seq, scores, normalize_logits=True)
    assert torch.equal(got_n, want_n) and torch.isfinite(got_n).all() and (got_n <= 0).all()
    with pytest.raises(NotImplementedError):
        T5Transformer.compute_transition_scores(seq, scores, beam_indices=torch.zeros(B, T, dtype=torch.long))


def test_compute_transition_scores_matches_transformers():
    tf = pytest.importorskip("transformers")
    if not hasattr(tf.GenerationMixin, "compute_transition_scores"):
        pytest.skip("this transformers has no compute_transition_scores")
    from types import SimpleNamespace
    s, seq = _random_scores(9, 4, 60, 3)
    cfg = SimpleNamespace(vocab_size=60, is_encoder_decoder=True)
    cfg.get_text_config = lambda *a, **k: cfg          # later versions read the vocabulary size through it
    hf = SimpleNamespace(config=cfg)
    for norm in (False, True):
        want = tf.GenerationMixin.compute_transition_scores(hf, seq, tuple(s.unbind(0)), normalize_logits=norm)
        got = T5Transformer.compute_transition_scores(seq, tuple(s.unbind(0)), normalize_logits=norm)
        assert torch.allclose(got, want, atol=1e-6, rtol=0), norm
