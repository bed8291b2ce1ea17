"""Per-token scores and log-probabilities of generate (return_dict_in_generate=True with output_scores / output_logprobs,
m2m_generate_scored) on the GPU: against the oracle's teacher-forced logits along the returned ids, against the device's own forced
decode steps bit for bit, and against the restated HF processors and warpers.

Position t of a row (the row of `scores[t]`, column t of `logprobs`) selects the row's token t + 1.  It is LIVE while the row has
not emitted EOS among its tokens 1 .. t; a finished row writes nothing, so both outputs are exactly 0.0 there (HF goes on
scoring finished rows; this project does not)."""
import ctypes as C

import numpy as np
import pytest
import torch

from music2midi_amd import native
from music2midi_amd.config import DEFAULT_CONFIG
from music2midi_amd.generation import resolve_generate_kwargs

import process_ref as pr
from forced_check import FP32_LOGIT_ERR_BOUND, forced_logits
from test_process_gpu import _KW
from test_sampling_gpu import allowed_mask, build_ragged
from test_t5_gpu import build, embeds, tiny_config

pytestmark = pytest.mark.gpu
M2M_ERR_INVALID = -1
NEG = -float("inf")
LOGPROB_ERR_BOUND = 2 * FP32_LOGIT_ERR_BOUND    # a logit error of e moves a log-softmax by at most 2 e
# log_softmax in fp32 (max, exp, sum, log over <= 4096 logits of magnitude <= 128) against float64 over the same row: the
# subtraction x - m rounds at 2^-24 * 256 = 1.5e-5, exp and log add a few ulp of values <= 1 and <= ln(4096) + 256: ~2e-5 in all;
# the bar leaves a 5x margin
SELF_LOGPROB_BOUND = 1e-4
SCORE_MAGNITUDE = 128.0


def _scored(model, x, L, **kw):
    kw.setdefault("output_scores", True)
    kw.setdefault("output_logprobs", True)
    out = model.generate_from_embeds(x.cuda(), max_length=L, return_dict_in_generate=True, **kw)
    seq = out.sequences.cpu()
    T = seq.shape[1] - 1
    scores = logprobs = None
    if out.scores is not None:
        assert isinstance(out.scores, tuple) and len(out.scores) == T
        assert all(s.shape == (seq.shape[0], model.geometry.vocab_size) and s.dtype == torch.float32 for s in out.scores)
        scores = torch.stack(out.scores).cpu() if T else torch.zeros(0, seq.shape[0], model.geometry.vocab_size)
    if out.logprobs is not None:
        assert out.logprobs.shape == (seq.shape[0], T) and out.logprobs.dtype == torch.float32
        logprobs = out.logprobs.cpu()
    return seq, scores, logprobs


def _live(ids, eos):
    """[B, T] bool: position t is scored (no EOS among the row's tokens 1 .. t)"""
    done = (ids[:, 1:] == eos).cumsum(1) > 0
    return torch.cat([torch.ones_like(done[:, :1]), ~done[:, :-1]], dim=1)


def _teacher_logits(orc, x, ids):
    labels = torch.cat([ids[:, 1:], torch.zeros_like(ids[:, :1])], dim=1)
    return orc.forward(x, labels)[1][:, : ids.shape[1] - 1]          # [B, T, V]


def _check_self_logprobs(ids, scores, logprobs, live):
    """logprobs against the float64 log_softmax of the device's own rows; finished positions exactly zero in both outputs"""
    sel = scores.permute(1, 0, 2)[live]                                # [n, V]
    assert float(sel[torch.isfinite(sel)].abs().max()) <= SCORE_MAGNITUDE
    want = torch.log_softmax(sel.double(), -1).gather(1, ids[:, 1:][live][:, None])[:, 0]
    err = float((logprobs[live].double() - want).abs().max())
    print(f"logprobs vs float64 log_softmax of the device scores: max err {err:.3e} over {int(live.sum())} positions")
    assert err <= SELF_LOGPROB_BOUND
    assert bool((scores.permute(1, 0, 2)[~live] == 0).all()) and bool((logprobs[~live] == 0).all())


def _check_greedy_against_oracle(orc, x, g, ids, scores, logprobs):
    live = _live(ids, g.eos_token_id)
    assert int(live.sum()) >= ids.shape[0]
    ref = _teacher_logits(orc, x, ids)
    err = float((scores.permute(1, 0, 2)[live] - ref[live]).abs().max())
    ref_lp = torch.log_softmax(ref.double(), -1).gather(2, ids[:, 1:, None])[..., 0]
    err_lp = float((logprobs.double() - ref_lp)[live].abs().max())
    print(f"greedy scores vs oracle: max logit err {err:.3e}, max logprob err {err_lp:.3e}, {int(live.sum())} live positions, "
          f"{int((~live).sum())} finished")
    assert err <= FP32_LOGIT_ERR_BOUND
    assert err_lp <= LOGPROB_ERR_BOUND
    _check_self_logprobs(ids, scores, logprobs, live)


@pytest.fixture(scope="module")
def tiny():
    model, orc, g = build(tiny_config(), "fp32")
    return model, orc, g, embeds(5, 19, g.d_model, seed=5)


def test_greedy_scores_fp32_tiny_against_the_oracle(tiny):
    model, orc, g, x = tiny
    L = 40
    plain = model.generate_from_embeds(x.cuda(), max_length=L).cpu()
    ids, scores, logprobs = _scored(model, x, L)
    assert torch.equal(ids, plain)
    assert scores.shape == (ids.shape[1] - 1, 5, g.vocab_size)
    _check_greedy_against_oracle(orc, x, g, ids, scores, logprobs)
    # compute_transition_scores over the returned scores is the logprobs output (live positions; finished rows hold zeros)
    live = _live(ids, g.eos_token_id)
    tr = model.compute_transition_scores(ids, tuple(scores.unbind(0)), normalize_logits=True)
    assert float((tr - logprobs)[live].abs().max()) <= SELF_LOGPROB_BOUND


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_the_row_written_is_the_row_selected_from(precision):
    """greedy scores == the logits of the device's own forced decode steps along the returned ids, bit for bit"""
    model, _, g = build(DEFAULT_CONFIG, precision)
    x = embeds(4, 64, g.d_model, seed=9)
    ids, scores, _ = _scored(model, x, 64, output_logprobs=False)
    assert torch.equal(ids, model.generate_from_embeds(x.cuda(), max_length=64).cpu())
    want = torch.from_numpy(forced_logits(model, x.cuda(), ids[:, :-1].contiguous().cuda(), "step"))      # [B, T, V]
    live = _live(ids, g.eos_token_id)
    assert int(live.sum()) >= 4 * 8
    got = scores.permute(1, 0, 2)
    assert torch.equal(got[live], want[live])
    assert torch.equal(got[live].argmax(-1), ids[:, 1:][live])


@pytest.fixture(scope="module")
def ragged_reference():
    return {}


@pytest.mark.parametrize("compact", ["0", "1"])
def test_ragged_rows_and_repacking(monkeypatch, ragged_reference, compact):
    monkeypatch.setenv("M2M_COMPACT", compact)
    model, orc, g = build_ragged("fp32")
    x = embeds(40, 40, g.d_model, seed=6)
    ids, scores, logprobs = _scored(model, x, 140)
    if compact == "1":
        assert model.repack_stats()[1] > 0
    live = _live(ids, g.eos_token_id)
    assert int((~live).sum()) > 0                        # rows end at different steps
    assert bool((scores.permute(1, 0, 2)[~live] == 0).all()) and bool((logprobs[~live] == 0).all())
    if ragged_reference:                                 # the other setting ran first: bit-identical, checked once against the oracle
        for a, b in zip((ids, scores, logprobs), ragged_reference["out"]):
            assert torch.equal(a, b)
    else:
        ragged_reference["out"] = (ids, scores, logprobs)
        assert torch.equal(ids, model.generate_from_embeds(x.cuda(), max_length=140).cpu())
        _check_greedy_against_oracle(orc, x, g, ids, scores, logprobs)


def test_large_chains_fp32():
    """128 clips: two chains of 64 (the multi-clip attention of four clips and the four-slice feed-forward) feed the head"""
    model, orc, g = build(DEFAULT_CONFIG, "fp32")
    x = embeds(128, 24, g.d_model, seed=8)
    ids, scores, logprobs = _scored(model, x, 40)
    assert torch.equal(ids, model.generate_from_embeds(x.cuda(), max_length=40).cpu())
    _check_greedy_against_oracle(orc, x, g, ids, scores, logprobs)


def test_processed_scores_are_the_rows_after_the_processors(tiny):
    model, orc, g, x = tiny
    L, kw = 40, _KW["all"]
    pc = resolve_generate_kwargs(kw, vocab_size=g.vocab_size).process
    ids, scores, logprobs = _scored(model, x, L, **kw)
    assert torch.equal(ids, pr.oracle_generate(orc, x, L, pc))
    assert torch.equal(ids, model.generate_from_embeds(x.cuda(), max_length=L, **kw).cpu())
    ref = _teacher_logits(orc, x, ids)
    live = _live(ids, g.eos_token_id)
    bound = FP32_LOGIT_ERR_BOUND * max(pc.repetition_penalty, 1 / pc.repetition_penalty)
    n_inf = 0
    for t in range(ids.shape[1] - 1):
        want = pr.process(ids[:, : t + 1], ref[:, t], pc, g.eos_token_id, L)[live[:, t]]
        got = scores[t][live[:, t]]
        assert torch.equal(got == NEG, want == NEG), t
        fin = want != NEG
        assert float((got[fin] - want[fin]).abs().max()) <= bound, t
        n_inf += int((~fin).sum())
    assert n_inf > 0
    _check_self_logprobs(ids, scores, logprobs, live)


def _sampled(model, x, L, seed, **kw):
    torch.manual_seed(seed)
    return _scored(model, x, L, do_sample=True, **kw)


def test_sampled_scores_with_temperature_only(tiny):
    model, orc, g, x = tiny
    ids, scores, logprobs = _sampled(model, x, 40, 3, temperature=2.0, top_k=0, top_p=1.0)
    live = _live(ids, g.eos_token_id)
    ref = _teacher_logits(orc, x, ids) / 2.0
    err = float((scores.permute(1, 0, 2)[live] - ref[live]).abs().max())
    print(f"sampled scores (temperature 2) vs oracle logits / 2: max err {err:.3e}")
    assert err <= 1e-3
    assert not torch.equal(ids, model.generate_from_embeds(x.cuda(), max_length=40).cpu())
    _check_self_logprobs(ids, scores, logprobs, live)


def test_sampled_scores_with_filters():
    model, orc, g = build_ragged("fp32")
    B, S, L = 6, 40, 40
    x = embeds(B, S, g.d_model, seed=9)
    T, k, p = 1.5, 40, 0.95
    tol = 1e-4                                                   # test_sampling_gpu._TOL["fp32"]
    ids, scores, logprobs = _sampled(model, x, L, 21, temperature=T, top_k=k, top_p=p)
    live = _live(ids, g.eos_token_id)
    rows = scores.permute(1, 0, 2)                               # [B, T, V]
    finite = torch.isfinite(rows)
    assert int(finite.sum(-1)[live].max()) <= k
    assert bool(finite.gather(2, ids[:, 1:, None])[..., 0][live].all())
    ref = _teacher_logits(orc, x, ids)
    may = allowed_mask(ref, T, k, p, tol / T, 1e-4)
    must = allowed_mask(ref, T, k, p, -tol / T, -1e-4)
    assert not bool((finite & ~may)[live].any()) and not bool((must & ~finite)[live].any())
    err = float((rows - ref / T)[live][finite[live]].abs().max())
    assert err <= FP32_LOGIT_ERR_BOUND
    _check_self_logprobs(ids, scores, logprobs, live)
    again = _sampled(model, x, L, 21, temperature=T, top_k=k, top_p=p)
    for a, b in zip((ids, scores, logprobs), again):
        assert torch.equal(a, b)
    assert not torch.equal(_sampled(model, x, L, 22, temperature=T, top_k=k, top_p=p)[0], ids)


def test_output_combinations_and_grouping(tiny):
    model, _, g, x = tiny
    kw = dict(temperature=1.5, top_k=40, top_p=0.95)
    both = _sampled(model, x, 40, 5, **kw)
    lp_only = _sampled(model, x, 40, 5, output_scores=False, **kw)
    sc_only = _sampled(model, x, 40, 5, output_logprobs=False, **kw)
    assert lp_only[1] is None and sc_only[2] is None
    assert torch.equal(lp_only[0], both[0]) and torch.equal(sc_only[0], both[0])
    assert torch.equal(lp_only[2], both[2]) and torch.equal(sc_only[1], both[1])
    torch.manual_seed(5)
    assert torch.equal(model.generate_from_embeds(x.cuda(), max_length=40, do_sample=True, **kw).cpu(), both[0])
    # neither output: the plain decode in a dict
    out = model.generate_from_embeds(x.cuda(), max_length=40, return_dict_in_generate=True)
    greedy = model.generate_from_embeds(x.cuda(), max_length=40).cpu()
    assert out.scores is None and out.logprobs is None and torch.equal(out["sequences"].cpu(), greedy)
    # output_scores without return_dict_in_generate: the plain tensor (4.34)
    assert torch.equal(model.generate_from_embeds(x.cuda(), max_length=40, output_scores=True).cpu(), greedy)
    # num_return_sequences: the n rows of a clip are consecutive (top_k = 1 keeps the arg-max: every copy is the clip's greedy row)
    ids, scores, logprobs = _sampled(model, x, 40, 6, top_k=1, num_return_sequences=3)
    assert ids.shape[0] == 15 and scores.shape[1:] == (15, g.vocab_size) and logprobs.shape[0] == 15
    assert torch.equal(ids, greedy.repeat_interleave(3, dim=0))
    live = _live(ids, g.eos_token_id)
    assert bool((torch.isfinite(scores).sum(-1).T[live] == 1).all()) and bool((logprobs[live] == 0).all())


def test_c_abi(golden_dir):
    z = np.load(golden_dir / "t5.npz")
    B, S, L, _, eos = [int(v) for v in z["tiny_eos/meta"]]
    golden = torch.from_numpy(z["tiny_eos/ids"].astype(np.int64))
    model, _, g = build(tiny_config(), "fp32", eos=bool(eos))
    x = embeds(B, S, g.d_model).cuda()
    assert torch.equal(model.generate_from_embeds(x, max_length=L).cpu(), golden)
    stats = model.repack_stats()
    lib = native.load()
    V, n = g.vocab_size, C.c_int(0)
    st = native.stream_handle(x.device)

    def call(tokens, scores, logprobs, max_length=L):
        sess, _ = model._encode(x, L)
        return lib.m2m_generate_scored(sess, max_length, None, None, tokens.data_ptr() if tokens is not None else None,
                                       scores.data_ptr() if scores is not None else None,
                                       logprobs.data_ptr() if logprobs is not None else None, C.byref(n), st)

    tokens = torch.empty((B, L), dtype=torch.long, device=x.device)
    scores = torch.full((L - 1, B, V), 7.0, device=x.device)
    logprobs = torch.full((B, L - 1), 7.0, device=x.device)
    # both outputs NULL: m2m_generate_greedy
    assert call(tokens, None, None) == 0
    assert torch.equal(tokens[:, : n.value].cpu(), golden)
    # invalid arguments: refused with a message, nothing written
    for rc in (call(None, scores, logprobs), call(None, None, None), call(tokens, scores, logprobs, max_length=L + 1),
               call(tokens, scores, logprobs, max_length=0), call(tokens, None, None, max_length=L + 1)):
        assert rc == M2M_ERR_INVALID
        assert b"m2m_generate" in lib.m2m_last_error()
    assert bool((scores == 7.0).all()) and bool((logprobs == 7.0).all())
    # one output at a time, then both: the same ids, and the buffers are zeroed where a row had finished
    assert call(tokens, None, logprobs) == 0 and torch.equal(tokens[:, : n.value].cpu(), golden)
    lp1 = logprobs.clone()
    logprobs.fill_(7.0)
    assert call(tokens, scores, logprobs) == 0 and torch.equal(tokens[:, : n.value].cpu(), golden)
    assert torch.equal(logprobs, lp1)
    live = _live(golden, g.eos_token_id)
    T = golden.shape[1] - 1
    assert bool((logprobs.cpu()[:, :T][~live] == 0).all()) and bool((logprobs.cpu()[:, :T][live] < 0).all())
    assert bool((scores.cpu()[:T].permute(1, 0, 2)[~live] == 0).all())
    assert bool((logprobs.cpu()[:, T:] == 0).all()) and bool((scores.cpu()[T:] == 0).all())
    # the head mode was restored: plain greedy and its re-packing statistics are what they were
    assert torch.equal(model.generate_from_embeds(x, max_length=L).cpu(), golden)
    assert model.repack_stats() == stats
