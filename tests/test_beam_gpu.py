"""Beam search on the GPU (T5Transformer.beam_search / m2m_generate_beam) against the transformers 4.34 restatement.

The restatement (tests/beam_ref.py, itself pinned to recorded HF output by tests/test_beam_cpu.py) runs on the fp32 oracle, so
in fp32 the ids must be equal and the scores agree to float rounding.  Every case prints the smallest decision gap the
restatement met: a device in other arithmetic could only decide differently where that gap is of the size of its rounding.
"""
import ctypes as C
import math

import pytest
import torch

from music2midi_amd import native
from music2midi_amd.config import DEFAULT_CONFIG
from music2midi_amd.transformer import T5Transformer  # noqa: F401  (the model class under test)

from beam_ref import oracle_beam_search
from test_t5_gpu import build, embeds, tiny_config

pytestmark = pytest.mark.gpu
M2M_ERR_INVALID = -1


def _cfg(name):
    return tiny_config() if name == "tiny" else DEFAULT_CONFIG


def _first_eos_trim(row, eos):
    r = row.tolist()
    return r[: r.index(eos) + 1] if eos in r else r


def _hyp_len(row, eos):
    """len of HF's hypothesis score: the start token and the generated ones, EOS not counted"""
    r = row.tolist()
    return r.index(eos, 1) if eos in r[1:] else len(r)


def _assert_ids_equal(got, want, eos):
    assert got.shape[0] == want.shape[0]
    for i in range(got.shape[0]):
        assert _first_eos_trim(got[i], eos) == _first_eos_trim(want[i], eos), (i, got[i].tolist(), want[i].tolist())
    assert torch.equal(got, want), "padding / width differ"


# (config, eos head, B, S, nb, n, length_penalty, early_stopping, max_length, input seed): the seeds are chosen so that the
# restatement's smallest decision gap exceeds 1e-4 (it is deterministic; other seeds of the same shapes go down to 1e-6)
FP32_CASES = [
    ("tiny", False, 1, 19, 2, 1, 1.0, False, 24, 7),
    ("tiny", False, 3, 19, 4, 4, 0.0, True, 24, 7),
    ("tiny", True, 5, 30, 4, 1, 2.0, "never", 24, 9),
    ("tiny", True, 1, 30, 4, 1, 2.0, "never", 40, 7),
    ("tiny", True, 3, 30, 8, 8, -0.5, False, 40, 7),
    ("tiny", True, 3, 30, 2, 2, 1.0, "never", 40, 7),
    ("tiny", True, 5, 30, 8, 1, 1.0, True, 24, 8),
    ("tiny", True, 5, 30, 2, 1, 0.0, True, 32, 7),
    ("full", True, 3, 40, 4, 4, 1.0, False, 24, 7),
    ("full", False, 1, 40, 8, 1, 0.0, "never", 20, 7),
]


@pytest.mark.parametrize("case", FP32_CASES, ids=lambda c: "-".join(map(str, c)))
def test_fp32_beam_equals_the_restatement(case):
    name, eos, B, S, nb, n, lp, es, L, seed = case
    model, orc, g = build(_cfg(name), "fp32", eos=eos)
    x = embeds(B, S, g.d_model, seed=seed)
    want_ids, want_scores, gap = oracle_beam_search(orc, x, nb, L, lp, es, n)
    ids, scores = model.beam_search_from_embeds(x.cuda(), nb, max_length=L, length_penalty=lp, early_stopping=es,
                                                num_return_sequences=n, return_scores=True)
    ids, scores = ids.cpu(), scores.cpu()
    # a score is sum / len ** lp, the sum one fp32 log-softmax term per step.  The device adds a row's exponentials in another
    # order than torch: log(z) differs by about ulp(1) = 1.2e-7 per term (absolute, whatever the term's size - near 0 when one
    # token takes almost all the mass); and its fp32 logits differ from the oracle's in the last bits (fixed-point residual,
    # other summation orders: 2.6e-5 relative on a sum of the full config measured).  So the sums are held to 5e-5 relative
    # plus 5e-7 per term
    lens = torch.tensor([_hyp_len(r, g.eos_token_id) for r in ids], dtype=torch.float64)
    d_sum = (scores.double() - want_scores.double()).abs() * lens ** lp
    bar = 5e-5 * (want_scores.double().abs() * lens ** lp) + 5e-7 * lens
    print(f"beam fp32 {case}: ids {tuple(ids.shape)} min decision gap {gap:.3e} | sum err / bar max {(d_sum / bar).max():.2f}")
    assert gap > 1e-4, "a near-tie in the restatement: choose another case"
    _assert_ids_equal(ids, want_ids, g.eos_token_id)
    assert torch.all(d_sum <= bar)


@pytest.mark.parametrize("name", ["tiny", "full"])
def test_bf16_beam_tracks_the_bf16_restatement(name):
    B, S, nb, n, L = (3, 30, 4, 2, 32) if name == "tiny" else (2, 40, 4, 2, 20)
    model, orc, g = build(_cfg(name), "bf16", eos=True)
    x = embeds(B, S, g.d_model)
    want_ids, want_scores, gap = oracle_beam_search(orc, x, nb, L, 1.0, False, n)
    ids, scores = model.beam_search_from_embeds(x.cuda(), nb, max_length=L, num_return_sequences=n, return_scores=True)
    ids, scores = ids.cpu(), scores.cpu()
    same = ids.shape == want_ids.shape and torch.equal(ids, want_ids)
    print(f"beam bf16 {name}: equal={same} min decision gap {gap:.3e} | scores {scores.tolist()} vs {want_scores.tolist()}")
    if same:
        assert torch.allclose(scores, want_scores, rtol=2e-2, atol=2e-2)
    else:   # the device's bf16 rounding differs from the emulation's in the last bits: only a near-tie may flip a decision
        assert gap < 5e-2


def _teacher_forced_scores(model, x, ids, nb_rows, lp, eos):
    """sum of the token log-probs of each returned row (EOS included) / len ** lp, len = tokens before EOS (or all)."""
    xr = x.repeat_interleave(nb_rows, 0)
    logits = model.logits_from_embeds(xr, ids[:, :-1].cuda()).float().cpu()
    lpb = torch.log_softmax(logits, -1).gather(-1, ids[:, 1:, None]).squeeze(-1)
    out = []
    for i in range(ids.shape[0]):
        r = ids[i].tolist()
        if eos in r[1:]:
            k = r.index(eos, 1)        # tokens before EOS: len = k
            s, ln = lpb[i, :k].sum().item(), k
        else:
            s, ln = lpb[i].sum().item(), len(r)
        out.append(s / ln ** lp)
    return torch.tensor(out)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_scores_are_the_teacher_forced_log_probs(precision):
    B, S, nb, n, lp, L = 3, 30, 4, 4, 1.5, 40
    model, _, g = build(tiny_config(), precision, eos=True)
    x = embeds(B, S, g.d_model).cuda()
    ids, scores = model.beam_search_from_embeds(x, nb, max_length=L, length_penalty=lp, num_return_sequences=n, return_scores=True)
    ids, scores = ids.cpu(), scores.cpu()
    tf = _teacher_forced_scores(model, x, ids, n, lp, g.eos_token_id)
    err = (tf - scores).abs().max().item()
    print(f"beam {precision}: |teacher-forced - reported| max {err:.2e}; scores {scores.tolist()}")
    assert err < (1e-4 if precision == "fp32" else 5e-2)     # bf16: the batched pass rounds in other places than the step
    for c in range(B):
        s = scores[c * n:(c + 1) * n]
        assert torch.all(s[:-1] >= s[1:]), s


def _beam_with_env(monkeypatch, cfg, precision, x, env, nb, L, **kw):
    for k, v in env.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    model, _, _ = build(cfg, precision, eos=True)        # M2M_DA_CLIPS is latched when the session is created: a model per leg
    out = model.beam_search_from_embeds(x, nb, max_length=L, return_scores=True, **kw)
    for k in env:
        monkeypatch.delenv(k, raising=False)
    return out[0].cpu(), out[1].cpu()


@pytest.mark.parametrize("large", [False, True])
def test_kernel_forms_give_identical_beams(monkeypatch, large):
    if large:   # S = 864, 12 clips x 4 beams = 48 rows: the multi-clip attention (C = 2, 4) with the ancestry read and shared cross K/V
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
        ids, scores = _beam_with_env(monkeypatch, cfg, precision, x, env, nb, L, num_return_sequences=2)
        print(f"beam forms {'large' if large else 'small'} {name}: ids {tuple(ids.shape)}")
        if base is None:
            base = (ids, scores)
        else:
            assert torch.equal(ids, base[0]), name
            assert torch.equal(scores, base[1]), name


def test_session_reuse_beam_greedy_beam():
    B, S, nb, L = 3, 30, 4, 40
    model, orc, g = build(tiny_config(), "fp32", eos=True)
    x = embeds(B, S, g.d_model)
    a_ids, a_sc = model.beam_search_from_embeds(x.cuda(), nb, max_length=L, num_return_sequences=2, return_scores=True)
    greedy = model.generate_from_embeds(x.cuda(), max_length=L).cpu()
    assert torch.equal(greedy, orc.generate(x, L))
    b_ids, b_sc = model.beam_search_from_embeds(x.cuda(), nb, max_length=L, num_return_sequences=2, return_scores=True)
    assert torch.equal(a_ids, b_ids) and torch.equal(a_sc, b_sc)


def test_invalid_calls_return_errors_and_launch_nothing():
    B, S, nb, L = 2, 19, 2, 16
    model, _, g = build(tiny_config(), "fp32")
    x = embeds(B, S, g.d_model).cuda()
    ok = model.beam_search_from_embeds(x, nb, max_length=L)          # the session: max_batch = B * nb = 4, encoded B = 2
    lib = native.load()
    sess = model._session
    out = torch.zeros((B * 32, L), dtype=torch.long, device="cuda")
    n_len = C.c_int(0)
    stream = native.stream_handle(x.device)

    def call(p, tokens=out.data_ptr(), length=C.byref(n_len)):
        rc = lib.m2m_generate_beam(sess, L, p, tokens, None, length, stream)
        return rc, lib.m2m_last_error().decode()

    for p, what in [(native.BeamParams(33, 1.0, 0, 1), "num_beams"), (native.BeamParams(2, 1.0, 0, 3), "num_return_sequences"),
                    (native.BeamParams(4, 1.0, 0, 1), "max_batch"), (native.BeamParams(2, 1.0, 3, 1), "early_stopping"),
                    (native.BeamParams(2, math.inf, 0, 1), "length_penalty")]:
        rc, msg = call(C.byref(p))
        print(f"m2m_generate_beam {what}: {rc} {msg}")
        assert rc == M2M_ERR_INVALID and what in msg
    rc, msg = call(None)
    assert rc == M2M_ERR_INVALID and "null" in msg
    rc, msg = call(C.byref(native.BeamParams(2, 1.0, 0, 1)), tokens=None)
    assert rc == M2M_ERR_INVALID and "null" in msg
    torch.cuda.synchronize()
    again = model.beam_search_from_embeds(x, nb, max_length=L)       # nothing faulted: the session still decodes the same
    assert torch.equal(ok, again)
    with pytest.raises(ValueError):
        model.beam_search_from_embeds(x, 1)
