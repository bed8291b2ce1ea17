"""Sampled decoding (generate(do_sample=True, temperature, top_k, top_p)) on the GPU against the oracle.

The device's draws come from a counter-based hash, not torch's generator, so sampled ids are never compared with HF's samples;
what is checked is what must hold for ANY correct sampler: top_k = 1 is greedy, a seed reproduces its ids whatever the kernel
forms, every sampled token lies in the set the HF warpers allow, and the empirical distribution of many draws matches the warped
softmax.
"""
import ctypes as C
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from music2midi_amd import native, synth
from music2midi_amd.checkpoint import load_t5_state
from music2midi_amd.config import DEFAULT_CONFIG, T5Geometry, load_config
from music2midi_amd.transformer import T5Transformer

from test_t5_gpu import build, embeds, tiny_config

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
M2M_ERR_INVALID = -1


# ----------------------------------------------------------------------------------------------------------------------------
# transformers 4.34 generation/logits_process.py, restated: TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
# (min_tokens_to_keep = 1, filter_value = -inf), applied in _get_logits_warper's order (generation/utils.py).
def hf_warp(scores: torch.Tensor, temperature: float, top_k: int, top_p: float) -> torch.Tensor:
    scores = scores.float()
    if temperature != 1.0:
        scores = scores / temperature
    if top_k != 0:
        k = min(max(top_k, 1), scores.size(-1))
        indices_to_remove = scores < torch.topk(scores, k)[0][..., -1, None]
        scores = scores.masked_fill(indices_to_remove, -float("inf"))
    if top_p < 1.0:
        sorted_logits, sorted_indices = torch.sort(scores, descending=False)
        cumulative_probs = sorted_logits.softmax(dim=-1).cumsum(dim=-1)
        sorted_indices_to_remove = cumulative_probs <= (1 - top_p)
        sorted_indices_to_remove[..., -1:] = 0
        indices_to_remove = sorted_indices_to_remove.scatter(-1, sorted_indices, sorted_indices_to_remove)
        scores = scores.masked_fill(indices_to_remove, -float("inf"))
    return scores


def allowed_mask(logits: torch.Tensor, temperature: float, top_k: int, top_p: float, tol_logit: float, tol_mass: float):
    """[..., V] -> bool mask of the tokens the warpers keep, widened at the two boundaries: a token whose scaled logit is within
    tol_logit of the k-th largest, or whose cumulative mass (ascending, itself included) is within tol_mass of 1 - top_p, counts
    as kept (the device and the oracle round differently there)."""
    x = logits.double() / temperature
    keep = torch.ones_like(x, dtype=torch.bool)
    if top_k != 0:
        k = min(max(top_k, 1), x.size(-1))
        kth = torch.topk(x, k)[0][..., -1, None]
        keep &= x >= kth - tol_logit
    if top_p < 1.0:
        xs = x                                  # the nucleus is taken over the exact top-k survivors
        if top_k != 0:
            xs = x.masked_fill(x < torch.topk(x, min(max(top_k, 1), x.size(-1)))[0][..., -1, None], -float("inf"))
        p = xs.softmax(-1)
        # cumulative mass of each token in ascending order, itself and its ties included
        cum = (p[..., None, :] * (xs[..., None, :] <= xs[..., :, None])).sum(-1)
        keep &= (cum > (1 - top_p) - tol_mass) | (x == x.max(-1, keepdim=True).values)
    return keep


def test_hf_warp_restatement_matches_allowed_mask_without_tolerance():
    """The two restatements agree (no ties in random logits): guards the test helpers themselves."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(64, 400, generator=g) * 3
    for T, k, p in [(1.0, 50, 1.0), (0.7, 5, 1.0), (1.5, 0, 0.9), (2.0, 20, 0.6), (1.0, 0, 0.0), (1.0, 400, 1.0)]:
        want = torch.isfinite(hf_warp(x, T, k, p))
        assert torch.equal(allowed_mask(x, T, k, p, 0.0, 0.0), want), (T, k, p)


# ----------------------------------------------------------------------------------------------------------------------------
def build_ragged(precision):
    """full config with the lm_head crafted so rows emit EOS at different steps and the live-row re-packing runs (the weights of
    tests/test_session_state_gpu.py)"""
    geom = T5Geometry(load_config(DEFAULT_CONFIG).model.t5)
    sd = synth.t5_state_dict(geom, seed=0)
    synth.perturb_layer_norms(sd, 0)
    synth.force_eos_head(sd, geom, active=340, eos_scale=1.6)
    m = T5Transformer(DEFAULT_CONFIG, precision=precision)
    load_t5_state(m, sd, strict=False)
    from oracle.t5 import T5Oracle
    return m.cuda().eval(), T5Oracle(geom, sd, emulate=precision), geom


def _sample(model, x, L, seed, **kw):
    torch.manual_seed(seed)
    return model.generate_from_embeds(x.cuda(), max_length=L, do_sample=True, **kw).cpu()


def _case(golden_dir, name):
    z = np.load(golden_dir / "t5.npz")
    return {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")}


@pytest.mark.parametrize("name", ["tiny", "tiny_eos", "full_s190", "full_eos"])
def test_top_k_1_reproduces_the_golden_greedy_ids(golden_dir, name):
    """do_sample=True, top_k=1 keeps only the arg-max: the fp32 ids are HF's greedy ids of the golden cases."""
    c = _case(golden_dir, name)
    B, S, L, Ld, eos = [int(v) for v in c["meta"]]
    cfg = tiny_config() if name.startswith("tiny") else DEFAULT_CONFIG
    model, _, g = build(cfg, "fp32", eos=bool(eos))
    ids = _sample(model, embeds(B, S, g.d_model), L, 5, top_k=1, temperature=0.8).numpy()
    assert np.array_equal(ids, c["ids"].astype(np.int64))


@pytest.mark.parametrize("compact", ["0", "1"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_top_k_1_is_greedy_on_a_large_batch(monkeypatch, precision, compact):
    """64 clips = two chains of 32 (the two-clip attention and two-slice feed-forward forms), rows ending at different steps (the
    re-packing runs with M2M_COMPACT=1): top_k = 1 gives exactly the greedy ids of the same model."""
    monkeypatch.setenv("M2M_COMPACT", compact)
    model, _, g = build_ragged(precision)
    x = embeds(64, 40, g.d_model, seed=3)
    greedy = model.generate_from_embeds(x.cuda(), max_length=160).cpu()
    moved = model.repack_stats()[1]
    ids = _sample(model, x, 160, 1, top_k=1, top_p=0.9, temperature=1.7)
    assert torch.equal(ids, greedy)
    if compact == "1":
        assert moved > 0 and model.repack_stats()[1] == moved   # same EOS pattern, same re-packings


_SAMPLE_KW = dict(temperature=1.5, top_k=40, top_p=0.95)

_CHILD = """
import sys, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
from music2midi_amd.config import DEFAULT_CONFIG
from test_sampling_gpu import build_ragged, embeds
model, _, g = build_ragged("fp32")
torch.manual_seed(11)
ids = model.generate_from_embeds(embeds(40, 40, g.d_model, seed=4).cuda(), max_length=140, do_sample=True, **%r).cpu()
print("IDS", ",".join(str(int(v)) for v in ids.flatten().tolist()), *ids.shape)
""" % (str(ROOT), str(ROOT / "tests"), _SAMPLE_KW)


def test_seed_reproduces_ids_across_kernel_forms(monkeypatch):
    """Same torch.manual_seed -> identical ids, whether rows are re-packed or not, whatever the chain split, the attention form or
    the greedy head fold (M2M_HEADLESS is latched when a session is created; set for a child process).  Another seed changes the ids."""
    model, _, g = build_ragged("fp32")
    x = embeds(40, 40, g.d_model, seed=4)
    monkeypatch.setenv("M2M_COMPACT", "1")
    a = _sample(model, x, 140, 11, **_SAMPLE_KW)
    assert model.repack_stats()[1] > 0
    assert torch.equal(_sample(model, x, 140, 11, **_SAMPLE_KW), a)
    monkeypatch.setenv("M2M_COMPACT", "0")
    assert torch.equal(_sample(model, x, 140, 11, **_SAMPLE_KW), a)
    monkeypatch.setenv("M2M_GROUP_ROWS", "8")                     # five chains of 8
    assert torch.equal(_sample(model, x, 140, 11, **_SAMPLE_KW), a)
    monkeypatch.delenv("M2M_GROUP_ROWS")
    monkeypatch.setenv("M2M_COMPACT", "1")
    for env in ("1", "4"):                                         # latched when a session is created: a model of its own each
        monkeypatch.setenv("M2M_DA_CLIPS", env)
        m2, _, _ = build_ragged("fp32")
        assert torch.equal(_sample(m2, x, 140, 11, **_SAMPLE_KW), a), env
        del m2
    monkeypatch.delenv("M2M_DA_CLIPS")
    b = _sample(model, x, 140, 12, **_SAMPLE_KW)
    assert not torch.equal(b[:8], a[:8])
    for headless in ("0", "1"):
        env = dict(os.environ, M2M_HEADLESS=headless, OMP_NUM_THREADS="4")
        r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=600)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("IDS")]
        assert r.returncode == 0 and line, r.stdout[-2000:] + r.stderr[-3000:]
        vals, rows, cols = line[-1].split()[1:]
        got = torch.tensor([int(v) for v in vals.split(",")]).view(int(rows), int(cols))
        assert torch.equal(got, a), headless


def _teacher_logits(orc, x, ids):
    """oracle logits along the sampled ids: position t predicts ids[:, t + 1] (forward() shifts its labels right)"""
    labels = torch.cat([ids[:, 1:], torch.zeros_like(ids[:, :1])], dim=1)
    return orc.forward(x, labels)[1]


# Boundary tolerance in RAW logits.  fp32: 1e-4.  bf16: the device and the bf16-emulating oracle round the same storage points but
# accumulate in other orders, and the difference compounds along the sequence; 0.5 is the bf16 noise bound the greedy parity test
# already uses (tests/test_t5_gpu.py test_bf16_mode_tracks_bf16_oracle: ids must agree wherever the oracle's top-2 margin is >= 0.5).
# The nucleus tolerance follows from it: a shift of at most d in every scaled logit moves a softmax by at most 2 d in L1, so any
# cumulative mass by at most 2 * tol / T.
_TOL = {"fp32": 1e-4, "bf16": 0.5}


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_sampled_tokens_lie_in_the_warped_support(precision):
    model, orc, g = build_ragged(precision)
    B, S, L = 6, 40, 40
    x = embeds(B, S, g.d_model, seed=9)
    tol = _TOL[precision]
    for seed, (T, k, p) in enumerate([(1.0, 50, 1.0), (0.7, 10, 1.0), (6.0, 0, 0.9), (12.0, 20, 0.8), (25.0, 0, 0.5)]):
        ids = _sample(model, x, L, 100 + seed, temperature=T, top_k=k, top_p=p)
        logits = _teacher_logits(orc, x, ids)
        ok = allowed_mask(logits, T, k, p, tol / T, 1e-4 if precision == "fp32" else 2 * tol / T)
        n_checked = 0
        for b in range(B):
            row = ids[b].tolist()
            end = row.index(g.eos_token_id, 1) if g.eos_token_id in row[1:] else len(row) - 1
            for t in range(end):                       # every sampled token up to and including EOS
                n_checked += 1
                assert ok[b, t, row[t + 1]], (T, k, p, b, t, row[t + 1])
            assert all(v == g.pad_token_id for v in row[end + 1:]), (b, row)
        assert n_checked >= B


def _first_step_logits(orc, x1):
    return _teacher_logits(orc, x1, torch.zeros((1, 1), dtype=torch.long))[0, 0]


@pytest.mark.parametrize("setting", ["top_k", "top_p"])
def test_sampled_distribution_matches_the_warped_softmax(setting):
    """One clip replicated over 256 rows, one token each (max_length = 2), under 8 seeds: n = 2048 independent draws (every
    (seed, row) pair hashes to its own uniform).  Their histogram over m bins (the 15 most likely tokens + the rest) against the
    oracle's warped softmax, by the L1 bound of Weissman et al. (2003): P(||p_hat - p||_1 >= eps) <= (2^m - 2) exp(-n eps^2 / 2).
    With m = 16, n = 2048 and eps = 0.16: 65534 * exp(-2048 * 0.0256 / 2) = 65534 * exp(-26.2) = 2.7e-7 < 1e-6."""
    model, orc, g = build(DEFAULT_CONFIG, "fp32")
    x1 = embeds(1, 8, g.d_model, seed=13)
    logits = _first_step_logits(orc, x1).double()
    T = float(logits.std()) / 1.5             # random-init logits are ~N(0, 400): scale them to a few bits of entropy
    k, p = (20, 1.0) if setting == "top_k" else (0, 0.7)
    probs = hf_warp(logits, T, k, p).softmax(-1)
    H = float(-(probs[probs > 0] * probs[probs > 0].log2()).sum())
    assert H >= 2.0, H
    if setting == "top_p":
        assert int((probs > 0).sum()) >= 3
    n_rows, seeds = 256, 8
    draws = torch.cat([_sample(model, x1.repeat(n_rows, 1, 1), 2, 1000 + s, temperature=T, top_k=k, top_p=p)[:, 1]
                       for s in range(seeds)])
    assert draws.numel() == 2048
    l1 = assert_draws_follow(probs, draws)
    print(f"{setting}: T={T:.2f} H={H:.2f} bits, support {int((probs > 0).sum())}, L1 {l1:.4f} (bound 0.16)")


def assert_draws_follow(probs, draws):
    """2048 draws against the warped softmax `probs` [V]: every draw in its support, and the histogram over 16 bins (the 15 most likely
    tokens + the rest) within the L1 bound of Weissman et al. (2003) that a correct sampler exceeds with probability < 1e-6; -> L1"""
    n = draws.numel()
    assert n == 2048
    assert bool((probs[draws] > 0).all()), "a draw outside the warped support"
    top = torch.argsort(probs, descending=True)[:15]
    emp = torch.bincount(draws, minlength=probs.numel()).double() / n
    bins_p = torch.cat([probs[top], (1 - probs[top].sum()).clamp_min(0)[None]])
    bins_e = torch.cat([emp[top], (1 - emp[top].sum()).clamp_min(0)[None]])
    m, eps = 16, 0.16
    assert (2 ** m - 2) * math.exp(-n * eps * eps / 2) < 1e-6
    l1 = float((bins_p - bins_e).abs().sum())
    assert l1 < eps, l1
    return l1


# ----------------------------------------------------------------------------------------------------------------------------
def test_num_return_sequences_rows_are_grouped_per_clip():
    model, _, g = build(tiny_config(), "fp32")
    x = embeds(3, 20, g.d_model, seed=2)
    greedy = model.generate_from_embeds(x.cuda(), max_length=24).cpu()
    ids = _sample(model, x, 24, 0, top_k=1, num_return_sequences=4)
    assert ids.shape == (12, greedy.shape[1])
    assert torch.equal(ids, greedy.repeat_interleave(4, dim=0))
    free = _sample(model, x, 24, 0, temperature=3.0, top_k=0, num_return_sequences=4)
    assert free.shape[0] == 12 and (free[:, 0] == g.decoder_start_token_id).all()
    assert len({tuple(r) for r in free[:4].tolist()}) > 1        # the 4 sequences of a clip are drawn independently


def test_invalid_parameters_raise():
    model, _, g = build(tiny_config(), "fp32")
    x = embeds(2, 12, g.d_model).cuda()
    for kw in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")), dict(top_k=-1),
               dict(top_p=1.5), dict(top_p=-0.1), dict(num_return_sequences=0)):
        with pytest.raises(ValueError):
            model.generate_from_embeds(x, max_length=8, do_sample=True, **kw)
    with pytest.raises(NotImplementedError):
        model.generate_from_embeds(x, max_length=8, do_sample=True, num_beams=2)
    # through the C ABI
    lib = native.load()
    sess, _ = model._encode(x, 8)
    tokens = torch.empty((2, 8), dtype=torch.long, device=x.device)
    n = C.c_int(0)
    for T, k, p in [(0.0, 50, 1.0), (float("inf"), 50, 1.0), (1.0, -2, 1.0), (1.0, 50, 1.01), (1.0, 50, float("nan"))]:
        sp = native.SampleParams(T, k, p, 1)
        rc = lib.m2m_generate_sample(sess, 8, C.byref(sp), tokens.data_ptr(), C.byref(n), native.stream_handle(x.device))
        assert rc == M2M_ERR_INVALID, (T, k, p, rc)
    sp = native.SampleParams(1.0, 0, 0.0, 1)                      # top_p = 0 is legal (only the top token)
    assert lib.m2m_generate_sample(sess, 8, C.byref(sp), tokens.data_ptr(), C.byref(n), native.stream_handle(x.device)) == 0
    greedy = model.generate_from_embeds(x, max_length=8).cpu()
    assert torch.equal(tokens[:, :n.value].cpu(), greedy)


def test_generate_surface_and_greedy_unchanged_after_sampling():
    from music2midi_amd import synth
    from music2midi_amd.input import ModelInputs
    model, _, g = build_ragged("fp32")
    x = embeds(40, 40, g.d_model, seed=6)
    greedy = model.generate_from_embeds(x.cuda(), max_length=140).cpu()
    stats = model.repack_stats()
    _sample(model, x, 140, 3, **_SAMPLE_KW)
    assert torch.equal(model.generate_from_embeds(x.cuda(), max_length=140).cpu(), greedy)
    assert model.repack_stats() == stats
    assert torch.equal(model.generate_from_embeds(x.cuda(), max_length=140, do_sample=False).cpu(), greedy)
    wav = torch.from_numpy(synth.waveform_batch(2, 2, 16000))
    idx = torch.from_numpy(synth.cond_index_batch(2, 2))
    inputs = ModelInputs(input_waveform=wav.cuda(), cond_index=idx.cuda())
    with pytest.raises(NotImplementedError):
        model.generate(inputs, num_beams=2, do_sample=True)
    with pytest.raises(ValueError):
        model.generate(inputs, do_sample=True, top_p=2.0)
    torch.manual_seed(4)
    a = model.generate(inputs, do_sample=True, max_length=30, temperature=20.0)
    torch.manual_seed(4)
    b = model.generate(inputs, do_sample=True, max_length=30, temperature=20.0)
    assert torch.equal(a, b) and a.shape[0] == 2
    torch.manual_seed(4)
    c = model.generate(inputs, do_sample=True, max_length=30, temperature=20.0, num_return_sequences=2)
    assert c.shape[0] == 4
    from music2midi.transformer import T5Transformer as Ref
    assert Ref is type(model)
