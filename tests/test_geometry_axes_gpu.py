"""GPU parity along the geometry keys config.yaml sets and the rest of the suite holds fixed: vocabulary size, the special token
ids, the relative-position bucket geometry and the trainer's widths, each against the CPU oracle (oracle/t5.py, autograd over
oracle/train.py, the HF warper restatement of tests/test_sampling_gpu.py).

Vocabulary sizes are chosen at the column edges of the kernels: dec_head_kernel's 512-column register batch, the 16-column tiles of
the lm_head (the headless arg-max fold masks the zero-padded rows past V), the four logits-per-lane bands of dec_sample_kernel
(V <= 512 / 1024 / 2048 / 4096), the trainer's logits row padded to a multiple of 8.  The lm_heads are crafted so that the ids
depend on exactly those columns."""
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
from music2midi_amd.config import T5Geometry, load_config
from music2midi_amd.transformer import T5Transformer

from test_sampling_gpu import _sample, _teacher_logits, allowed_mask, assert_draws_follow, hf_warp
from test_t5_gpu import embeds, tiny_config
from test_train_gpu import _setup, check_bf16_step, check_fp32_step, check_fp8_step

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
M2M_ERR_INVALID = -1

VOCABS = [3, 17, 64, 400, 511, 513, 1025, 2049, 4096, 4097, 32128]
BF16_VOCABS = [17, 513, 2049, 32128]


def geom_config(vocab_size=400, d_model=128, d_ff=256, num_heads=2, **t5):
    """the tiny model (2 + 2 layers) with other geometry keys"""
    cfg = tiny_config()
    cfg["model"]["t5"].update(vocab_size=vocab_size, d_model=d_model, d_ff=d_ff, num_heads=num_heads, **t5)
    return cfg


def race_rows(geom):
    """lm_head rows that compete for the arg-max: the edges of the register batch (511 | 512), of the 32-lane column groups and of
    the sampling bands, the first column of the last (partial) 16-column tile, V - 2, V - 1 and EOS; never pad"""
    V = geom.vocab_size
    cand = {3, 9, 31, 32, 255, 500, 511, 512, 513, 1023, 1024, 2047, 2048, 4095, 4096, 16 * ((V - 1) // 16), V - 17, V - 2, V - 1,
            geom.eos_token_id}
    return sorted(r for r in cand if 0 <= r < V and r != geom.pad_token_id)


def tail_head(sd, geom, dups=()):
    """Every lm_head row but race_rows zeroed (their logits are exactly 0), EOS scaled down so rows end at different steps, V - 1
    scaled up so that it wins some steps.  dups = ((a, b), ...): row b becomes a copy of row a (a < b): exactly tied logits, the
    lower index must win."""
    w = sd["transformer.lm_head.weight"]
    rows = race_rows(geom)
    keep = w[rows].copy()
    w[:] = 0.0
    w[rows] = keep
    w[geom.eos_token_id] *= 0.35
    w[geom.vocab_size - 1] *= 1.2
    for a, b in dups:
        w[b] = w[a]


def build_geom(cfg, precision, seed=0, head=None):
    geom = T5Geometry(load_config(cfg).model.t5)
    sd = synth.t5_state_dict(geom, seed=seed)
    synth.perturb_layer_norms(sd, seed)
    if head is not None:
        head(sd, geom)
    model = T5Transformer(cfg, precision=precision)
    load_t5_state(model, sd, strict=False)
    from oracle.t5 import T5Oracle
    return model.cuda().eval(), T5Oracle(geom, sd, emulate=precision), geom, sd


def oracle_greedy(orc, x, L, dups=()):
    """the oracle's greedy ids with every duplicate row's logit replaced by its first row's (the CPU BLAS need not make identical
    rows tie bit for bit; the device's products do): torch.argmax then takes the lower index, as HF does on an exact tie"""
    def collapse(t, logits):
        for a, b in dups:
            logits[:, b] = logits[:, a]
    return orc.generate(x, L, return_margins=True, logits_hook=collapse if dups else None)


def assert_bf16_ids_track(out, ref, margins):
    """the bf16 rule of tests/test_t5_gpu.py test_bf16_mode_tracks_bf16_oracle: ids equal up to the first divergence, which may
    only happen where the oracle's top-2 margin is below 0.5"""
    n = min(out.shape[1], ref.shape[1])
    for b in range(out.shape[0]):
        for t in range(1, n):
            if out[b, t] != ref[b, t]:
                assert margins[b, t - 1] < 0.5, f"row {b} step {t}: diverged at margin {margins[b, t - 1]:.3f}"
                break


# (a, b): a, a frequent winner of the race, copied over b across a 32-lane group, the register batch, into the last tile or V - 1
DUPS = {513: ((32, 512), (255, 511), (3, 31)), 2049: ((500, 2048), (255, 1024), (9, 1023))}


def check_greedy(V, precision, dups=(), ids=None):
    """greedy ids of a tail-dependent head against the oracle (fp32: equal; bf16: the margin rule); the case must really decode
    the tail columns.  Called in this process (M2M_HEADLESS=1, the arg-max folded into the lm_head product) and in a child
    process with M2M_HEADLESS=0 (dec_head_kernel)."""
    cfg = geom_config(V, **(ids or {}))
    model, orc, g, _ = build_geom(cfg, precision, head=lambda sd, geom: tail_head(sd, geom, dups))
    B, S, L = 6, 19, 40
    x = embeds(B, S, g.d_model, seed=V % 97)
    ref, margins = oracle_greedy(orc, x, L, dups)
    out = model.generate_from_embeds(x.cuda(), max_length=L).cpu()
    if precision == "fp32":
        assert out.shape == ref.shape and torch.equal(out, ref), (V, dups, out, ref)
    else:
        assert_bf16_ids_track(out, ref, margins)
    seen = set(ref[:, 1:].flatten().tolist())
    assert V - 1 in seen or (V - 1) in {b for _, b in dups}, (V, sorted(seen))
    if V > 512:
        assert max(seen) >= 512 or max(b for _, b in dups) >= 512, (V, sorted(seen))
    for a, _ in dups:                                  # every tie is decided at least once
        assert a in seen, (V, a, sorted(seen))
    return ref


# ----------------------------------------------------------------------------------------------------------- 1. vocabulary, decode
@pytest.mark.parametrize("V", VOCABS)
def test_vocab_size_through_encode_greedy_and_forced_logits_fp32(monkeypatch, V):
    check_greedy(V, "fp32")
    model, orc, g, _ = build_geom(geom_config(V), "fp32", head=tail_head)
    B, S, Ld = 3, 23, 21
    x = embeds(B, S, g.d_model, seed=5)
    assert (model.encode(x.cuda()).cpu() - orc.encode(x)).abs().max().item() < 2e-4
    labels = torch.from_numpy((synth.uniform01(V, "labels", B * Ld) * V).astype(np.int64).reshape(B, Ld))
    labels[0, :3] = torch.tensor([V - 1, 0, V - 1])
    _, ref = orc.forward(x, labels)
    dec_in = torch.full_like(labels, g.decoder_start_token_id)
    dec_in[:, 1:] = labels[:, :-1]
    for mode in ("batched", "step"):
        monkeypatch.setenv("M2M_FORWARD", mode)
        out = model.logits_from_embeds(x.cuda(), dec_in.cuda()).cpu()
        assert out.shape == ref.shape
        err = (out - ref).abs().max().item()
        print(f"V={V} forced logits {mode}: max|diff| {err:.3e}")
        assert err < 2e-3, (mode, err)


@pytest.mark.parametrize("V", BF16_VOCABS)
def test_vocab_size_through_encode_and_greedy_bf16(V):
    check_greedy(V, "bf16")
    model, orc, g, _ = build_geom(geom_config(V), "bf16")
    x = embeds(3, 19, g.d_model)
    assert (model.encode(x.cuda()).cpu() - orc.encode(x)).abs().max().item() < 0.08


@pytest.mark.parametrize("V", sorted(DUPS))
def test_exact_ties_go_to_the_lower_index(V):
    check_greedy(V, "fp32", DUPS[V])


TOKEN_IDS = dict(pad_token_id=7, eos_token_id=512, decoder_start_token_id=511)

_CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_geometry_axes_gpu as t
for V in t.VOCABS:
    t.check_greedy(V, "fp32")
for V in t.BF16_VOCABS:
    t.check_greedy(V, "bf16")
for V, d in t.DUPS.items():
    t.check_greedy(V, "fp32", d)
t.check_greedy(513, "fp32", ids=t.TOKEN_IDS)
print("CHILD OK")
""" % (str(ROOT), str(ROOT / "tests"))


def test_vocab_size_through_the_head_kernel():
    """M2M_HEADLESS=0 (latched when a session is created; set for a child process) decodes every case above through dec_head_kernel: the register batch of 512
    columns and the loop over the rest, its tie-break, the special ids."""
    env = dict(os.environ, M2M_HEADLESS="0", OMP_NUM_THREADS="8")
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "CHILD OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------------------------------------ 2. vocabulary, sampling head
SAMPLE_VOCABS = [17, 400, 511, 513, 1024, 1025, 2048, 2049, 4096]


@pytest.mark.parametrize("V", SAMPLE_VOCABS)
def test_sampling_head_across_the_vocabulary_bands(V):
    """every logits-per-lane band of dec_sample_kernel and its edges: top_k = 1 (and top_p = 0) is greedy, and every sampled
    token lies in the set the HF warpers keep, for k >= V, k = V - 1, T = 0.05 and T = 20 (the tied zero rows of the head put
    many k boundaries inside a group of exactly tied logits)"""
    model, orc, g, _ = build_geom(geom_config(V), "fp32", head=tail_head)
    B, S, L = 5, 19, 32
    x = embeds(B, S, g.d_model, seed=V % 89)
    greedy = model.generate_from_embeds(x.cuda(), max_length=L).cpu()
    assert torch.equal(_sample(model, x, L, 1, top_k=1, temperature=0.7), greedy)
    assert torch.equal(_sample(model, x, L, 2, top_k=0, top_p=0.0), greedy)
    settings = [(1.0, V, 1.0), (1.0, V + 7, 0.9), (1.0, V - 1, 1.0), (0.05, 5, 1.0), (20.0, 0, 1.0), (20.0, 3, 0.95), (3.0, 0, 0.6)]
    for seed, (T, k, p) in enumerate(settings):
        ids = _sample(model, x, L, 100 + seed, temperature=T, top_k=k, top_p=p)
        logits = _teacher_logits(orc, x, ids)
        n = L if p == 1.0 or V <= 1025 else 8            # (allowed_mask's nucleus is O(V^2) per position)
        ok = allowed_mask(logits[:, :n], T, k, p, 1e-4 / T, 1e-4)
        for b in range(B):
            row = ids[b].tolist()
            end = row.index(g.eos_token_id, 1) if g.eos_token_id in row[1:] else len(row) - 1
            for t in range(min(end, n)):
                assert ok[b, t, row[t + 1]], (V, T, k, p, b, t, row[t + 1])
            assert all(v == g.pad_token_id for v in row[end + 1:]), (b, row)


@pytest.mark.parametrize("V", [400, 1024, 2048, 4096])
def test_sampled_ids_are_the_same_from_every_select_kernel(V):
    """dec_sample_kernel, dec_process_kernel and dec_scored_kernel are one select body (decode.hip select_head): with the same
    seed and processors that cannot alter a row they emit the same ids, at one vocabulary in each logits-per-lane band, without
    warpers and with all three.  The legs: plain do_sample=True (dec_sample_kernel); output_logprobs=True (dec_scored_kernel with
    the neutral processor block); min_length=1 (dec_process_kernel: resolve_generate_kwargs takes any min_length > 0 as an active
    processor, and cur_len >= 1 never falls below it, so EOS is never banned).  Not yet run on a GPU, neither on this tree
    nor on the build before the fold (where it would prove that the three copies agreed): see DESIGN.md section 17."""
    model, _, g, _ = build_geom(geom_config(V), "fp32", head=tail_head)
    B, S, L = 5, 19, 32
    x = embeds(B, S, g.d_model, seed=V % 89).cuda()
    for seed, kw in enumerate([dict(temperature=1.0, top_k=0, top_p=1.0), dict(temperature=0.7, top_k=50, top_p=0.9)]):
        def ids(**more):
            torch.manual_seed(300 + seed)
            out = model.generate_from_embeds(x, max_length=L, do_sample=True, **kw, **more)
            return (out.sequences if more.get("return_dict_in_generate") else out).cpu()
        plain = ids()
        assert torch.equal(ids(return_dict_in_generate=True, output_logprobs=True), plain), (V, kw)
        assert torch.equal(ids(min_length=1), plain), (V, kw)


def first_step_head(sd, geom, orc_cls, x1, targets):
    """lm_head whose first-step logits are `targets` {row: logit} (every other row 0): the oracle's first-step hidden state h is
    read through an identity head, then row r = targets[r] * h / |h|^2 (the head does not feed back into that step)"""
    w = sd["transformer.lm_head.weight"]
    d = geom.d_model
    w[:] = 0.0
    w[:d] = np.eye(d, dtype=np.float32)
    h = _teacher_logits(orc_cls(geom, sd), x1, torch.zeros((1, 1), dtype=torch.long))[0, 0, :d].double()
    w[:] = 0.0
    for r, v in targets.items():
        w[r] = (v * h / h.dot(h)).float().numpy()


def build_first_step(V, targets_of):
    from oracle.t5 import T5Oracle
    cfg = geom_config(V)
    geom = T5Geometry(load_config(cfg).model.t5)
    sd = synth.t5_state_dict(geom, seed=0)
    synth.perturb_layer_norms(sd, 0)
    x1 = embeds(1, 8, geom.d_model, seed=13)
    first_step_head(sd, geom, T5Oracle, x1, targets_of(V))
    model = T5Transformer(cfg, precision="fp32")
    load_t5_state(model, sd, strict=False)
    orc = T5Oracle(geom, sd)
    return model.cuda().eval(), orc, geom, x1


def tail_targets(V):
    """V - 1 carries 0.55 of the mass, eleven rows spread over [V / 2, V - 2] the rest, no two alike (an exact tie at the nucleus
    boundary is kept whole by the device, cut in sort order by HF); for V > 4096 / 2 they all sit at or above 2048; the zero rows
    are e^-16 below"""
    rows = np.linspace(V // 2, V - 2, 11).astype(int).tolist()
    w = np.arange(1, 12, dtype=np.float64)
    p = {V - 1: 0.55, **{r: 0.45 * float(wi / w.sum()) for r, wi in zip(rows, w)}}
    return {r: 16.0 + math.log(v) for r, v in p.items()}


@pytest.mark.parametrize("V,T,k,p", [(513, 1.0, 8, 1.0), (2049, 1.0, 0, 1.0), (4096, 1.3, 0, 0.9)])
def test_sampled_distribution_reaches_the_top_of_the_vocabulary(V, T, k, p):
    """2048 first-step draws (256 rows x 8 seeds) against the warped softmax (assert_draws_follow: the L1 bound of
    test_sampled_distribution_matches_the_warped_softmax).  The mass sits on the top half of the vocabulary and V - 1: a lane or
    band that drops the tail cannot pass."""
    model, orc, g, x1 = build_first_step(V, tail_targets)
    logits = _teacher_logits(orc, x1, torch.zeros((1, 1), dtype=torch.long))[0, 0].double()
    probs = hf_warp(logits, T, k, p).double().softmax(-1)
    assert float(probs[V - 1]) > 0.3 and float(probs[V // 2:].sum()) > 0.99
    if V > 2048:
        assert float(probs[2048:].sum()) > 0.5
    draws = torch.cat([_sample(model, x1.repeat(256, 1, 1), 2, 1000 + s, temperature=T, top_k=k, top_p=p)[:, 1] for s in range(8)])
    l1 = assert_draws_follow(probs, draws)
    print(f"V={V}: L1 {l1:.4f}, P(V-1) {float(probs[V - 1]):.3f}, draws of V-1 {int((draws == V - 1).sum())}")


def test_top_k_boundary_inside_exactly_tied_logits_keeps_the_whole_tie():
    """HF's TopKLogitsWarper removes only what is strictly below the k-th largest: with four exactly tied rows on top (duplicate
    rows across the 32-lane groups, the register batch and the last lane) and top_k = 2, all four are drawn and nothing else"""
    tie = [100, 511, 512, 1024]

    def targets(V):
        return {**{r: 12.0 for r in tie}, 3: 11.0, 700: 10.0, 900: 9.0}

    model, orc, g, x1 = build_first_step(1025, targets)          # equal targets: bit-identical rows
    draws = torch.cat([_sample(model, x1.repeat(256, 1, 1), 2, 50 + s, top_k=2)[:, 1] for s in range(2)])
    assert set(draws.tolist()) == set(tie), sorted(set(draws.tolist()))


def test_sampling_refuses_a_vocabulary_beyond_the_sampling_head():
    """V = 4097 is past dec_sample_kernel's register row: m2m_generate_sample refuses it before launching anything (greedy decoding
    at 4097 is held to the oracle above)"""
    model, _, g, _ = build_geom(geom_config(4097), "fp32")
    x = embeds(2, 12, g.d_model).cuda()
    with pytest.raises(native.NativeError, match="vocab_size 4097"):
        model.generate_from_embeds(x, max_length=8, do_sample=True, top_k=5)
    lib = native.load()
    sess, _ = model._encode(x, 8)
    tokens = torch.full((2, 8), -5, dtype=torch.long, device=x.device)
    n = C.c_int(-1)
    sp = native.SampleParams(1.0, 5, 1.0, 1)
    assert lib.m2m_generate_sample(sess, 8, C.byref(sp), tokens.data_ptr(), C.byref(n), native.stream_handle(x.device)) == M2M_ERR_INVALID
    assert b"vocab_size 4097" in lib.m2m_last_error()
    assert (tokens.cpu() == -5).all()
    ids = model.generate_from_embeds(x, max_length=8).cpu()          # the session still decodes greedily
    assert ids.shape[0] == 2


# --------------------------------------------------------------------------------------------------- 3. vocabulary, training
@pytest.mark.parametrize("V", [37, 333, 1001, 4097, 32128])
def test_vocab_size_through_the_training_step_fp32(V):
    """odd V and V % 8 != 0 (the logits row padded to 8, the non-vector transposes), labels over all of [0, V) incl. 0 and V - 1"""
    model, tr, orc, params, geom, x, feats, cond, labels = _setup(geom_config(V), "fp32", 3, 21, 14, label_range=(0, V))
    assert int(labels.max()) == V - 1 and int(labels[labels >= 0].min()) == 0
    check_fp32_step(tr, orc, x, feats, cond, labels, f"V={V}")


def test_odd_vocab_size_through_the_training_step_bf16():
    _, tr, orc, _, _, x, feats, cond, labels = _setup(geom_config(1001), "bf16", 4, 90, 48, label_range=(0, 1001))
    check_bf16_step(tr, orc, x, feats, cond, labels, "V=1001")


def test_odd_vocab_size_through_the_training_step_fp8():
    _, tr, orc, _, _, x, feats, cond, labels = _setup(geom_config(333), "fp8", 3, 21, 14, label_range=(0, 333))
    check_fp8_step(tr, orc, x, feats, cond, labels, "geometry")


# ------------------------------------------------------------------------------------------------------------- 4. token ids
def test_special_token_ids_away_from_0_2_1(monkeypatch):
    """pad 7, EOS V - 1, start V - 2 at V = 513: greedy (rows end on EOS and pad with 7 afterwards), forced logits, top_k = 1
    sampling, a training step"""
    ids_ref = check_greedy(513, "fp32", ids=TOKEN_IDS)
    assert (ids_ref[:, 0] == 511).all()
    padded = [r[r.tolist().index(512) + 1:] for r in ids_ref if 512 in r.tolist()[:-1]]
    assert padded and all((tail == 7).all() for tail in padded)          # a row ended early, and pads with 7
    cfg = geom_config(513, **TOKEN_IDS)
    model, orc, g, _ = build_geom(cfg, "fp32", head=tail_head)
    x = embeds(6, 19, g.d_model, seed=513 % 97)
    greedy = model.generate_from_embeds(x.cuda(), max_length=40).cpu()
    assert torch.equal(greedy, ids_ref)
    assert torch.equal(_sample(model, x, 40, 3, top_k=1), greedy)
    labels = greedy[:, 1:].clone()
    labels[labels == 7] = -100
    _, ref = orc.forward(x, labels)
    dec_in = greedy[:, :-1]
    for mode in ("batched", "step"):
        monkeypatch.setenv("M2M_FORWARD", mode)
        out = model.logits_from_embeds(x.cuda(), dec_in.cuda()).cpu()
        assert (out - ref).abs().max().item() < 2e-3, mode
    monkeypatch.delenv("M2M_FORWARD")
    model, tr, orc, params, geom, x, feats, cond, labels = _setup(cfg, "fp32", 3, 21, 14, label_range=(0, 513))
    check_fp32_step(tr, orc, x, feats, cond, labels, "special ids")


# ----------------------------------------------------------------------------------------------- 5. relative-position buckets
BUCKETS = [(4, 3), (8, 16), (32, 33), (128, 1024)]      # max_distance far below S ... above the longest S


@pytest.mark.parametrize("nb,md", BUCKETS)
def test_bucket_geometry_through_the_encoder(monkeypatch, nb, md):
    """S = 19, 300, 864: the bias table's constant far range (enc_bias_far) inside nearly every key tile, or nowhere; fp32 vs the
    oracle with M2M_ATTN_WIDE on and off (fp32 keeps its kernel: equal), the bf16 wide form vs the first form and the oracle"""
    cfg = geom_config(relative_attention_num_buckets=nb, relative_attention_max_distance=md)
    out = {}
    for prec in ("fp32", "bf16"):
        for wide in ("1", "0"):
            monkeypatch.setenv("M2M_ATTN_WIDE", wide)
            model, orc, g, _ = build_geom(cfg, prec)      # latched per session: a model per leg
            for B, S in ((3, 19), (3, 300), (2, 864)):
                x = embeds(B, S, g.d_model, seed=S)
                y = model.encode(x.cuda()).cpu()
                ref = orc.encode(x)
                err = (y - ref).abs().max().item()
                assert err < (2e-4 if prec == "fp32" else 0.08), (prec, wide, S, err)
                out[prec, wide, S] = y
            del model
    for S in (19, 300, 864):
        assert torch.equal(out["fp32", "1", S], out["fp32", "0", S])
        d = (out["bf16", "1", S] - out["bf16", "0", S]).double()
        assert float(d.norm() / out["bf16", "0", S].double().norm()) < 2e-2, S


@pytest.mark.parametrize("nb,md", BUCKETS)
def test_bucket_geometry_through_the_decoder(monkeypatch, nb, md):
    """forced logits (batched and step) up to L = 200 and greedy ids, fp32 vs the oracle"""
    cfg = geom_config(relative_attention_num_buckets=nb, relative_attention_max_distance=md)
    model, orc, g, _ = build_geom(cfg, "fp32")
    B, S, Ld = 2, 40, 200
    x = embeds(B, S, g.d_model, seed=nb)
    labels = torch.from_numpy((synth.uniform01(nb, "labels", B * Ld) * g.vocab_size).astype(np.int64).reshape(B, Ld))
    _, ref = orc.forward(x, labels)
    dec_in = torch.full_like(labels, g.decoder_start_token_id)
    dec_in[:, 1:] = labels[:, :-1]
    for mode in ("batched", "step"):
        monkeypatch.setenv("M2M_FORWARD", mode)
        err = (model.logits_from_embeds(x.cuda(), dec_in.cuda()).cpu() - ref).abs().max().item()
        assert err < 2e-3, (mode, err)
    monkeypatch.delenv("M2M_FORWARD")
    assert torch.equal(model.generate_from_embeds(x.cuda(), max_length=64).cpu(), orc.generate(x, 64))


def test_bucket_geometry_bf16():
    model, orc, g, _ = build_geom(geom_config(relative_attention_num_buckets=8, relative_attention_max_distance=16), "bf16")
    x = embeds(3, 300, g.d_model)
    assert (model.encode(x.cuda()).cpu() - orc.encode(x)).abs().max().item() < 0.08
    ref, margins = orc.generate(x, 40, return_margins=True)
    assert_bf16_ids_track(model.generate_from_embeds(x.cuda(), max_length=40).cpu(), ref, margins)


@pytest.mark.parametrize("nb,md", [(4, 3), (128, 1024)])
def test_bucket_geometry_through_the_training_step(nb, md):
    """both relative_attention_bias gradients (bias_bucket_kernel's grid is num_buckets x heads) and every other one"""
    cfg = geom_config(relative_attention_num_buckets=nb, relative_attention_max_distance=md)
    model, tr, orc, params, geom, x, feats, cond, labels = _setup(cfg, "fp32", 2, 300, 40)
    check_fp32_step(tr, orc, x, feats, cond, labels, f"buckets {nb}/{md}")


# ------------------------------------------------------------------------------------------------------------ 6. trainer widths
@pytest.mark.parametrize("d_model,d_ff,heads,F", [(192, 200, 3, 530), (256, 520, 4, 70), (320, 1000, 5, 70), (448, 1152, 7, 70),
                                                  (512, 2048, 8, 70)])
def test_trainer_widths_fp32(d_model, d_ff, heads, F):
    """d_model a multiple of 64 but not of 128, d_ff not a multiple of 64, odd head counts (inner 192 / 320 / 448); F = 530 runs
    the non-fused attention path"""
    cfg = geom_config(d_model=d_model, d_ff=d_ff, num_heads=heads)
    model, tr, orc, params, geom, x, feats, cond, labels = _setup(cfg, "fp32", 3, F, 33)
    check_fp32_step(tr, orc, x, feats, cond, labels, f"d={d_model} ff={d_ff} H={heads}")


def test_trainer_width_bf16():
    cfg = geom_config(d_model=320, d_ff=1000, num_heads=5)
    _, tr, orc, _, _, x, feats, cond, labels = _setup(cfg, "bf16", 4, 90, 48)
    check_bf16_step(tr, orc, x, feats, cond, labels, "d=320 ff=1000 H=5")


@pytest.mark.parametrize("d_model,d_ff,heads,floors", [(256, 512, 4, "tiny"), (512, 1152, 2, "geometry")])
def test_trainer_widths_fp8(d_model, d_ff, heads, floors):
    cfg = geom_config(d_model=d_model, d_ff=d_ff, num_heads=heads)
    _, tr, orc, _, _, x, feats, cond, labels = _setup(cfg, "fp8", 3, 21, 14)
    check_fp8_step(tr, orc, x, feats, cond, labels, floors)
