"""CPU: the oracle reproduces the golden vectors (which HuggingFace T5 / torch.stft produced
in the build container, tests/golden/make_golden.py).  This is what pins the oracle.

Three of the bars below (1e-5 on the fp32 log-mel, 1e-3 on the bf16 emulation's logits and margins) hold only where the host
CPU's fp32 arithmetic is the fixture machine's bit for bit: the BLAS / FFT libraries pick their kernels, and so their summation
orders, by CPU model, and the fixtures' own fp32 log-mel misses the float64 value of the same formula by 1.6e-5.  Whether a host
has that arithmetic is decided once, independently of the code under test: the fp32 oracle must reproduce the fixture's fp32
step-0 logits (t5_forced.npz ``full_s864_fp32``, which the fp32 oracle wrote) bit for bit.  Where it does, the bars are the
ones above; where it does not, each test holds the oracle to what a different summation order of the same formula leaves: the
fp32 log-mel to 1e-5 beyond this host's own fp32 rounding error (its distance to the float64 evaluation), the bf16 emulation to
its own noise floor stored in the fixture (tests/forced_check.py: the bars the device is held to)."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from music2midi_amd import synth
from music2midi_amd.config import DEFAULT_CONFIG, T5Geometry
from oracle.logmel import LogMelOracle, melscale_fbanks
from oracle.t5 import T5Oracle

from forced_check import BF16_FLOOR_FACTORS, bf16_margin_threshold
from test_t5_gpu import embeds, tiny_config


@lru_cache(maxsize=None)
def fixture_arithmetic(golden_dir) -> bool:
    """True when this host's fp32 oracle reproduces the fixture machine's fp32 step-0 logits of full_s864 bit for bit."""
    z = np.load(golden_dir / "t5_forced.npz")
    geom = T5Geometry(DEFAULT_CONFIG["model"]["t5"])
    sd = synth.t5_state_dict(geom, seed=0)
    synth.perturb_layer_norms(sd, 0)
    got = []
    T5Oracle(geom, sd).generate(embeds(2, 864, geom.d_model), 2, logits_hook=lambda t, lg: got.append(lg.clone()))
    return bool(np.array_equal(got[0].numpy(), z["full_s864_fp32/full_logits"][:, 0]))


def _case(golden_dir, name):
    z = np.load(golden_dir / "t5.npz")
    return {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")}


def _oracle(name, eos):
    cfg = tiny_config() if name.startswith("tiny") else DEFAULT_CONFIG
    geom = T5Geometry(cfg["model"]["t5"])
    sd = synth.t5_state_dict(geom, seed=0)
    synth.perturb_layer_norms(sd, 0)
    if eos:
        synth.force_eos_head(sd, geom)
    return T5Oracle(geom, sd), geom


@pytest.mark.parametrize("name", ["tiny", "tiny_eos", "full_s190", "full_eos"])
def test_t5_oracle_matches_hf_goldens(golden_dir, name):
    c = _case(golden_dir, name)
    B, S, L, Ld, eos = [int(v) for v in c["meta"]]
    orc, g = _oracle(name, bool(eos))
    x = embeds(B, S, g.d_model)
    enc = orc.encode(x)
    rows = c["enc_rows"].tolist()
    assert np.abs(enc[:, rows].numpy() - c["enc_sample"]).max() < 1e-4
    assert abs(enc.double().abs().sum().item() - float(c["enc_abs_sum"])) / float(c["enc_abs_sum"]) < 1e-5
    ids = orc.generate(x, L, enc_out=enc)
    assert ids.shape == c["ids"].shape and np.array_equal(ids.numpy(), c["ids"].astype(np.int64))
    labels = torch.from_numpy(c["labels"].astype(np.int64))
    loss, logits = orc.forward(x, labels, enc_out=enc)
    assert abs(loss.item() - float(c["loss"])) < 1e-4
    assert np.abs(logits[:, :: max(1, Ld // 4)].numpy() - c["logits_sample"]).max() < 2e-3


def test_t5_golden_covers_eos_pad_and_max_length(golden_dir):
    """The fixtures pin the three stopping behaviours (hf generation/utils.py:2929-2937)."""
    eos = _case(golden_dir, "tiny_eos")["ids"]
    assert (eos[:, 0] == 1).all()
    r, c = np.nonzero(eos == 2)
    assert len(r) >= 2 and len(set(c.tolist())) >= 1
    for row, col in zip(r, c):                       # pad after EOS
        assert (eos[row, col + 1:] == 0).all()
    full = _case(golden_dir, "full_s864")["ids"]
    # max_length truncation: the batch runs to exactly 1024 columns because a row never emits EOS
    assert full.shape == (2, 1024) and any(not (row == 2).any() for row in full)


def test_frontend_oracle_matches_goldens(golden_dir):
    z = np.load(golden_dir / "frontend.npz")
    fb = melscale_fbanks(1025, 20.0, 8000.0, 384, 16000).numpy()
    assert tuple(z["fb_shape"]) == fb.shape
    dense = np.zeros(fb.shape, dtype=np.float32)
    dense[z["fb_rows"], z["fb_cols"]] = z["fb_vals"]
    assert np.array_equal(dense, fb) and len(z["fb_vals"]) == 2034
    orc = LogMelOracle(16000, 2048, 256, 20.0, 384)
    for kind in ("noise", "tones", "zeros"):
        out = orc(torch.from_numpy(synth.waveform_batch(0, 2, 4096, kind))).numpy()
        assert out.shape == (2, 17, 384)
        tol = 1e-5 if kind != "tones" else 5e-2   # "tones": fp32 STFT noise floor, see test_frontend_gpu.py
        if kind != "tones" and not fixture_arithmetic(golden_dir):     # other fp32 summation orders: this host's own fp32 error on top
            wav = torch.from_numpy(synth.waveform_batch(0, 2, 4096, kind))
            tol += float(np.abs(out - orc(wav, dtype=torch.float64).numpy()).max())
        assert np.abs(out - z[f"logmel_{kind}"]).max() <= tol
    assert np.all(z["logmel_zeros"] == np.float32(np.log(np.float32(1e-6))))


def test_bf16_emulation_rounds_weights_and_caches():
    geom = T5Geometry(tiny_config()["model"]["t5"])
    sd = synth.t5_state_dict(geom, seed=0)
    o32, o16 = T5Oracle(geom, sd), T5Oracle(geom, sd, emulate="bf16")
    k = "encoder.block.0.layer.0.SelfAttention.q.weight"
    assert torch.equal(o16.w[k], o32.w[k].bfloat16().float()) and not torch.equal(o16.w[k], o32.w[k])
    assert torch.equal(o16.w["shared.weight"], o32.w["shared.weight"])       # residual stream stays fp32
    x = embeds(2, 9, geom.d_model)
    d = (o16.encode(x) - o32.encode(x)).abs().max().item()
    assert 1e-4 < d < 0.2


def test_training_oracle_reproduces_huggingface_golden(golden_dir):
    """oracle/train.py (differentiable forward + restated Adafactor) vs the fixture made by HF T5 autograd and
    transformers.optimization.Adafactor(warmup_init=True): losses of 3 steps, gradients of step 0, parameters after step 3."""
    from music2midi_amd import synth
    from music2midi_amd.config import DEFAULT_CONFIG, T5Geometry
    from oracle.train import AdafactorOracle, T5TrainOracle, leaf_params
    import copy
    z = np.load(golden_dir / "train.npz")
    B, F, Ld = [int(v) for v in z["meta"]]
    t5 = copy.deepcopy(DEFAULT_CONFIG["model"]["t5"])
    t5.update(d_model=128, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2)
    geom = T5Geometry(t5)
    sd = synth.t5_state_dict(geom, seed=0)
    synth.perturb_layer_norms(sd, 0)
    params = leaf_params(sd)
    orc, opt = T5TrainOracle(geom, params), AdafactorOracle(params)
    feats = torch.from_numpy(synth.normal(5, "feats", (B, F, geom.d_model), 2.0))
    cond = torch.from_numpy(synth.cond_index_batch(2, B))
    labels = torch.from_numpy(z["labels"].astype(np.int64))
    keys = [str(k) for k in z["keys"]]
    for step in range(3):
        loss, logits, grads = orc.loss_and_grads(feats, cond, labels)
        assert abs(loss.item() - z["losses"][step]) < 2e-5
        if step == 0:
            assert np.abs(logits.numpy()[:, ::4] - z["logits_sample"]).max() < 2e-3
            for i, k in enumerate(keys):
                assert abs(grads[k].double().norm().item() - z["grad_l2"][i]) <= 1e-4 * z["grad_l2"][i] + 1e-10, k
        opt.step(grads)
    for i, k in enumerate(keys):
        assert abs(params[k].detach().double().abs().sum().item() - z["param_abs_sum_after3"][i]) <= 1e-6 * z["param_abs_sum_after3"][i], k


def test_bf16_emulating_oracle_reproduces_its_headline_fixture_prefix(golden_dir):
    """tests/golden/t5_bf16.npz (the bf16 mode's pin at S = 864): the oracle regenerates the first 24 tokens and margins of the
    committed 1024 (the whole run takes ~40 s; `make_golden.py t5_bf16` regenerates all of it), and the fixture's fp32 twin is the
    HF-pinned full_s864 case."""
    z = np.load(golden_dir / "t5_bf16.npz")
    geom = T5Geometry(DEFAULT_CONFIG["model"]["t5"])
    sd = synth.t5_state_dict(geom, seed=0)
    synth.perturb_layer_norms(sd, 0)
    x = embeds(2, 864, geom.d_model)
    ids, margins = T5Oracle(geom, sd, emulate="bf16").generate(x, 24, return_margins=True)
    want = z["full_s864_bf16/ids"].astype(np.int64)
    assert want.shape == (2, 1024) and z["full_s864_bf16/margins"].shape == (2, 1023)
    if fixture_arithmetic(golden_dir):
        assert np.array_equal(ids.numpy(), want[:, :24])
        assert np.abs(margins.numpy() - z["full_s864_bf16/margins"][:, :23]).max() < 1e-3
    else:       # the emulation's own noise floor: same ids up to the first position whose margin is under the arg-max threshold
        zf = np.load(golden_dir / "t5_forced.npz")
        fm = z["full_s864_bf16/margins"][:, :23]
        for b in range(2):
            close = np.flatnonzero(fm[b] <= bf16_margin_threshold(zf, "full_s864_bf16"))
            n = 1 + (int(close[0]) if len(close) else 23)
            assert np.array_equal(ids.numpy()[b, :n], want[b, :n]), b
            m = min(n, 23)        # margins of the steps whose inputs are the same ids
            assert np.abs(margins.numpy()[b, :m] - fm[b, :m]).max() <= BF16_FLOOR_FACTORS[0] * float(zf["full_s864_bf16/self_noise_margin"][0])
    assert z["bench_clips_bf16/ids"].shape == z["bench_clips_fp32/ids"].shape == (2, 1024)
    assert (z["bench_clips_bf16/ids"][:, 0] == 1).all() and z["bench_clips_bf16/margins"].min() > 0


def test_forced_fixture_is_what_the_oracle_computes(golden_dir):
    """tests/golden/t5_forced.npz (every position of the headline sequence, both precision modes): structure, consistency with the
    older fixtures (same ids: t5.npz is HF's own output, t5_bf16.npz the emulation's), and the first 8 steps regenerated — top-4
    logits and the full step-0 logits — for the bf16 emulation (`make_golden.py t5_forced` regenerates all of it in ~1 min)."""
    z, zb, z32 = (np.load(golden_dir / f) for f in ("t5_forced.npz", "t5_bf16.npz", "t5.npz"))
    for case in ("full_s864_fp32", "full_s864_bf16", "bench_clips_fp32", "bench_clips_bf16"):
        assert z[f"{case}/ids"].shape == (2, 1024) and z[f"{case}/margins"].shape == (2, 1023)
        assert z[f"{case}/top_vals"].shape == (2, 1023, 4) and z[f"{case}/top_idx"].shape == (2, 1023, 4)
        n = len(z[f"{case}/full_steps"])
        assert z[f"{case}/full_logits"].shape == (2, n, 400) and z[f"{case}/full_steps"][0] == 0 and z[f"{case}/full_steps"][-1] == 1022
        tv = z[f"{case}/top_vals"]
        nxt, am = z[f"{case}/ids"][:, 1:], z[f"{case}/top_idx"][:, :, 0]
        live = np.cumsum(np.concatenate([np.zeros((2, 1), bool), nxt[:, :-1] == 2], axis=1), axis=1) == 0    # up to and including a row's EOS
        assert np.array_equal(am[live], nxt[live]) and (nxt[~live] == 0).all()     # greedy: the top column IS the next id; pad after EOS
        assert np.allclose(tv[:, :, 0] - tv[:, :, 1], z[f"{case}/margins"], atol=1e-5) and (np.diff(tv, axis=2) <= 0).all()
    assert np.array_equal(z["full_s864_fp32/ids"], z32["full_s864/ids"]) and np.array_equal(z["full_s864_bf16/ids"], zb["full_s864_bf16/ids"])
    assert np.array_equal(z["bench_clips_fp32/ids"], zb["bench_clips_fp32/ids"]) and np.array_equal(z["bench_clips_bf16/ids"], zb["bench_clips_bf16/ids"])
    geom = T5Geometry(DEFAULT_CONFIG["model"]["t5"])
    sd = synth.t5_state_dict(geom, seed=0)
    synth.perturb_layer_norms(sd, 0)
    got = []
    T5Oracle(geom, sd, emulate="bf16").generate(embeds(2, 864, geom.d_model), 9, logits_hook=lambda t, lg: got.append(lg.clone()))
    got = torch.stack(got, 1).numpy()
    # other fp32 summation orders: the emulation's own noise floor (max |d logit|, median over the perturbation seeds) x 1.5
    tol = 1e-3 if fixture_arithmetic(golden_dir) else BF16_FLOOR_FACTORS[0] * float(z["full_s864_bf16/self_noise_logit"][0])
    assert np.abs(np.take_along_axis(got, z["full_s864_bf16/top_idx"][:, :8].astype(np.int64), 2) - z["full_s864_bf16/top_vals"][:, :8]).max() < tol
    assert np.abs(got[:, 0] - z["full_s864_bf16/full_logits"][:, 0]).max() < tol
