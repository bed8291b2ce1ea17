"""The decode feed-forward reads its weights from a step image written once in m2m_model_create (t5.h DecLayerPacked::ff_img,
repack.hip ff_image_kernel): wi and wo_ff permuted into the order dec_ff_body's fragment loads read them - hidden slice, wave,
the eight wi fragments, the four wo_ff fragments, 64 lanes x 16 bytes each.  Greedy ids and teacher-forced step logits against the
oracle: at the default geometry in every form of the kernel (8- and 16-row tiles, one, two and four hidden slices per workgroup, the
step with and without dec_head_kernel, two clips per attention workgroup), and at the smallest geometries where a wrong index map
shows: every reduction length the kernel is instantiated for (d_model 128 / 256 / 384 / 512 = 2 / 4 / 6 / 8 waves), two slices
(d_ff 64), six slices (d_ff 192: the XCD mapping wraps with a partial group of workgroups), four slices in one workgroup
(d_ff 128) and another head count.  A permuted or shifted image multiplies the rows with the wrong weights: the logits land far
outside either bar.

The decode attention kernels read their output projections from images too (DecLayerPacked::wo_img / wco_img: head, load
instruction, thread); every case above runs them (one and two clips per workgroup), and one beam-search call (two beams, three
clips) runs their BEAM instantiations against the restatement of tests/beam_ref.py, as tests/test_beam_gpu.py does."""
import numpy as np
import pytest
import torch

from music2midi_amd import synth
from music2midi_amd.checkpoint import load_t5_state
from music2midi_amd.config import DEFAULT_CONFIG, T5Geometry, load_config
from music2midi_amd.transformer import T5Transformer

from beam_ref import oracle_beam_search
from test_beam_gpu import _assert_ids_equal, _hyp_len
from test_geometry_axes_gpu import geom_config
from test_t5_gpu import build, embeds, tiny_config

pytestmark = pytest.mark.gpu

S, L = 8, 12
# (M2M_DEC_FF_ROWS, M2M_DEC_FF_SLICES, M2M_HEADLESS, M2M_DA_CLIPS)
BASE = ("0", "0", "1", "0")
FORMS = [("16", "1", "1", "0"), ("8", "2", "1", "0"), ("8", "4", "1", "0"), ("0", "0", "0", "0"), ("0", "0", "1", "2")]


def _weights(cfg):
    geom = T5Geometry(load_config(cfg).model.t5)
    sd = synth.t5_state_dict(geom, seed=0)
    synth.perturb_layer_norms(sd, 0)
    return geom, sd


@pytest.fixture(scope="module")
def default_weights():
    return _weights(DEFAULT_CONFIG)


def _check(monkeypatch, cfg, geom, sd, precision, B, legs, what):
    from oracle.t5 import T5Oracle
    x = torch.from_numpy(synth.normal(43, "embeds", (B, S, geom.d_model), 3.0))
    labels = torch.from_numpy((synth.uniform01(7, "labels", B * L) * 330).astype(np.int64).reshape(B, L)) + 3
    dec_in = torch.full_like(labels, geom.decoder_start_token_id)
    dec_in[:, 1:] = labels[:, :-1]
    orc = T5Oracle(geom, sd, emulate=precision)
    ref_ids, margins = orc.generate(x, L, return_margins=True)
    _, ref_logits = orc.forward(x, labels)

    ids, logits = {}, {}
    for leg in legs:
        rows, slices, headless, clips = leg
        monkeypatch.setenv("M2M_DEC_FF_ROWS", rows)            # latched when the session is created: a new model per leg
        monkeypatch.setenv("M2M_DEC_FF_SLICES", slices)
        monkeypatch.setenv("M2M_HEADLESS", headless)
        monkeypatch.setenv("M2M_DA_CLIPS", clips)
        m = T5Transformer(cfg, precision=precision)
        load_t5_state(m, sd, strict=False)
        m = m.cuda().eval()
        monkeypatch.delenv("M2M_FORWARD", raising=False)
        ids[leg] = m.generate_from_embeds(x.cuda(), max_length=L).cpu()
        monkeypatch.setenv("M2M_FORWARD", "step")              # the same step kernels, teacher-forced
        logits[leg] = m.logits_from_embeds(x.cuda(), dec_in.cuda()).cpu()
        del m
    base = legs[0]
    # every form computes a row with the same operations in the same order
    for leg in legs:
        assert torch.equal(ids[leg], ids[base]), f"{what}: ids differ with rows/slices/headless/clips = {leg}"
        assert torch.equal(logits[leg], logits[base]), f"{what}: step logits differ with rows/slices/headless/clips = {leg}"
    out, lg = ids[base], logits[base]
    err = (lg - ref_logits).abs().max().item()
    scale = ref_logits.abs().max().item()
    print(f"weight images {what} {precision} B={B}: step logits max|diff| {err:.3e} on logits up to {scale:.1f}, min margin {margins.min().item():.4f}")
    if precision == "fp32":
        assert out.shape == ref_ids.shape and torch.equal(out, ref_ids)
        assert err < 2e-3
    else:
        # bf16 has 8 significant bits: the bars of tests/test_dec_row_stage_gpu.py
        assert err < 0.03 * scale
        n = min(out.shape[1], ref_ids.shape[1])
        for b in range(B):
            for t in range(1, n):
                if out[b, t] != ref_ids[b, t]:
                    assert margins[b, t - 1] < 0.5, f"row {b} step {t}: diverged at margin {margins[b, t - 1]:.3f}"
                    break


@pytest.mark.parametrize("B", [1, 8, 9, 17])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_default_geometry_in_every_form_of_the_step(monkeypatch, default_weights, precision, B):
    geom, sd = default_weights
    _check(monkeypatch, DEFAULT_CONFIG, geom, sd, precision, B, [BASE] + FORMS, "default geometry")


# d_model, d_ff, heads, the one leg: the form whose index map the geometry exercises
MAPS = {
    "d128_ks2": (128, 256, 2, BASE),
    "d256_ks4": (256, 256, 2, BASE),
    "d512_ks8": (512, 256, 2, BASE),
    "dff64_two_slices": (128, 64, 2, BASE),
    "dff192_six_slices_xcd_wrap": (128, 192, 2, BASE),
    "dff128_four_slices_per_workgroup": (128, 128, 2, ("8", "4", "1", "0")),
    "four_heads": (256, 128, 4, BASE),
}


@pytest.mark.parametrize("case", sorted(MAPS))
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_image_index_map_at_the_small_geometries(monkeypatch, precision, case):
    d_model, d_ff, heads, leg = MAPS[case]
    cfg = geom_config(d_model=d_model, d_ff=d_ff, num_heads=heads)
    geom, sd = _weights(cfg)
    _check(monkeypatch, cfg, geom, sd, precision, 9, [leg], case)


def test_beam_search_reads_the_attention_images():
    # a case of tests/test_beam_gpu.py FP32_CASES (its input seed keeps the restatement's smallest decision gap above 1e-4), its bars
    B, S, nb, n, lp, es, L, seed = 3, 30, 2, 2, 1.0, "never", 40, 7
    model, orc, g = build(tiny_config(), "fp32", eos=True)
    x = embeds(B, S, g.d_model, seed=seed)
    want_ids, want_scores, gap = oracle_beam_search(orc, x, nb, L, lp, es, n)
    ids, scores = model.beam_search_from_embeds(x.cuda(), nb, max_length=L, length_penalty=lp, early_stopping=es,
                                                num_return_sequences=n, return_scores=True)
    ids, scores = ids.cpu(), scores.cpu()
    lens = torch.tensor([_hyp_len(r, g.eos_token_id) for r in ids], dtype=torch.float64)
    d_sum = (scores.double() - want_scores.double()).abs() * lens ** lp
    bar = 5e-5 * (want_scores.double().abs() * lens ** lp) + 5e-7 * lens
    print(f"weight images beam: ids {tuple(ids.shape)} min decision gap {gap:.3e} | sum err / bar max {(d_sum / bar).max():.2f}")
    assert gap > 1e-4, "a near-tie in the restatement: choose another case"
    _assert_ids_equal(ids, want_ids, g.eos_token_id)
    assert torch.all(d_sum <= bar)
