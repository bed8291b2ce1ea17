"""The decode feed-forward and lm_head kernels stage the residual rows of their MFMA tile through LDS (decode.hip, row_stage_at):
whole-line cooperative loads of the block's real rows, then every lane reads back the 16 elements it used to read from memory.
Greedy ids and teacher-forced step logits against the oracle, on the smallest shapes where the staging can go wrong: a partial row
block (B = 1, 7), exactly one block (8), a block plus one row (9), a partial 16-row lm_head tile next to a full one (17), two
chains and a third row block (33); 8- and 16-row tiles, one and two hidden slices per workgroup, both lm_head instantiations
(the headless greedy step and the step with dec_head_kernel, which the teacher-forced pass always takes)."""
import numpy as np
import pytest
import torch

from music2midi_amd import synth
from music2midi_amd.checkpoint import load_t5_state
from music2midi_amd.config import DEFAULT_CONFIG, T5Geometry, load_config
from music2midi_amd.transformer import T5Transformer

pytestmark = pytest.mark.gpu

S, L = 8, 12
# (M2M_DEC_FF_ROWS, M2M_DEC_FF_SLICES, M2M_HEADLESS) beside the default ("0", "0", "1"), by batch size
EXTRA_LEGS = {1: [("0", "0", "0")], 7: [("0", "0", "0")], 8: [("16", "1", "1")], 9: [("8", "2", "1")], 17: [("16", "1", "1")],
              33: [("8", "2", "1"), ("16", "1", "0")]}


@pytest.fixture(scope="module")
def weights():
    geom = T5Geometry(load_config(DEFAULT_CONFIG).model.t5)
    sd = synth.t5_state_dict(geom, seed=0)
    synth.perturb_layer_norms(sd, 0)
    return geom, sd


@pytest.mark.parametrize("B", [1, 7, 8, 9, 17, 33])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_staged_rows_reproduce_the_oracle_in_every_tile_form(monkeypatch, weights, precision, B):
    from oracle.t5 import T5Oracle
    geom, sd = weights
    x = torch.from_numpy(synth.normal(41, "embeds", (B, S, geom.d_model), 3.0))
    labels = torch.from_numpy((synth.uniform01(5, "labels", B * L) * 330).astype(np.int64).reshape(B, L)) + 3
    dec_in = torch.full_like(labels, geom.decoder_start_token_id)
    dec_in[:, 1:] = labels[:, :-1]
    orc = T5Oracle(geom, sd, emulate=precision)
    ref_ids, margins = orc.generate(x, L, return_margins=True)
    _, ref_logits = orc.forward(x, labels)

    ids, logits = {}, {}
    base = ("0", "0", "1")
    for leg in [base] + EXTRA_LEGS[B]:
        rows, slices, headless = leg
        monkeypatch.setenv("M2M_DEC_FF_ROWS", rows)            # latched when the session is created: a new model per leg
        monkeypatch.setenv("M2M_DEC_FF_SLICES", slices)
        monkeypatch.setenv("M2M_HEADLESS", headless)
        m = T5Transformer(DEFAULT_CONFIG, precision=precision)
        load_t5_state(m, sd, strict=False)
        m = m.cuda().eval()
        if B in (9, 17):
            m._get_session(33, S, L)                           # a session sized above the batch it decodes (max_batch > B)
        monkeypatch.delenv("M2M_FORWARD", raising=False)
        ids[leg] = m.generate_from_embeds(x.cuda(), max_length=L).cpu()
        monkeypatch.setenv("M2M_FORWARD", "step")              # the same step kernels, teacher-forced
        logits[leg] = m.logits_from_embeds(x.cuda(), dec_in.cuda()).cpu()
        del m
    # every form computes a row with the same operations in the same order
    for leg in ids:
        assert torch.equal(ids[leg], ids[base]), f"ids differ with rows/slices/headless = {leg}"
        assert torch.equal(logits[leg], logits[base]), f"step logits differ with rows/slices/headless = {leg}"
    out, lg = ids[base], logits[base]
    err = (lg - ref_logits).abs().max().item()
    scale = ref_logits.abs().max().item()
    print(f"row staging {precision} B={B}: step logits max|diff| {err:.3e} on logits up to {scale:.1f}, min margin {margins.min().item():.4f}")
    if precision == "fp32":
        assert out.shape == ref_ids.shape and torch.equal(out, ref_ids)
        assert err < 2e-3
    else:
        # bf16 has 8 significant bits: the bars of test_forward_bf16_tracks_bf16_oracle / test_bf16_mode_tracks_bf16_oracle
        assert err < 0.03 * scale
        n = min(out.shape[1], ref_ids.shape[1])
        for b in range(B):
            for t in range(1, n):
                if out[b, t] != ref_ids[b, t]:
                    assert margins[b, t - 1] < 0.5, f"row {b} step {t}: diverged at margin {margins[b, t - 1]:.3f}"
                    break
