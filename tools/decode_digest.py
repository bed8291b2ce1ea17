#!/usr/bin/env python3
"""SHA-256 over what the decode kernels produce, per kernel form: greedy ids and out length, the teacher-forced step logits
(M2M_FORWARD=step, first 24 positions), the scores of a scored decode, beam search; and the host paths around them: the encoder
states, the batched teacher-forced logits, a seeded sampled, a processed and a grammar decode, a processed beam search.  For changes
of decode.hip's device code or of the inference host (t5_api.hip) that must not move a bit: run once per build and compare the lines.

    M2M_LIBRARY=<the other build> python tools/decode_digest.py > a.txt;  python tools/decode_digest.py > b.txt;  diff a.txt b.txt

Weights and inputs are fixed; the bits depend on the ROCm build, so the digests are compared, never stored.  The decode switches
are latched when a session is created, so every leg sets its environment before it creates its model.

For changes of the encoder-side kernels (enc_gemm.hip, enc_attn.hip) run it a second time with
M2M_GEMM_SMALL_BELOW=0 M2M_NORM_GEMM=0 M2M_RESID_PANEL=0 M2M_ATTN_WIDE=0 set for the whole process: every product then takes
gemm_kernel's 128x128 tile and the bf16 attention takes attn_kernel, forms the default run does not launch."""
import copy
import hashlib
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402
from music2midi_amd import synth  # noqa: E402
from music2midi_amd.checkpoint import load_t5_state  # noqa: E402
from music2midi_amd.config import DEFAULT_CONFIG, T5Geometry, load_config  # noqa: E402
from music2midi_amd.transformer import T5Transformer  # noqa: E402

SWITCHES = ("M2M_DA_CLIPS", "M2M_DEC_FF_ROWS", "M2M_DEC_FF_SLICES", "M2M_HEADLESS", "M2M_FORWARD")
B, S, L = 13, 40, 64
LEGS = [("1", "8", "1"), ("2", "16", "2"), ("4", "8", "4"), ("4", "16", "1")]       # (M2M_DA_CLIPS, M2M_DEC_FF_ROWS, M2M_DEC_FF_SLICES)


def embeds(B, S, d, seed):
    """encoder inputs [B, S, d] from the seed (the suite's inputs: normal, scale 3)"""
    return torch.from_numpy(synth.normal(seed, "embeds", (B, S, d), 3.0))


def sha(*tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def model_for(cfg, sd, precision, env):
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    m = T5Transformer(cfg, precision=precision)
    load_t5_state(m, sd, strict=False)
    return m.cuda().eval()


def greedy_case(name, cfg, sd, precision, x, env):
    """ids + out length, step logits along those ids, the scores of the same decode"""
    m = model_for(cfg, sd, precision, env)
    ids = m.generate_from_embeds(x, max_length=L)
    out = m.generate_from_embeds(x, max_length=L, return_dict_in_generate=True, output_scores=True)
    os.environ["M2M_FORWARD"] = "step"
    logits = m.logits_from_embeds(x, ids[:, : min(24, ids.shape[1])])
    os.environ.pop("M2M_FORWARD")
    what = " ".join(f"{k}={v}" for k, v in env.items())
    print(f"{name} {precision} {what}: out_len {ids.shape[1]} ids {sha(ids)} step logits {sha(logits)} "
          f"scored ids {sha(out.sequences)} scores {sha(*out.scores)}", flush=True)
    del m


def host_paths_case(cfg, sd, precision, x):
    """the host paths around the decode step: encoder states, the batched teacher-forced pass, and the calls that reach the kernels
    through a parameter block (sampled, processed, grammar, processed beam search); default switches"""
    m = model_for(cfg, sd, precision, {})
    print(f"encode {precision}: states {sha(m.encode(x))}", flush=True)
    ids = m.generate_from_embeds(x, max_length=L)
    print(f"batched logits {precision}: {sha(m.logits_from_embeds(x, ids))}", flush=True)
    torch.manual_seed(7)
    ids = m.generate_from_embeds(x, max_length=L, do_sample=True, temperature=0.9, top_k=50, top_p=0.9)
    print(f"sampled {precision}: out_len {ids.shape[1]} ids {sha(ids)}", flush=True)
    ids = m.generate_from_embeds(x, max_length=L, repetition_penalty=1.3, no_repeat_ngram_size=3, suppress_tokens=[5, 17, 140])
    print(f"processed {precision}: out_len {ids.shape[1]} ids {sha(ids)}", flush=True)
    ids = m.generate_from_embeds(x, max_length=L, midi_grammar=True)
    print(f"midi_grammar {precision}: out_len {ids.shape[1]} ids {sha(ids)}", flush=True)
    ids, scores = m.beam_search_processed_from_embeds(x[:5], 2, max_length=L, return_scores=True, midi_grammar=True, min_length=8,
                                                      suppress_tokens=[5, 17, 140])   # 2 beams on 5 clips
    print(f"processed beam {precision}: out_len {ids.shape[1]} ids {sha(ids)} sequence scores {sha(scores)}", flush=True)
    del m


def main():
    cfg = DEFAULT_CONFIG
    geom = T5Geometry(load_config(cfg).model.t5)
    sd = synth.t5_state_dict(geom, seed=0)
    synth.perturb_layer_norms(sd, 0)
    synth.force_eos_head(sd, geom, active=340, eos_scale=1.6)          # rows end raggedly
    x = embeds(B, S, geom.d_model, seed=33).cuda()
    for precision in ("fp32", "bf16"):
        for clips, rows, slices in LEGS:
            greedy_case("default", cfg, sd, precision, x, {"M2M_DA_CLIPS": clips, "M2M_DEC_FF_ROWS": rows, "M2M_DEC_FF_SLICES": slices})
        greedy_case("default", cfg, sd, precision, x,
                    {"M2M_DA_CLIPS": "1", "M2M_DEC_FF_ROWS": "8", "M2M_DEC_FF_SLICES": "1", "M2M_HEADLESS": "0"})
        for clips in ("1", "2"):                                        # 2 beams on 5 clips
            m = model_for(cfg, sd, precision, {"M2M_DA_CLIPS": clips})
            ids, scores = m.beam_search_from_embeds(x[:5], 2, max_length=L, return_scores=True)
            print(f"beam {precision} M2M_DA_CLIPS={clips}: out_len {ids.shape[1]} ids {sha(ids)} sequence scores {sha(scores)}", flush=True)
            del m
        host_paths_case(cfg, sd, precision, x)
    # another width: d_model 128 (two waves per feed-forward workgroup, one wave per attention row)
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["model"]["t5"].update(d_model=128, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2)
    geom = T5Geometry(load_config(cfg).model.t5)
    sd = synth.t5_state_dict(geom, seed=3)
    synth.perturb_layer_norms(sd, 3)
    synth.force_eos_head(sd, geom)
    x = embeds(B, S, geom.d_model, seed=41).cuda()
    for precision in ("fp32", "bf16"):
        for clips, rows, slices in (("1", "8", "1"), ("2", "8", "2")):
            greedy_case("d_model=128", cfg, sd, precision, x, {"M2M_DA_CLIPS": clips, "M2M_DEC_FF_ROWS": rows, "M2M_DEC_FF_SLICES": slices})


if __name__ == "__main__":
    main()
