#!/usr/bin/env python3
"""Beam search against greedy decoding on the same number of decoder rows, one GPU, bf16, random-init weights (synth seed 0).

    python tools/beam_bench.py [--reps 2] [--warmup 1] [--skip-ref]

Two workloads at max_length 1024: bench.py's default (32 clips x 10 s at 22.05 kHz) with num_beams = 4, and the reference's
inference chunk (128 segments of 3 s at 16 kHz) with num_beams = 2.  The beam leg encodes B clips and decodes B x nb rows; the
greedy leg decodes the same B x nb rows as B x nb encoded clips (each clip repeated nb times), so the two legs run the same
number of decoder rows per step and differ in the head, the ancestry reads of the self-attention and the cross K/V shared by a
clip's beams.  Random weights emit no EOS, so both legs decode every step: us per step = batch time / 1023 is the like-for-like
figure; tokens/s counts B x nb rows x steps for both.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from music2midi_amd import synth  # noqa: E402
from music2midi_amd.checkpoint import load_t5_state  # noqa: E402
from music2midi_amd.config import DEFAULT_CONFIG, T5Geometry, load_config  # noqa: E402
from music2midi_amd.input import ModelInputs  # noqa: E402
from music2midi_amd.transformer import T5Transformer  # noqa: E402

MAX_LENGTH = 1024


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out


def workload(model, B, n_samples, seed, nb, reps, warmup):
    wav = torch.from_numpy(synth.waveform_batch(seed, B, n_samples)).cuda()
    cond = torch.from_numpy(synth.cond_index_batch(seed, B)).cuda()
    x = model.encoder_inputs(ModelInputs(input_waveform=wav, cond_index=cond))
    xr = x.repeat_interleave(nb, 0).contiguous()
    tb, ids_b = timed(lambda: model.beam_search_from_embeds(x, nb, max_length=MAX_LENGTH), reps, warmup)
    tg, ids_g = timed(lambda: model.generate_from_embeds(xr, max_length=MAX_LENGTH), reps, warmup)
    steps_b, steps_g = MAX_LENGTH - 1, ids_g.shape[1] - 1
    rows = B * nb
    beam = {"ms_per_batch": tb * 1e3, "us_per_step": tb / steps_b * 1e6, "row_tokens_per_s": rows * steps_b / tb,
            "out_width": int(ids_b.shape[1])}
    greedy = {"ms_per_batch": tg * 1e3, "us_per_step": tg / steps_g * 1e6, "row_tokens_per_s": rows * steps_g / tg,
              "decoded_steps": steps_g}
    return {"clips": B, "num_beams": nb, "rows": rows, "S": int(x.shape[1]), "beam": beam, "greedy_same_rows": greedy,
            "beam_vs_greedy_us_per_step": beam["us_per_step"] / greedy["us_per_step"]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--skip-ref", action="store_true", help="only bench.py's default workload")
    args = ap.parse_args()
    cfg = load_config(DEFAULT_CONFIG)
    geom = T5Geometry(cfg.model.t5)
    model = T5Transformer(DEFAULT_CONFIG, precision="bf16")
    load_t5_state(model, synth.t5_state_dict(geom, seed=0), strict=False)
    model = model.cuda().eval()
    out = {"metric": "beam search vs greedy on B x nb rows, bf16", "max_length": MAX_LENGTH, "reps": args.reps}
    out["default"] = dict(workload(model, 32, 220500, 0, 4, args.reps, args.warmup),
                          workload_desc="32 clips x 10 s @ 22.05 kHz (bench.py default), num_beams 4")
    if not args.skip_ref:
        Tn = int(cfg.model.sample_rate * cfg.dataset.segment_duration)
        Bn = int(cfg.inference.batch_size)
        out["reference"] = dict(workload(model, Bn, Tn, 1000, 2, args.reps, args.warmup),
                                workload_desc=f"{Bn} segments x {Tn} samples (reference inference chunk), num_beams 2")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
