#!/usr/bin/env python3
"""Greedy decode against decode that also returns per-token scores (generate(return_dict_in_generate=True, output_scores /
output_logprobs)) on one GPU, random-init weights (synth seed 0).

    python tools/score_bench.py [--reps 3] [--warmup 1] [--precisions bf16,fp32] [--legs greedy,...]

Legs, timed interleaved rep by rep at bench.py's default workload (32 clips x 10 s, max_length 1024): plain greedy (the headless
step), greedy with logprobs only (4 bytes per token), greedy with scores (the V-wide fp32 row per token as well) and sampling
(temperature 1.0, top_k 50, top_p 0.9) with logprobs.  The scored legs run the non-headless step with the scored head.  Random-init
rows never emit EOS, so every leg decodes the same 1 023 columns; the figure is useful tokens per second and its ratio to plain
greedy.  `--legs greedy` needs nothing of the scored surface: it is the leg to run on an earlier commit for a same-box comparison.
Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import torch  # noqa: E402

from music2midi_amd import synth  # noqa: E402
from music2midi_amd.checkpoint import load_t5_state  # noqa: E402
from music2midi_amd.config import DEFAULT_CONFIG, T5Geometry, load_config  # noqa: E402
from music2midi_amd.input import ModelInputs  # noqa: E402
from music2midi_amd.transformer import T5Transformer  # noqa: E402
from sample_bench import MAX_LENGTH, useful_tokens  # noqa: E402

SAMPLE_KW = dict(do_sample=True, temperature=1.0, top_k=50, top_p=0.9)
LEGS = {"greedy": {},
        "greedy_logprobs": dict(return_dict_in_generate=True, output_logprobs=True),
        "greedy_scores": dict(return_dict_in_generate=True, output_scores=True),
        "sampled_logprobs": dict(SAMPLE_KW, return_dict_in_generate=True, output_logprobs=True)}


def build_model(precision):
    geom = T5Geometry(load_config(DEFAULT_CONFIG).model.t5)
    model = T5Transformer(DEFAULT_CONFIG, precision=precision)
    load_t5_state(model, synth.t5_state_dict(geom, seed=0), strict=False)
    return model.cuda().eval(), geom


def run_once(model, inputs, eos, seed, **kw):
    torch.manual_seed(seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = model.generate(inputs, max_length=MAX_LENGTH, **kw)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    toks = out if torch.is_tensor(out) else out.sequences
    return dt, useful_tokens(toks.cpu(), eos), toks.shape[1] - 1


def workload(model, eos, legs, reps, warmup):
    wav = torch.from_numpy(synth.waveform_batch(0, 32, 220500)).cuda()
    cond = torch.from_numpy(synth.cond_index_batch(0, 32)).cuda()
    inputs = ModelInputs(input_waveform=wav, cond_index=cond)
    for name in legs:
        for _ in range(warmup):
            run_once(model, inputs, eos, 0, **LEGS[name])
    runs = {name: [] for name in legs}
    for r in range(reps):
        for name in legs:
            runs[name].append(run_once(model, inputs, eos, r, **LEGS[name]))
    out = {}
    for name, v in runs.items():
        t, useful, cols = (sum(x[i] for x in v) for i in range(3))
        out[name] = {"ms_per_batch": t / len(v) * 1e3, "tokens_per_s": useful / t, "decoded_steps": cols / len(v),
                     "us_per_step": t / cols * 1e6, "ms_per_batch_runs": [round(x[0] * 1e3, 2) for x in v]}
    if "greedy" in out:
        for name in out:
            out[name]["vs_greedy_tokens_per_s"] = out[name]["tokens_per_s"] / out["greedy"]["tokens_per_s"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--precisions", default="bf16,fp32")
    ap.add_argument("--legs", default=",".join(LEGS))
    args = ap.parse_args()
    legs = [n for n in args.legs.split(",") if n]
    if any(n not in LEGS for n in legs):
        ap.error(f"--legs takes {sorted(LEGS)}")
    out = {"metric": "scored vs greedy decode", "workload": "32 clips x 10 s @ 22.05 kHz (bench.py default)",
           "max_length": MAX_LENGTH, "reps": args.reps, "sample_kw": SAMPLE_KW}
    for precision in args.precisions.split(","):
        model, geom = build_model(precision)
        out[precision] = workload(model, geom.eos_token_id, legs, args.reps, args.warmup)
        del model
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
