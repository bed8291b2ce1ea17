#!/usr/bin/env python3
"""Greedy against sampled generation (generate(do_sample=True)) on one GPU, bf16, random-init weights (synth seed 0).

    python tools/sample_bench.py [--reps 3] [--warmup 1] [--skip-ref]

Two workloads: bench.py's default (32 clips x 10 s at 22.05 kHz, max_length 1024) and the reference's inference geometry (one
inference.batch_size = 128 chunk of 3 s segments at 16 kHz, max_length 1024).  The sampled leg uses HF's defaults with a nucleus
(temperature 1.0, top_k 50, top_p 0.9).  A sampled row may draw EOS early, so the two legs can decode different numbers of steps:
the line reports both the useful tokens per second (per row up to and including its EOS) and the time per decode step (batch time /
decoded columns), which is the like-for-like figure.  Prints one JSON line.
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
SAMPLE_KW = dict(do_sample=True, temperature=1.0, top_k=50, top_p=0.9)


def useful_tokens(toks: torch.Tensor, eos: int) -> int:
    """generated tokens per row up to and including its first EOS (the whole row when it has none), summed"""
    gen = toks[:, 1:]
    hit = gen == eos
    first = torch.where(hit.any(1), hit.int().argmax(1) + 1, torch.full_like(hit[:, 0], gen.shape[1], dtype=torch.long))
    return int(first.sum())


def time_leg(model, inputs, eos, reps, warmup, **kw):
    for _ in range(warmup):
        model.generate(inputs, max_length=MAX_LENGTH, **kw)
    torch.cuda.synchronize()
    t_all, useful, cols = 0.0, 0, 0
    for r in range(reps):
        torch.manual_seed(r)
        t0 = time.perf_counter()
        toks = model.generate(inputs, max_length=MAX_LENGTH, **kw)
        torch.cuda.synchronize()
        t_all += time.perf_counter() - t0
        useful += useful_tokens(toks.cpu(), eos)
        cols += toks.shape[1] - 1
    return {"ms_per_batch": t_all / reps * 1e3, "tokens_per_s": useful / t_all, "decoded_steps": cols / reps,
            "us_per_step": t_all / cols * 1e6}


def workload(model, eos, B, n_samples, seed, reps, warmup):
    wav = torch.from_numpy(synth.waveform_batch(seed, B, n_samples)).cuda()
    cond = torch.from_numpy(synth.cond_index_batch(seed, B)).cuda()
    inputs = ModelInputs(input_waveform=wav, cond_index=cond)
    g = time_leg(model, inputs, eos, reps, warmup)
    s = time_leg(model, inputs, eos, reps, warmup, **SAMPLE_KW)
    return {"greedy": g, "sampled": s, "sampled_vs_greedy_tokens_per_s": s["tokens_per_s"] / g["tokens_per_s"],
            "sampled_vs_greedy_us_per_step": s["us_per_step"] / g["us_per_step"]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--skip-ref", action="store_true", help="only bench.py's default workload")
    args = ap.parse_args()
    cfg = load_config(DEFAULT_CONFIG)
    geom = T5Geometry(cfg.model.t5)
    model = T5Transformer(DEFAULT_CONFIG, precision="bf16")
    load_t5_state(model, synth.t5_state_dict(geom, seed=0), strict=False)
    model = model.cuda().eval()
    out = {"metric": "sampled vs greedy decode, bf16", "sample_kwargs": {k: v for k, v in SAMPLE_KW.items() if k != "do_sample"},
           "max_length": MAX_LENGTH, "reps": args.reps}
    out["default"] = dict(workload(model, geom.eos_token_id, 32, 220500, 0, args.reps, args.warmup),
                          workload_desc="32 clips x 10 s @ 22.05 kHz (bench.py default)")
    if not args.skip_ref:
        Tn = int(cfg.model.sample_rate * cfg.dataset.segment_duration)
        Bn = int(cfg.inference.batch_size)
        out["reference"] = dict(workload(model, geom.eos_token_id, Bn, Tn, 1000, args.reps, args.warmup),
                                workload_desc=f"{Bn} segments x {Tn} samples (reference inference chunk)")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
