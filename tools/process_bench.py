#!/usr/bin/env python3
"""Greedy decode against decode with logits processors (generate(repetition_penalty=..., ...)) on one GPU, bf16, random-init weights
(synth seed 0).

    python tools/process_bench.py [--reps 3] [--warmup 1] [--skip-ref]

Legs, timed interleaved rep by rep: greedy (the headless step), greedy with M2M_HEADLESS=0 (latched in the session's switches when it
is created: a child process per rep), processed greedy (repetition_penalty 1.2, no_repeat_ngram_size 4, min_length 64) and processed sampling (the same with
do_sample, temperature 1.0, top_k 50, top_p 0.9).  Workloads as tools/sample_bench.py: bench.py's default (32 clips x 10 s,
max_length 1024) and the reference's 128-segment chunk.  A leg's rows may end at other steps, so the like-for-like figure is the
time per decode step (batch time / decoded columns); the line also gives its ratio to headless greedy.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
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
from sample_bench import MAX_LENGTH, time_leg  # noqa: E402

PROC_KW = dict(repetition_penalty=1.2, no_repeat_ngram_size=4, min_length=64)
LEGS = {"greedy": {}, "processed_greedy": PROC_KW,
        "processed_sampled": dict(PROC_KW, do_sample=True, temperature=1.0, top_k=50, top_p=0.9)}


def build_model():
    geom = T5Geometry(load_config(DEFAULT_CONFIG).model.t5)
    model = T5Transformer(DEFAULT_CONFIG, precision="bf16")
    load_t5_state(model, synth.t5_state_dict(geom, seed=0), strict=False)
    return model.cuda().eval(), geom


def make_inputs(B, n_samples, seed):
    wav = torch.from_numpy(synth.waveform_batch(seed, B, n_samples)).cuda()
    cond = torch.from_numpy(synth.cond_index_batch(seed, B)).cuda()
    return ModelInputs(input_waveform=wav, cond_index=cond)


def child_leg(B, n_samples, seed, warmup):
    env = dict(os.environ, M2M_HEADLESS="0")
    cmd = [sys.executable, str(Path(__file__).resolve()), "--child", f"{B},{n_samples},{seed},{warmup}"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"M2M_HEADLESS=0 child failed ({r.returncode}): {r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def merge(runs):
    t = sum(r["ms_per_batch"] for r in runs) / len(runs)
    cols = sum(r["decoded_steps"] for r in runs) / len(runs)
    return {"ms_per_batch": t, "decoded_steps": cols, "us_per_step": t * 1e3 / cols,
            "tokens_per_s": sum(r["tokens_per_s"] for r in runs) / len(runs)}


def workload(model, eos, B, n_samples, seed, reps, warmup):
    inputs = make_inputs(B, n_samples, seed)
    runs = {k: [] for k in [*LEGS, "greedy_headless0"]}
    for _ in range(reps):
        for name, kw in LEGS.items():
            runs[name].append(time_leg(model, inputs, eos, 1, warmup, **kw))
        runs["greedy_headless0"].append(child_leg(B, n_samples, seed, warmup))
    out = {k: merge(v) for k, v in runs.items()}
    base = out["greedy"]["us_per_step"]
    for k in out:
        out[k]["vs_greedy_us_per_step"] = out[k]["us_per_step"] / base
        out[k]["vs_greedy_step_rate"] = base / out[k]["us_per_step"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--skip-ref", action="store_true", help="only bench.py's default workload")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    model, geom = build_model()
    if args.child:
        B, n, seed, warmup = (int(v) for v in args.child.split(","))
        print(json.dumps(time_leg(model, make_inputs(B, n, seed), geom.eos_token_id, 1, warmup)), flush=True)
        return
    cfg = load_config(DEFAULT_CONFIG)
    out = {"metric": "processed vs greedy decode, bf16", "processors": PROC_KW, "max_length": MAX_LENGTH, "reps": args.reps}
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
