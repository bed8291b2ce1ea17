#!/usr/bin/env python3
"""Beam search under the MIDI token grammar against plain beam search, one GPU, bf16, random-init weights (synth seed 0).

    python tools/beam_grammar_bench.py [--reps 3] [--warmup 1] [--skip-ref]

Two workloads at max_length 1024: bench.py's default (32 clips x 10 s at 22.05 kHz) with num_beams = 4, and the reference's
inference chunk (128 segments of 3 s at 16 kHz) with num_beams = 2.  Three legs on the same encoder inputs, interleaved within
every repetition so that drift hits them alike:

    plain      T5Transformer.beam_search_from_embeds                     dec_beam_kernel<NPL>
    grammar    beam_search_processed_from_embeds(midi_grammar=True)      dec_beam_kernel<NPL, true>
    grammar+   ... with min_length=max_length as well                    the same kernel, the EOS ban active at every step

Random weights emit no EOS on their own, so the plain leg decodes every step: us per step = batch time / 1023.  Under the grammar
they do end: time ids only grow, a random model takes large jumps, and once the 200 time ids are used up EOS is the one id left,
so every clip is done after one to two hundred tokens.  The grammar+ leg bans EOS throughout (min_length = max_length; rows
left with no allowed id go on at -inf).  With num_beams = 2 it then decodes every step as the plain leg does (the -inf EOS of
beam 0 has rank 2 >= num_beams and is dropped) and its us per step = batch time / 1023 is the like-for-like figure; with
num_beams = 4 that EOS has rank 2 < num_beams, the -inf hypotheses fill the store and the clips still end.  A leg that returned
fewer than max_length columns is reported per returned column (batch time / (out_width - 1), "every_step_decoded": false): an
estimate, since the host notices a finished batch at its next poll, up to 63 steps late, and early steps read shorter caches.  Per leg the tool
reports every repetition (the spread is the yardstick for any difference) and their median.  The plain leg is the figure to
hold against tools/beam_bench.py run from a checkout of the parent commit.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import statistics
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


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def workload(model, B, n_samples, seed, nb, reps, warmup):
    wav = torch.from_numpy(synth.waveform_batch(seed, B, n_samples)).cuda()
    cond = torch.from_numpy(synth.cond_index_batch(seed, B)).cuda()
    x = model.encoder_inputs(ModelInputs(input_waveform=wav, cond_index=cond))
    legs = {
        "plain": lambda: model.beam_search_from_embeds(x, nb, max_length=MAX_LENGTH),
        "grammar": lambda: model.beam_search_processed_from_embeds(x, nb, max_length=MAX_LENGTH, midi_grammar=True),
        "grammar_min_length": lambda: model.beam_search_processed_from_embeds(x, nb, max_length=MAX_LENGTH, midi_grammar=True,
                                                                              min_length=MAX_LENGTH),
    }
    times = {k: [] for k in legs}
    width = {}
    for rep in range(warmup + reps):
        for name, fn in legs.items():                      # interleaved: one call of every leg per repetition
            t, ids = once(fn)
            if rep >= warmup:
                times[name].append(t)
                width[name] = int(ids.shape[1])
    out = {"clips": B, "num_beams": nb, "rows": B * nb, "S": int(x.shape[1])}
    for name, ts in times.items():
        steps = max(width[name] - 1, 1)
        out[name] = {"us_per_step": [t / steps * 1e6 for t in ts], "us_per_step_median": statistics.median(ts) / steps * 1e6,
                     "ms_per_batch_median": statistics.median(ts) * 1e3, "out_width": width[name], "steps_divided_by": steps,
                     "every_step_decoded": width[name] == MAX_LENGTH}
    base = out["plain"]["us_per_step_median"]
    if out["grammar_min_length"]["every_step_decoded"]:
        out["grammar_min_length_vs_plain"] = out["grammar_min_length"]["us_per_step_median"] / base
    return out


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
    out = {"metric": "beam search: plain vs token grammar vs grammar + min_length, bf16", "max_length": MAX_LENGTH, "reps": args.reps}
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
