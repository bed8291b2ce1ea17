#!/usr/bin/env python3
"""Cost of generate(midi_grammar=True) per decode step on one GPU, bf16, random-init weights (synth seed 0), against the PARENT
commit's build.

    python tools/grammar_bench.py --parent /path/to/parent/checkout [--reps 3] [--calls 5]

Legs: (a) headless greedy, (b) processed greedy with min_length only, (c) the same plus midi_grammar (this tree only).  Both
workloads of tools/process_bench.py (32 clips x 10 s, 128 segments x 3 s) with max_length = min_length = 128: min_length bans EOS
at every step, so no row finishes and every leg runs every step.  (A row of leg (c) CAN reach a state in which only EOS is allowed -
the last time id used and every note closed, six tokens suffice - and, EOS being banned, then emits id 0 and feeds PAD embeddings
for the rest of the call: the step count holds, the row's content no longer means anything.)  The yardstick for (c) is (b) on the
parent: the grammar adds no scan, so (c) should sit inside the spread of (b)'s own repetitions.

The parent's library lacks m2m_generate_grammar, so this tree's binding cannot load it through M2M_LIBRARY; ``--parent`` is a
checkout of the parent commit with its library built (``python -m music2midi_amd.csrc.build`` there), and its legs run this file in
a child process that imports the package from that checkout.  Parent and tree children alternate, rep by rep.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve()
MAX_LENGTH = 128
LEGS = {"a_greedy": {}, "b_min_length": dict(min_length=MAX_LENGTH), "c_min_length_grammar": dict(min_length=MAX_LENGTH, midi_grammar=True)}
WORKLOADS = {"default": (32, 220500, 0), "reference": (128, 48000, 1000)}     # clips, samples per clip, synth seed


def child(root: str, legs, calls: int):
    sys.path.insert(0, root)
    import torch
    from music2midi_amd import synth
    from music2midi_amd.checkpoint import load_t5_state
    from music2midi_amd.config import DEFAULT_CONFIG, T5Geometry, load_config
    from music2midi_amd.input import ModelInputs
    from music2midi_amd.transformer import T5Transformer

    geom = T5Geometry(load_config(DEFAULT_CONFIG).model.t5)
    model = T5Transformer(DEFAULT_CONFIG, precision="bf16")
    load_t5_state(model, synth.t5_state_dict(geom, seed=0), strict=False)
    model = model.cuda().eval()
    out = {}
    for wname, (B, n, seed) in WORKLOADS.items():
        inputs = ModelInputs(input_waveform=torch.from_numpy(synth.waveform_batch(seed, B, n)).cuda(),
                             cond_index=torch.from_numpy(synth.cond_index_batch(seed, B)).cuda())
        x = model.encoder_inputs(inputs)
        times = {leg: [] for leg in legs}
        for i in range(2 + calls):                                  # two warm-up rounds (graph capture), then the timed ones
            for leg in legs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                toks = model.generate_from_embeds(x, max_length=MAX_LENGTH, **LEGS[leg])
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if leg != "a_greedy":
                    assert toks.shape[1] == MAX_LENGTH, (leg, toks.shape)
                if i >= 2:
                    times[leg].append(dt * 1e6 / (toks.shape[1] - 1))
        out[wname] = {leg: statistics.mean(v) for leg, v in times.items()}
    print(json.dumps(out), flush=True)


def run_child(root, legs, calls):
    cmd = [sys.executable, str(HERE), "--child", str(root), "--legs", ",".join(legs), "--calls", str(calls)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"child for {root} failed ({r.returncode}): {r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent", default=None, help="checkout of the parent commit with its library built")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5, help="timed calls per leg and repetition")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--legs", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.legs.split(","), args.calls)
    tree = str(HERE.parents[1])
    runs = {"parent": [], "tree": []}
    for _ in range(args.reps):
        if args.parent:
            runs["parent"].append(run_child(args.parent, ["a_greedy", "b_min_length"], args.calls))
        runs["tree"].append(run_child(tree, list(LEGS), args.calls))
    out = {"metric": "us per decode step, bf16, max_length = min_length = 128", "reps": args.reps, "calls": args.calls}
    for w in WORKLOADS:
        res = {}
        for side, rr in runs.items():
            for leg in (rr[0][w] if rr else {}):
                v = [r[w][leg] for r in rr]
                res[f"{side}/{leg}"] = {"us_per_step": statistics.mean(v), "reps": v, "spread": max(v) - min(v)}
        yard = res.get("parent/b_min_length") or res["tree/b_min_length"]
        c = res["tree/c_min_length_grammar"]
        res["c_vs_b"] = {"yardstick": "parent/b_min_length" if args.parent else "tree/b_min_length",
                         "ratio": c["us_per_step"] / yard["us_per_step"],
                         "c_inside_b_reps": min(yard["reps"]) <= c["us_per_step"] <= max(yard["reps"])}
        out[w] = res
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
