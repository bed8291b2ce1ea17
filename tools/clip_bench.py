#!/usr/bin/env python3
"""Time the Adafactor step with gradient clipping off, in norm mode and in value mode, at the full default model.

    python tools/clip_bench.py [--rounds 3] [--samples 30] [--inner 10]
    M2M_LIBRARY=/path/to/the/parent/commit's/libmusic2midi_amd.so python tools/clip_bench.py      # adds the "parent" leg

Every measurement runs in a child process of its own (one library per process; never more than one process on the GPU).  A product
child times the three legs ALTERNATING — off, norm, value, off, norm, ... — so a drift of the clocks meets all of them alike; a sample
is `inner` optimizer steps back to back between two events, divided by `inner`; a leg's figure is the median of `samples` samples,
warm.  With M2M_LIBRARY set, parent children (the unclipped step of that library, bound without the two clipping exports it does not
have) alternate with the product children, `rounds` of each; the spread printed is min .. max of the rounds' medians.
The gradient is N(0, 1) in every tensor; max_norm is half its norm (the clip is active), the value clamp 0.05.  One JSON line at the end.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def child(legs, samples, inner):
    import torch
    from music2midi_amd import native, synth
    if legs == ["parent"]:                                  # the parent commit's library: it has no clipping exports to bind
        for name in ("m2m_trainer_set_grad_clip", "m2m_trainer_grad_norm"):
            native._SIGNATURES.pop(name, None)
    from music2midi_amd.checkpoint import load_t5_state
    from music2midi_amd.config import T5Geometry, default_config
    from music2midi_amd.training import NativeTrainer
    from music2midi_amd.transformer import T5Transformer
    cfg = default_config()
    model = T5Transformer(cfg.to_dict(), precision="fp32")
    load_t5_state(model, synth.t5_state_dict(T5Geometry(cfg.model.t5), 0), strict=False)
    tr = NativeTrainer(model.cuda(), 1, 4, 2, precision="fp32")
    for off, shape in tr.layout.values():
        n = 1
        for s in shape:
            n *= s
        tr.grads[off:off + n].normal_(generator=torch.Generator(device="cuda").manual_seed(off))
    norm = float(tr.grads.double().norm())
    settings = {"off": ("off", 0.0), "norm": ("norm", 0.5 * norm), "value": ("value", 0.05), "parent": None}
    times = {leg: [] for leg in legs}
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(-3, samples):                            # three warm rounds
        for leg in legs:
            if settings[leg] is not None:
                tr.set_grad_clip(*settings[leg])
            start.record()
            for _ in range(inner):
                tr.optimizer_step()
            stop.record()
            stop.synchronize()
            if i >= 0:
                times[leg].append(1e3 * start.elapsed_time(stop) / inner)      # us per step
    tr.close()
    print("CLIP_BENCH_CHILD " + json.dumps({leg: statistics.median(v) for leg, v in times.items()}), flush=True)


def run_child(legs, args, library):
    env = dict(os.environ)
    env.pop("M2M_LIBRARY", None)
    if library:
        env["M2M_LIBRARY"] = library
    cmd = [sys.executable, str(Path(__file__).resolve()), "--child", ",".join(legs), "--samples", str(args.samples), "--inner", str(args.inner)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise SystemExit(f"child {legs} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("CLIP_BENCH_CHILD ")][-1]
    return json.loads(line[len("CLIP_BENCH_CHILD "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child.split(","), args.samples, args.inner)
    parent_lib = os.environ.get("M2M_LIBRARY")
    medians = {}
    for _ in range(args.rounds):
        if parent_lib:
            for leg, v in run_child(["parent"], args, parent_lib).items():
                medians.setdefault(leg, []).append(v)
        for leg, v in run_child(["off", "norm", "value"], args, None).items():
            medians.setdefault(leg, []).append(v)
    out = {}
    for leg in ("parent", "off", "norm", "value"):
        if leg in medians:
            v = medians[leg]
            out[leg] = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
            print(f"{leg:7s} {out[leg]['median_us']:8.2f} us per step   (rounds: {out[leg]['min_us']:.2f} .. {out[leg]['max_us']:.2f})")
    print(json.dumps({"bench": "adafactor_step_clipping", "rounds": args.rounds, "samples": args.samples, "inner": args.inner, **out}))


if __name__ == "__main__":
    main()
