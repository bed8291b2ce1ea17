#!/usr/bin/env python3
"""Time of the training augmentation for one batch: the device path (music2midi_amd.augment.pitch_shift_batch) against the host
definition (music2midi_amd.audio.normalize + pitch_shift, one clip after the other).

    python tools/augment_bench.py [--clips 16] [--samples 66150] [--iters 50] [--host-reps 1]

The batch: ``--clips`` x ``--samples`` fp32 samples of seeded noise plus two tones (every bin of every frame carries energy, so the
host function is well conditioned and the parity figure printed at the end means something; on signals with silent bins the
host's own output moves by more than its peak under fp32-sized input noise), steps cycling through -6 .. 5 (the reference's
``randint(-6, 6)``), every other clip normalised.  The device time is the mean of ``--iters`` calls between two events on the
stream after 5 warm-up calls (the workspace exists, the tables are in cache); the yardstick is one training step, 3.89 ms for 16
clips (README).  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--samples", type=int, default=66150)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=1, help="0 skips the host leg")
    args = ap.parse_args()

    import numpy as np
    import torch
    from music2midi_amd import audio, augment

    B, T = args.clips, args.samples
    steps = [(i % 12) - 6 for i in range(B)]
    norms = [i % 2 == 1 for i in range(B)]
    t = np.arange(T) / 22050.0
    tones = 0.2 * np.sin(2 * np.pi * 440.0 * t) + 0.15 * np.sin(2 * np.pi * 1318.5 * t)
    wav = np.stack([(0.25 * np.random.default_rng(b).standard_normal(T) + tones).astype(np.float32) for b in range(B)])
    x = torch.from_numpy(wav).cuda()
    for _ in range(5):
        out = augment.pitch_shift_batch(x, steps, norms)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    wall0 = time.perf_counter()
    t0.record()
    for _ in range(args.iters):
        out = augment.pitch_shift_batch(x, steps, norms)
    t1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - wall0) / args.iters
    dev_ms = t0.elapsed_time(t1) / args.iters
    res = {"clips": B, "samples": T, "steps": steps, "device_ms": dev_ms, "device_wall_ms": wall * 1e3, "train_step_ms": 3.89,
           "device_below_one_step": dev_ms < 3.89}
    if args.host_reps > 0:
        best = None
        for _ in range(args.host_reps):
            h0 = time.perf_counter()
            host = [audio.pitch_shift(audio.normalize(wav[b]) if norms[b] else wav[b], 22050, steps[b]) for b in range(B)]
            dt = time.perf_counter() - h0
            best = dt if best is None else min(best, dt)
        got = out.cpu().numpy()
        res["host_ms"] = best * 1e3
        res["host_ms_per_clip"] = best * 1e3 / B
        res["host_over_device"] = best * 1e3 / dev_ms
        res["worst_rel_err_vs_host"] = max(float(np.abs(got[b] - host[b]).max() / np.abs(host[b]).max()) for b in range(B))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
