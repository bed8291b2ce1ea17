#!/usr/bin/env python3
"""Gradient accumulation cost (m2m_train_forward_backward_acc): one JSON line per measurement.

  * micro: one forward+backward of 16 clips x 3 s (S = 261, 256 labels, dropout 0.1) in overwrite mode (the plain pass) against
    accumulate mode (grad_scale = 1/8, gradients added in every writer's epilogue), bf16 and fp8; both replay their captured graphs.
  * step: one optimizer step at an effective batch of 128 — 8 accumulated micro-batches of 16 + Adafactor on one GPU — against a
    single 128-clip pass + Adafactor (when the trainer fits on the device).

Times are medians over --reps rounds of --iters calls each, the two modes interleaved round by round (CUDA events, no host sync
inside a round).  Usage: python tools/accum_bench.py [--precisions bf16,fp8] [--iters 20] [--reps 7]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from music2midi_amd import synth  # noqa: E402
from music2midi_amd.checkpoint import load_t5_state  # noqa: E402
from music2midi_amd.config import T5Geometry, default_config  # noqa: E402
from music2midi_amd.training import NativeTrainer  # noqa: E402
from music2midi_amd.transformer import T5Transformer  # noqa: E402

S, LD, MICRO, N = 261, 256, 16, 8


def inputs(B, seed):
    x = torch.from_numpy(synth.normal(seed, "x", (B, S, 384), 2.0)).cuda()
    cond = torch.from_numpy(synth.cond_index_batch(seed, B)).cuda()
    labels = (torch.from_numpy((synth.uniform01(seed, "l", B * LD) * 330).astype(np.int64).reshape(B, LD)) + 3).cuda()
    return x, cond, labels


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precisions", default="bf16,fp8")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    cfg = default_config()
    geom = T5Geometry(cfg.model.t5)
    model = T5Transformer(cfg.to_dict(), precision="fp32")
    load_t5_state(model, synth.t5_state_dict(geom, 0), strict=False)
    model = model.cuda()
    for prec in args.precisions.split(","):
        tr = NativeTrainer(model, MICRO, S, LD, precision=prec)
        tr.set_dropout(0.1, seed=1)
        x, cond, labels = inputs(MICRO, 1)
        over = lambda: tr.forward_backward(x, cond, labels)                                          # noqa: E731
        acc = lambda: tr.forward_backward(x, cond, labels, grad_scale=1.0 / N, accumulate=True)    # noqa: E731
        for _ in range(3):                                   # direct issue, capture, replay: both modes have their graphs
            over(); acc()
        torch.cuda.synchronize()
        t_over, t_acc = [], []
        for _ in range(args.reps):
            t_over.append(timed(over, args.iters))
            t_acc.append(timed(acc, args.iters))
        mo, ma = statistics.median(t_over), statistics.median(t_acc)
        print(json.dumps({"what": "micro_batch", "precision": prec, "clips": MICRO, "S": S, "labels": LD, "dropout": 0.1,
                          "overwrite_ms": round(mo, 4), "accumulate_ms": round(ma, 4), "accumulate_over_overwrite": round(ma / mo, 4),
                          "overwrite_ms_all": [round(v, 4) for v in t_over], "accumulate_ms_all": [round(v, 4) for v in t_acc]}), flush=True)
        if args.skip_step:
            tr.close()
            continue
        micro = [inputs(MICRO, 10 + i) for i in range(N)]

        def window():
            for i, (xi, ci, li) in enumerate(micro):
                tr.forward_backward(xi, ci, li, grad_scale=1.0 / N, accumulate=i > 0)
            tr.optimizer_step()

        window()
        window()
        torch.cuda.synchronize()
        t_win = statistics.median(timed(window, 2) for _ in range(args.reps))
        rec = {"what": "optimizer_step_effective_128", "precision": prec, "accumulated_8x16_ms": round(t_win, 3)}
        tr.close()
        torch.cuda.empty_cache()
        try:
            big = NativeTrainer(model, MICRO * N, S, LD, precision=prec)
            big.set_dropout(0.1, seed=1)
            xb, cb, lb = inputs(MICRO * N, 2)

            def single():
                big.forward_backward(xb, cb, lb)
                big.optimizer_step()

            for _ in range(3):
                single()
            torch.cuda.synchronize()
            t_single = statistics.median(timed(single, 2) for _ in range(args.reps))
            rec.update(single_128_ms=round(t_single, 3), accumulated_over_single=round(t_win / t_single, 4))
            big.close()
        except (RuntimeError, torch.cuda.OutOfMemoryError) as e:      # (the native trainer reports allocation failures as NativeError)
            rec["single_128"] = f"does not fit: {str(e)[:120]}"
        torch.cuda.empty_cache()
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
