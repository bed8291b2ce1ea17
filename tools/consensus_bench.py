#!/usr/bin/env python3
"""Cost of consensus decoding: the pairwise note-level agreement of the K candidates of every clip and the selection on the device
(music2midi_amd.scoring.consensus_choice, csrc/consensus.hip) against the definition on the host on the same ids
(note_metrics.match_counts over the K * (K - 1) ordered pairs of every clip), and ``generate_consensus`` against the two decodes it
contains.

    python tools/consensus_bench.py [--runs 30] [--host-reps 3] [--no-decode] [--limit 600]

Two sizes: a user's, 8 clips x 16 candidates x 1 023 ids over 10 s, and the reference geometry's chunk, 16 segments x 8 candidates x
346 ids over 3 s.  Every clip has a hidden note list in the style of ``render.synthetic_notes`` (as many notes as fill the row);
each candidate is that list quantised, jittered by -1..+1 steps at both ends, a tenth of the notes dropped and up to 3 inserted,
tokenised and cut to the row.  Every size is measured in a child process of its own under a time limit of ``--limit`` seconds; the
first one that fails ends the run.  After 5 warm calls, with ``offset_ratio`` 0.2 and onsets only, the median and the quartiles
over ``--runs`` of
  pairwise_kernel_ms   the time between two events around the pairwise launch alone (notes already on the device)
  select_kernel_ms     the same around the select launch
  choice_ms            the host clock around consensus_choice from the ids to ``chosen``, ending in a synchronise
  host_ms              match_counts over the same pairs on this machine's CPUs, ``--host-reps`` passes (detokenising not included)
and, unless ``--no-decode``, on random-init weights of the default model (bf16) under the MIDI grammar, the host clock (ending in a
synchronise) around ``generate_consensus`` and around the greedy decode and the sampled decode of K - 1 rows per clip it contains,
each run alone.  One lane runs one matching, so the lanes of a wave run loops of different lengths: the kernel time is what it is,
no share of any peak is claimed.  The integers of the two paths must be equal.  Prints one JSON line.  It fails without a GPU.
"""
from __future__ import annotations

import argparse
import copy
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SIZES = [  # clips, candidates per clip, ids per row, notes of the hidden list, seconds per row
    dict(clips=8, K=16, length=1023, notes=250, seconds=10.0),
    dict(clips=16, K=8, length=346, notes=85, seconds=3.0),
]


def _quartiles(values) -> dict:
    q1, q2, q3 = statistics.quantiles(values, n=4)
    return {"median": q2, "q1": q1, "q3": q3}


def measure(size: dict, args) -> dict:
    import numpy as np
    import torch
    from music2midi_amd import consensus, native, note_metrics, scoring
    from music2midi_amd.config import DEFAULT_CONFIG, load_config
    from music2midi_amd.tokenizer import PAD, MidiTokenizer

    native.require_gpu()
    cfg = load_config(copy.deepcopy(DEFAULT_CONFIG))
    tok = MidiTokenizer(cfg)
    B, K, L, n, span = size["clips"], size["K"], size["length"], size["notes"], size["seconds"]
    step = tok.time_step
    rng = np.random.default_rng(B * K)
    ids = np.full((B * K, L), PAD, dtype=np.int64)
    for b in range(B):
        onset = rng.uniform(0.0, span - 0.1, n)
        length = rng.uniform(0.05, 1.0, n)
        pitch = rng.integers(21, 109, n)
        offset = np.minimum(onset + length, span - step)
        for k in range(K):
            keep = rng.random(n) >= 0.1
            on = np.maximum(0, np.rint(onset[keep] / step).astype(np.int64) + rng.integers(-1, 2, keep.sum()))
            off = np.maximum(on + 1, np.rint(offset[keep] / step).astype(np.int64) + rng.integers(-1, 2, keep.sum()))
            extra = int(rng.integers(0, 4))
            e_on = rng.integers(0, int(span / step) - 12, extra)
            on, off = np.concatenate([on, e_on]), np.concatenate([off, e_on + rng.integers(1, 12, extra)])
            pitches = np.concatenate([pitch[keep], rng.integers(21, 109, extra)])
            notes = np.stack([on * step, off * step, pitches.astype(np.float64), np.full(len(on), 80.0)], axis=1)
            row = tok._tokenize(notes[np.argsort(notes[:, 0], kind="stable")]).numpy()[:L]
            ids[b * K + k, :len(row)] = row
    ids_dev = torch.from_numpy(ids).cuda()
    decoded = tok.decode(ids)

    def events(call):
        times = []
        for _ in range(args.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        return _quartiles(times)

    def wall(call, runs):
        times = []
        for _ in range(runs):
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - w0) * 1e3)
        return _quartiles(times)

    dn = scoring.detokenize(tok, ids_dev)
    res = {"clips": B, "candidates": K, "ids_per_row": L, "runs": args.runs, "decoded_notes": int(dn.counts.sum()),
           "workspace_bytes": int(native.load().m2m_consensus_workspace_bytes(B * K, L, K)), "cases": []}
    for ratio in (0.2, None):
        r = -1.0 if ratio is None else ratio
        choice = lambda: scoring.consensus_choice(tok, ids_dev, K, offset_ratio=ratio)
        for _ in range(5):
            chosen, utility = choice()
        tp_dev, n_dev = scoring._enqueue_pairwise(dn, K, 0.05, r, 0.05)
        got = scoring.pairwise_note_counts(tok, ids_dev, K, offset_ratio=ratio)
        case = {"offset_ratio": ratio,
                "pairwise_kernel_ms": events(lambda: scoring._enqueue_pairwise(dn, K, 0.05, r, 0.05)),
                "select_kernel_ms": events(lambda: scoring._enqueue_select(tp_dev, n_dev)),
                "choice_ms": wall(choice, args.runs), "chosen": chosen.cpu().tolist(), "tp_sum": int(got.tp.sum()), "n_sum": int(got.n.sum())}
        host, want = [], None
        for _ in range(args.host_reps):
            h0 = time.perf_counter()
            want = [consensus.pairwise_counts(decoded[b * K:(b + 1) * K], offset_ratio=ratio) for b in range(B)]
            host.append((time.perf_counter() - h0) * 1e3)
        if host:
            case["host_ms"] = statistics.median(host)
            case["host_over_choice"] = case["host_ms"] / case["choice_ms"]["median"]
            case["equal_to_host"] = bool(all(np.array_equal(got.tp[b], w[0]) and np.array_equal(got.n[b], w[1]) for b, w in enumerate(want))
                                         and chosen.cpu().tolist() == [consensus.select(*w)[0] for w in want]
                                         and all(np.array_equal(utility[b].cpu().numpy(), consensus.select(*w)[1]) for b, w in enumerate(want)))
        res["cases"].append(case)
    if not args.no_decode:
        from music2midi_amd import synth
        from music2midi_amd.input import ModelInputs
        from music2midi_amd.model import Music2MIDI
        torch.manual_seed(0)
        m = Music2MIDI(copy.deepcopy(DEFAULT_CONFIG), precision="bf16").cuda().eval()
        samples = int(cfg.dataset.segment_duration * cfg.model.sample_rate)                  # one segment per clip, whatever the row length
        wav = torch.stack([torch.from_numpy(synth.waveform(b, samples, "music")) for b in range(B)]).cuda()
        inputs = ModelInputs(input_waveform=wav, cond_index=torch.zeros((B, len(m.model.conditioning.embeds)), dtype=torch.long).cuda())
        legs = {"generate_consensus_ms": lambda: m.model.generate_consensus(inputs, K, max_length=L + 1, midi_grammar=True),
                "greedy_ms": lambda: m.model.generate(inputs, max_length=L + 1, midi_grammar=True),
                "sampled_ms": lambda: m.model.generate(inputs, max_length=L + 1, midi_grammar=True, do_sample=True,
                                                       num_return_sequences=K - 1)}
        res["decode"] = {"max_length": L + 1, "runs": args.decode_runs}
        for name, leg in legs.items():
            for _ in range(2):
                out = leg()
            res["decode"][name] = wall(leg, args.decode_runs)
            res["decode"][name.replace("_ms", "_width")] = int(out.shape[1])
        d = res["decode"]
        d["consensus_minus_decodes_ms"] = d["generate_consensus_ms"]["median"] - d["greedy_ms"]["median"] - d["sampled_ms"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--decode-runs", type=int, default=30, help="runs of each decode leg")
    ap.add_argument("--host-reps", type=int, default=3, help="0 skips the host leg")
    ap.add_argument("--no-decode", action="store_true", help="skip generate_consensus and the two decodes")
    ap.add_argument("--limit", type=float, default=600.0, help="seconds one size may take")
    ap.add_argument("--size", type=int, default=None, help="measure this size only, in this process")
    args = ap.parse_args()
    if args.runs < 20 or args.decode_runs < 5:
        ap.error("--runs must be at least 20 and --decode-runs at least 5")
    if args.size is not None:
        print(json.dumps(measure(SIZES[args.size], args)), flush=True)
        return
    results = []
    for i in range(len(SIZES)):
        cmd = [sys.executable, str(Path(__file__).resolve()), "--size", str(i), "--runs", str(args.runs), "--decode-runs", str(args.decode_runs),
               "--host-reps", str(args.host_reps)] + (["--no-decode"] if args.no_decode else [])
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"size {i} did not finish within {args.limit:g} s: nothing more is started") from None
        if done.returncode != 0:
            raise SystemExit(f"size {i} failed with status {done.returncode}: nothing more is started\n{done.stderr[-2000:]}")
        results.append(json.loads(done.stdout.strip().splitlines()[-1]))
    print(json.dumps({"sizes": results}), flush=True)
    if any(c.get("equal_to_host") is False for r in results for c in r["cases"]):
        raise SystemExit("the device results differ from the definition's")


if __name__ == "__main__":
    main()
