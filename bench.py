#!/usr/bin/env python3
"""Headline benchmark: decoded MIDI tokens / second on synthetic 10 s clips.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--precision bf16|fp32] [--batch 32] [--dump-outputs DIR] [--full]

A "step" is one pass of the whole hot path over one batch of synthetic clips:
fused STFT/log-mel frontend -> conditioning rows -> T5 encoder -> cross-K/V
projection -> 1023 KV-cached greedy decode steps (max_length 1024; the headline
clips' trajectories under the random-init weights hold no EOS, so every clip
yields 1023 new tokens; the line counts tokens up to a row's EOS and reports
`config.rows_with_eos`, so a trajectory that did end would not be over-counted).
Workload = BASELINE.json configs[2] (bf16, batch 32 per GPU, 220 500-sample
clips -> encoder length 864); with N > 1 every rank decodes its own 32 clips
(weak scaling, configs[3]) after one RCCL weight broadcast, and the decoded
token matrices are all-gathered every step.  Waveforms are resident in HBM when
the timed region starts.

Launching N > 1: either under ``torch.distributed.run`` (RANK / LOCAL_RANK /
WORLD_SIZE in the environment) or plainly as ``python bench.py --gpus N`` — in
that case THIS process starts N fresh rank processes itself (before it has made
any HIP call; nothing that touched the GPU is ever exec'ed or forked), forwards
rank 0's JSON line and exits non-zero if any rank failed.

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times the steps,
writes its outputs if asked and prints the headline line, nothing more.
``--full`` adds (N = 1, rank 0, after the timed steps) the records beside the
headline: phase timings and `roofline`, the configs[1] frontend, the reference's
own geometry and the ragged-EOS batches, the fp32 parity mode, the configs[4]
training step and the CPU baselines; the ``--no-*`` options leave single ones
out.  `roofline` is measured live with hipEvents on
the stream the kernels run on (m2m_bench_kernel); `cpu_baseline` times the
oracle (a PyTorch-CPU restatement of the reference path — the reference's own
Python cannot run here: torchaudio/lightning/omegaconf are absent) on a bounded
sample on the host cores.  ``--dump-outputs DIR`` writes what the timed path returned in its last step
(rank 0: the generate mode's token ids; the train mode's loss and a fixed sample of the updated weights and
gradients) as ``DIR/<name>.npy``, so two builds can be compared output for output.  ``--dry-run`` exercises the launcher and both
collectives on CPU tensors (gloo) without any GPU work — tests/test_bench_launcher.py.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0     # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured-achievable)
MFMA_PEAK_TFLOPS = {"bf16": 2500.0, "fp8": 5000.0}   # dense peaks (no 2:1 sparsity)
N_SAMPLES = 220500        # 10 s @ 22.05 kHz
N_FRAMES = 1 + N_SAMPLES // 256
MAX_LENGTH = 1024
DEC_PARAMS_PER_STEP = 15201664   # decoder weights read once per step, elements


# ------------------------------------------------------------------ launcher
def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_log_dir() -> Path:
    """Where the ranks' stderr goes: gpurun_out/ (merged back from the GPU box) or $M2M_BENCH_LOG_DIR; a temp dir as a last resort."""
    for cand in (os.environ.get("M2M_BENCH_LOG_DIR"), ROOT / "gpurun_out"):
        if not cand:
            continue
        try:
            Path(cand).mkdir(parents=True, exist_ok=True)
            probe = Path(cand) / ".bench_write_probe"
            probe.write_text("")
            probe.unlink()
            return Path(cand)
        except OSError:
            continue
    import tempfile
    return Path(tempfile.mkdtemp(prefix="m2m_bench_"))


def _tail(path: Path, n: int = 25) -> str:
    try:
        return "\n".join(path.read_text(errors="replace").splitlines()[-n:])
    except OSError:
        return ""


DUMP_LIMIT_BYTES = 64 << 20   # --dump-outputs: everything written together stays under 64 MB
DUMP_SAMPLE = 1 << 20          # elements of a fixed, seeded sample taken from a flat output larger than this


def dump_sample(flat: torch.Tensor) -> np.ndarray:
    """A fixed sample of a large flat tensor: the same sorted indices (seed 0) on every run of the same shape."""
    n = flat.numel()
    if n <= DUMP_SAMPLE:
        return flat.detach().float().cpu().numpy()
    idx = np.sort(np.random.default_rng(0).choice(n, DUMP_SAMPLE, replace=False))
    return flat.detach().float()[torch.from_numpy(idx).to(flat.device)].cpu().numpy()


def dump_outputs(outdir: str, arrays: dict) -> None:
    """Write each array as <outdir>/<name>.npy in float32 / float64 (token ids go as float64: exact)."""
    arrs = {k: np.ascontiguousarray(v, dtype=np.float32 if v.dtype == np.float32 else np.float64) for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrs.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit(f"[bench] --dump-outputs: {total} bytes exceed the {DUMP_LIMIT_BYTES}-byte limit")
    Path(outdir).mkdir(parents=True, exist_ok=True)
    for k, a in arrs.items():
        np.save(Path(outdir) / f"{k}.npy", a)


def spawn_ranks(n: int) -> int:
    """Start n rank processes of this script (one per GPU) and wait for them — with a deadline.

    Runs in a parent that has not touched the GPU (no torch.cuda / HIP call so far): children are
    fresh interpreters started with subprocess (never an exec of this process), each pinned to its GPU
    through LOCAL_RANK and to its share of the host cores through OMP_NUM_THREADS.  stdout of rank 0
    carries the JSON line and is inherited; every rank's stderr goes to a file of its own
    (bench_rank<r>.err: 8 interleaved RCCL logs are unreadable).  A failing rank ends the others (by
    PID) and makes the exit code non-zero; so does the watchdog: if the ranks have not all finished
    after M2M_BENCH_TIMEOUT seconds (default 1500; a rank stuck in RCCL initialisation is the likeliest
    failure of a first multi-GPU run) the parent says which ranks were still alive, shows the tail of
    their logs, terminates them (SIGTERM, then SIGKILL) and exits with 124."""
    port = _free_port()
    logdir = _rank_log_dir()
    deadline = time.monotonic() + float(os.environ.get("M2M_BENCH_TIMEOUT", "1500"))
    threads = max(1, min(16, (os.cpu_count() or n) // n))
    procs, logs = [], []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), M2M_BENCH_CHILD="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        env.setdefault("OMP_NUM_THREADS", str(threads))
        env.setdefault("M2M_BENCH_THREADS", str(threads))
        logs.append(logdir / f"bench_rank{r}.err")
        with open(logs[r], "w") as errf:
            procs.append(subprocess.Popen([sys.executable, str(Path(__file__).resolve()), *sys.argv[1:]], env=env,
                                          stdout=None if r == 0 else subprocess.DEVNULL, stderr=errf))

    def stop(ranks):
        for o in ranks:
            procs[o].terminate()
        t_end = time.monotonic() + 10.0
        for o in ranks:
            try:
                procs[o].wait(max(0.1, t_end - time.monotonic()))
            except subprocess.TimeoutExpired:
                procs[o].kill()

    rc = 0
    pending = set(range(n))
    while pending:
        for r in sorted(pending):
            code = procs[r].poll()
            if code is None:
                continue
            pending.discard(r)
            if code != 0 and rc == 0:
                rc = code if code > 0 else 1
                print(f"[bench] rank {r} exited with {code}: stopping the other ranks (logs: {logdir}/bench_rank*.err)\n"
                      f"---- rank {r} stderr (tail) ----\n{_tail(logs[r])}", file=sys.stderr)
                stop(sorted(pending))
        if pending and rc == 0 and time.monotonic() > deadline:
            alive = sorted(pending)
            print(f"[bench] watchdog: ranks {alive} still running after {os.environ.get('M2M_BENCH_TIMEOUT', '1500')} s "
                  f"(finished: {sorted(set(range(n)) - pending)}); terminating them", file=sys.stderr)
            for r in alive:
                print(f"---- rank {r} stderr (tail) ----\n{_tail(logs[r], 12)}", file=sys.stderr)
            stop(alive)
            return 124
        time.sleep(0.05)
    if rc == 0:      # a clean run still shows what rank 0 had to say (warnings), briefly
        t0 = _tail(logs[0], 6)
        if t0.strip():
            print(t0, file=sys.stderr)
    return rc


def pin_host_threads(world: int) -> int:
    """Each rank keeps to its share of the host cores (8 ranks x every core oversubscribes the box; the CPU side of a step is tiny)."""
    n = int(os.environ.get("M2M_BENCH_THREADS") or max(1, min(16, (os.cpu_count() or world) // max(1, world))))
    torch.set_num_threads(n)
    return n


# ------------------------------------------------------------------ CPU baselines (oracle; checker code, timed only)
def host_cpu_share() -> dict:
    """What this process may use of the host: visible CPUs and the cgroup quota (cpu.max = "<quota> <period>" in microseconds).
    The GPU boxes show 256 CPUs with a quota of 16: a 16-thread figure IS the whole share (round-4 review asked for a whole-host
    figure next to it; tools/cpu_threads_probe.py's 32 / 64 / 128-thread runs were slower because they oversubscribe that quota)."""
    out = {"visible_cpus": os.cpu_count(), "cgroup_cpu_quota": None}
    try:
        q, per = Path("/sys/fs/cgroup/cpu.max").read_text().split()[:2]
        out["cgroup_cpu_quota"] = None if q == "max" else round(int(q) / int(per), 2)
    except Exception:
        pass
    return out


ENC_PASSES = 20      # encoder + cross-K/V passes timed for extras.encoder_plus_crosskv_ms


def cpu_baseline(cfg, state, new_tokens: int, clips: int = 8, threads: int = 16):
    """Oracle on the host cores, fp32: `clips` clips batched (frontend + encoder + `new_tokens` greedy
    steps each) and ONE clip alone (BASELINE configs[0]).

    16 intra-op threads: measured fastest on the GPU box's 256-core host (tools/cpu_threads_probe.py:
    4/8/16/32/64/128 threads -> 198/205/211/99/44/18 tokens/s for one clip; the matmuls are tiny, so
    one process uses ~16 cores productively — the other cores could run further independent processes)."""
    from music2midi_amd import synth
    from music2midi_amd.config import T5Geometry
    from oracle.logmel import LogMelOracle, conditioning
    from oracle.t5 import T5Oracle

    geom = T5Geometry(cfg.model.t5)
    threads = min(threads, os.cpu_count() or threads)
    torch.set_num_threads(threads)
    fe = LogMelOracle(cfg.model.sample_rate, cfg.spectrogram.n_fft, cfg.spectrogram.hop_length,
                      cfg.spectrogram.f_min, geom.d_model)
    orc = T5Oracle(geom, state, emulate="fp32")
    emb = [torch.from_numpy(state[f"conditioning.embeds.{i}.weight"]) for i in range(2)]

    def run(n_clips):
        wav = torch.from_numpy(synth.waveform_batch(0, n_clips, N_SAMPLES))
        idx = torch.from_numpy(synth.cond_index_batch(0, n_clips))
        t0 = time.perf_counter()
        x = conditioning(fe(wav), idx, emb)
        ids = orc.generate(x, new_tokens + 1)
        dt = time.perf_counter() - t0
        return (ids.shape[1] - 1) * n_clips / dt, dt, ids.shape[1] - 1

    single, dt1, n1 = run(1)
    batched, dtb, nb = run(clips)
    share = host_cpu_share()
    return {"value": batched, "unit": "tokens/s", "cores": threads, "kind": "port", "host_share": share,
            "whole_share_note": (f"the box grants this job {share['cgroup_cpu_quota']} CPUs (cgroup cpu.max) of {share['visible_cpus']} visible: "
                                 f"{threads} threads use the whole share" if share["cgroup_cpu_quota"] else "no cgroup CPU quota found"),
            "sample": f"{clips} clips x {N_SAMPLES} samples in one batch: log-mel + encoder (S=864) + {nb} greedy "
                      f"decode steps each, fp32 torch-CPU oracle, {dtb:.1f} s wall, {threads} threads of "
                      f"os.cpu_count()={os.cpu_count()}",
            "configs0_single_clip": {"value": single, "unit": "tokens/s", "cores": threads,
                                     "sample": f"BASELINE configs[0]: ONE 10 s clip, log-mel + encoder + {n1} greedy steps, "
                                               f"{dt1:.1f} s wall"}}


def cpu_frontend_baseline(cfg, clips: int = 64, threads: int = 16):
    """BASELINE configs[1]'s CPU side: torch.stft + dense mel matmul + clamp/log (the oracle) on `clips` clips."""
    from music2midi_amd import synth
    from oracle.logmel import LogMelOracle
    threads = min(threads, os.cpu_count() or threads)
    torch.set_num_threads(threads)
    fe = LogMelOracle(cfg.model.sample_rate, cfg.spectrogram.n_fft, cfg.spectrogram.hop_length,
                      cfg.spectrogram.f_min, cfg.model.t5.d_model)
    wav = torch.from_numpy(synth.waveform_batch(0, clips, N_SAMPLES))
    fe(wav[:2])
    t0 = time.perf_counter()
    fe(wav)
    dt = time.perf_counter() - t0
    return {"clips_per_s": clips / dt, "ms_per_batch": dt * 1e3, "cores": threads, "kind": "port",
            "sample": f"torch.stft + dense [1025x384] mel matmul + clamp/log on {clips} x {N_SAMPLES} samples, fp32"}


def pmc_traffic_bytes(kernel_substr: str, batch: int, n_chains: int = 1, profiles_dir=None, precision: str = "bf16"):
    """HBM bytes of one co-scheduled launch set (all `batch` clips) of a kernel from the newest committed PMC summary
    (profiles/*pmc_traffic_summary.txt, collected by tools/pmc_traffic.sh in separate FETCH_SIZE / WRITE_SIZE passes;
    FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes for gfx950).  The summary lists bytes per KERNEL launch; a launch
    covers `clips/launch` clips — stated in the summary's header, which tools/pmc_traffic.sh writes — so the figure is scaled to
    `batch` clips.  A summary WITHOUT that header is refused (None, with a note on stderr): guessing the launch width is how round 2
    reported half the traffic.  None when no summary is present."""
    import re
    best = None
    files = sorted(Path(profiles_dir or ROOT / "profiles").glob("*pmc_traffic_summary.txt"), key=lambda f: (_round_of(f.name), f.name))
    # the fp32 mode has summaries of its own (tools/r6_fp32_profile.sh: *_fp32_pmc_traffic_summary.txt)
    files = [f for f in files if "frontend" not in f.name and ("fp32" in f.name) == (precision == "fp32")]
    for f in files[-1:]:                       # the newest round's summary only: an older one describes older kernels
        text = f.read_text()
        m = re.search(r"clips/launch\s*=\s*(\d+)", text)
        if not m:
            print(f"[bench] {f.name} has no 'clips/launch = N' header: roofline.traffic left null", file=sys.stderr)
            return None
        per_launch = int(m.group(1))
        vals = []
        for line in text.splitlines():
            if kernel_substr in line:
                m = re.search(r"x2 corrected\s+([0-9.]+) MB\).*WRITE_SIZE/launch\s+[0-9.]+ KiB \(\s*([0-9.]+) MB\)", line)
                if m:
                    vals.append((float(m.group(1)) + float(m.group(2))) * 1e6 * batch / per_launch)
        if vals:   # several template variants of the kernel (cache policy): mean per launch
            best = sum(vals) / len(vals)
    return best


def _round_of(name: str) -> int:
    import re
    m = re.match(r"r(\d+)_", name)
    return int(m.group(1)) if m else 0


def _bf16_noise_margin(case: str) -> float:
    """1.5 x the largest change of (top-1 - top-2) the bf16-emulating oracle shows against itself under a 1e-6 input perturbation
    along the forced sequence (tests/golden/t5_forced.npz, `self_noise_margin`): the measured floor tests/test_golden_gpu.py uses."""
    sys.path.insert(0, str(ROOT / "tests")) if str(ROOT / "tests") not in sys.path else None
    from forced_check import bf16_margin_threshold
    return bf16_margin_threshold(np.load(ROOT / "tests" / "golden" / "t5_forced.npz"), case)


def golden_divergence(ids_bf16, ids_fp32) -> dict:
    """Clips 0 and 1 of this workload against the committed oracle ids (tests/golden/t5_bf16.npz, written by
    tests/golden/make_golden.py t5_bf16 from the bf16-EMULATING oracle and the fp32 oracle on the same waveforms): where the
    device's bf16 ids first leave the emulation's, and the oracle's own top-2 margin at that step — a divergence at a margin
    below the measured bf16 noise margin is rounding, one above it would be a bug; the fp32 mode must not diverge at all.  A fixture file
    (data), read here; the oracle itself is not imported."""
    f = ROOT / "tests" / "golden" / "t5_bf16.npz"
    if not f.exists() or not (ROOT / "tests" / "golden" / "t5_forced.npz").exists():
        return {}
    z = np.load(f)
    noise_margin = _bf16_noise_margin("bench_clips_bf16")

    def first_div(ids, want, margins):
        ids = ids[: want.shape[0], : want.shape[1]].cpu().numpy()
        rows = []
        for b in range(want.shape[0]):
            d = np.nonzero(ids[b] != want[b, : ids.shape[1]])[0]
            # ids[:, t] is chosen from margins[:, t - 1]; column 0 is the start token (a difference there is not a decode decision)
            rows.append({"step": int(d[0]), "oracle_margin": float(margins[b, d[0] - 1]) if d[0] >= 1 else None} if len(d)
                        else {"step": -1, "oracle_margin": None})
        return rows
    bf = first_div(ids_bf16, z["bench_clips_bf16/ids"].astype(np.int64), z["bench_clips_bf16/margins"])
    fp = first_div(ids_fp32, z["bench_clips_fp32/ids"].astype(np.int64), z["bench_clips_fp32/margins"])
    return {"bf16_vs_bf16_oracle_first_divergence": bf, "bf16_noise_margin": noise_margin,
            "bf16_noise_margin_source": "min(0.5, 1.5 x the bf16-emulating oracle's own largest top-2 margin change under a 1e-6 input perturbation, median of 5 seeds; t5_forced.npz)",
            "bf16_divergences_above_noise_margin": int(sum(1 for r in bf if r["step"] >= 0 and (r["oracle_margin"] is None or r["oracle_margin"] >= noise_margin))),
            "fp32_vs_fp32_oracle_first_divergence": [r["step"] for r in fp]}


def forced_parity_record(cfg, geom, dev, model_bf16, model_fp32, x_bench2) -> dict:
    """Both precision modes along ALL 1 023 positions of the headline sequence (tests/forced_check.py + tests/golden/t5_forced.npz):
    the oracle's ids forced through the KV-cached decode kernels on a 32-clip batch.  `x_bench2`: clips 0-1 of this workload as the
    DEVICE's frontend produced them (the tests use the oracle's log-mel; the frontend's <= 1e-4 is inside the fp32 record here)."""
    sys.path.insert(0, str(ROOT / "tests"))
    from forced_check import forced_check
    from music2midi_amd import synth
    from music2midi_amd.checkpoint import load_t5_state
    from music2midi_amd.transformer import T5Transformer
    out = {}
    sd = synth.t5_state_dict(geom, seed=0)
    synth.perturb_layer_norms(sd, 0)
    x_full = torch.from_numpy(synth.normal(7, "embeds", (2, 864, geom.d_model), 3.0)).to(dev)
    for prec, mbench in (("bf16", model_bf16), ("fp32", model_fp32)):
        mfull = T5Transformer(cfg.to_dict(), precision=prec)
        load_t5_state(mfull, sd, strict=False)
        mfull = mfull.to(dev).eval()
        recs = [forced_check(mfull, x_full, f"full_s864_{prec}", prec), forced_check(mbench, x_bench2, f"bench_clips_{prec}", prec)]
        del mfull
        out[f"{prec}_forced_positions_checked"] = int(sum(r["positions"] for r in recs))
        out[f"{prec}_forced_argmax_agree"] = int(sum(r["argmax_agree"] for r in recs))
        out[f"{prec}_forced_argmax_asserted"] = int(sum(r["argmax_asserted_positions"] for r in recs))
        out[f"{prec}_forced_max_logit_err"] = max(r["max_logit_err"] for r in recs)
        out[f"{prec}_forced_p999_logit_err"] = max(r["p999_logit_err"] for r in recs)
        out[f"{prec}_forced_mean_logit_err"] = float(np.mean([r["mean_logit_err"] for r in recs]))
        out[f"{prec}_forced_logit_err_bars"] = [r["logit_err_bars_max_p999_mean"] for r in recs]
    # ... and the bf16 mode against the FP32 reference itself, to fixed absolute bars (nothing here comes from the emulation)
    from forced_check import forced_bf16_vs_fp32
    mfull = T5Transformer(cfg.to_dict(), precision="bf16")
    load_t5_state(mfull, sd, strict=False)
    mfull = mfull.to(dev).eval()
    cross = [forced_bf16_vs_fp32(mfull, x_full, "full_s864_fp32"), forced_bf16_vs_fp32(model_bf16, x_bench2, "bench_clips_fp32")]
    del mfull
    out["bf16_vs_fp32_oracle_forced_max_p999_mean_logit_err"] = [r["max_p999_mean_logit_err_vs_fp32_oracle"] for r in cross]
    out["bf16_vs_fp32_oracle_forced_bars"] = cross[0]["bars"]
    out["bf16_vs_fp32_oracle_forced_argmax_agree"] = int(sum(r["argmax_agree_with_fp32_oracle"] for r in cross))
    out["forced_note"] = ("oracle ids forced through the KV-cached decode kernels (M2M_FORWARD=step), S=864, 1023 positions x 4 clips, batch 32 "
                          "(16 bit-identical copies); bf16 bars = the bf16-emulating oracle's own noise floor x (1.5, 1.3, 1.2) on (max, p99.9, mean); "
                          "logit scale ~75-85")
    return out


def ragged_eos_record(cfg, geom, dev, B: int, S: int, eos_scale: float = 1.6, reps: int = 3) -> dict:
    """Rows that END: real checkpoints finish a segment after tens to hundreds of tokens of the 1 024 budget, the synthetic headline
    workload never emits EOS.  Weights crafted with synth.force_eos_head so that the rows of a batch stop at different steps;
    timed with the finished-row early-out of the decode attention kernels on (default) and off (M2M_FINISHED_SKIP=0: a finished
    row keeps streaming its K/V until the whole chain is done, as HF does and as rounds 1-3 did).  The ids must be identical.
    `useful` tokens = tokens up to and including each row's EOS (or the budget).  Inputs are synthetic encoder embeddings
    (N(0, 3^2), as the parity tests use): on white-noise waveforms the crafted head never wins, every row runs to the budget
    (tools/eos_scale_probe.py); the record is about the decode loop, the frontend is not part of it."""
    from music2midi_amd import synth
    from music2midi_amd.checkpoint import load_t5_state
    from music2midi_amd.input import ModelInputs
    from music2midi_amd.transformer import T5Transformer
    sd = synth.t5_state_dict(geom, seed=0)
    synth.perturb_layer_norms(sd, 0)
    synth.force_eos_head(sd, geom, active=340, eos_scale=eos_scale)
    x = torch.from_numpy(synth.normal(21, "embeds", (B, S, geom.d_model), 3.0)).to(dev)
    out, ids, repacks = {}, {}, (0, 0)
    old = {k: os.environ.get(k) for k in ("M2M_FINISHED_SKIP", "M2M_COMPACT")}
    try:
        # three legs: the product (finished-row early-out + live-row re-packing at the host polls, round 5), the early-out alone
        # (round 4), and neither (every row computed to the end of the chain, as HF does and as rounds 1-3 did)
        for leg, skip, comp in (("repack", None, None), ("skip_on", None, "0"), ("skip_off", "0", "0")):
            for k, v in (("M2M_FINISHED_SKIP", skip), ("M2M_COMPACT", comp)):
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
            m = T5Transformer(cfg.to_dict(), precision="bf16")        # a session of its own: the flag is baked into its captured graphs
            load_t5_state(m, sd, strict=False)
            m = m.to(dev).eval()
            ids[leg] = m.generate_from_embeds(x, max_length=MAX_LENGTH)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(reps):
                m.generate_from_embeds(x, max_length=MAX_LENGTH)
            torch.cuda.synchronize(dev)
            out[leg] = (time.perf_counter() - t0) / reps
            if leg == "repack":
                repacks = m.repack_stats()
            del m
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    a = ids["skip_on"].cpu().numpy()
    L = a.shape[1]
    ends = []
    for r in range(B):
        e = np.nonzero(a[r] == geom.eos_token_id)[0]
        ends.append(int(e[0]) if len(e) else L - 1)
    useful = int(sum(ends))
    qs = sorted(ends)
    return {"workload": f"{B} clips, encoder length S={S} (synthetic embeddings), bf16, max_length {MAX_LENGTH}, lm_head crafted (force_eos_head active=340, "
                        f"eos_scale={eos_scale}) so rows end at different steps; encoder + greedy decode",
            "eos_position_quartiles": [qs[int(q * (B - 1))] for q in (0, 0.25, 0.5, 0.75, 1.0)],
            "rows_with_eos": int(sum(1 for r in range(B) if (a[r] == geom.eos_token_id).any())), "output_length": int(L),
            "eos_position_min_median_max": [int(min(ends)), int(np.median(ends)), int(max(ends))], "useful_tokens": useful,
            "decoded_positions": int(B * (L - 1)),
            "ids_identical_with_and_without_skip": bool(torch.equal(ids["skip_on"], ids["skip_off"]) and torch.equal(ids["repack"], ids["skip_off"])),
            "repackings_per_batch": int(repacks[0]), "rows_moved_per_batch": int(repacks[1]),
            "ms_per_batch": out["repack"] * 1e3, "ms_per_batch_skip_on": out["skip_on"] * 1e3, "ms_per_batch_skip_off": out["skip_off"] * 1e3,
            "useful_tokens_per_s": useful / out["repack"], "useful_tokens_per_s_skip_on": useful / out["skip_on"],
            "useful_tokens_per_s_skip_off": useful / out["skip_off"],
            "speedup": out["skip_off"] / out["repack"], "speedup_early_out_alone": out["skip_off"] / out["skip_on"],
            "legs": "ms_per_batch = early-out + live-row re-packing (product); _skip_on = early-out alone (M2M_COMPACT=0, round 4); "
                    "_skip_off = every row computed to the end (M2M_FINISHED_SKIP=0 M2M_COMPACT=0, HF's behaviour, rounds 1-3); speedup = _skip_off / product"}


def reference_native_record(model, cfg, geom, dev, reps: int = 3, esize: int = 2) -> dict:
    """The reference's own inference geometry (ref config.yaml:16,46-47, model.py:115-134): one `inference.batch_size` = 128 chunk of
    3 s segments at 16 kHz (48 000 samples -> S = 190), max_length 1024, bf16, same random-init weights (no EOS: 1 023 tokens per row)."""
    from music2midi_amd import synth
    from music2midi_amd.input import ModelInputs
    Bn, Tn = int(cfg.inference.batch_size), int(cfg.model.sample_rate * cfg.dataset.segment_duration)
    Sn = 1 + Tn // 256 + 2
    wav = torch.from_numpy(synth.waveform_batch(1000, Bn, Tn)).to(dev)
    cond = torch.from_numpy(synth.cond_index_batch(1000, Bn)).to(dev)
    inputs = ModelInputs(input_waveform=wav, cond_index=cond)
    toks = model.generate(inputs, max_length=MAX_LENGTH)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(reps):
        toks = model.generate(inputs, max_length=MAX_LENGTH)
    torch.cuda.synchronize(dev)
    dt = (time.perf_counter() - t0) / reps
    n_steps = toks.shape[1] - 1
    step_bytes = decode_bytes_per_step(Bn, Sn, (1 + n_steps) / 2.0, esize)
    step_us = dt / n_steps * 1e6              # encoder + frontend included (an upper bound on the step: they are ~1 % of the batch)
    # the attention launch sets of this geometry, live (m2m_bench_kernel: both 64-clip chains' launches on their own streams, cycling the layers)
    from music2midi_amd import native
    x = model.encoder_inputs(inputs)
    model._encode(x, MAX_LENGTH)
    cross_us, cross_bytes = model.bench_kernel(native.KERNEL_DEC_CROSS_ATTN, MAX_LENGTH // 2, 300)
    self_us, self_bytes = model.bench_kernel(native.KERNEL_DEC_SELF_ATTN, MAX_LENGTH // 2, 300)
    kernels = {"cross_attn_launch_set_us": cross_us, "cross_attn_GBs": cross_bytes / (cross_us * 1e-6) / 1e9,
               "cross_attn_frac": cross_bytes / (cross_us * 1e-6) / 1e9 / HBM_PEAK_GBS,
               "self_attn_launch_set_us_at_t512": self_us, "self_attn_GBs": self_bytes / (self_us * 1e-6) / 1e9,
               "self_attn_frac": self_bytes / (self_us * 1e-6) / 1e9 / HBM_PEAK_GBS,
               "launch_set": f"{Bn} clips = 2 co-scheduled chain launches of {Bn // 2} clips (dec_attn_mc_kernel, 4 clips of one head per workgroup)"}
    del x
    return {"kernels": kernels, "workload": f"reference-native geometry: {Bn} segments x {Tn} samples (3 s @ 16 kHz, S={Sn}), {'bf16' if esize == 2 else 'fp32'}, max_length {MAX_LENGTH}",
            "tokens_per_s": Bn * n_steps / dt, "ms_per_batch": dt * 1e3, "new_tokens_per_clip": int(n_steps),
            "step_algorithmic_bytes": step_bytes, "step_mean_us": step_us, "step_achieved_GBs": step_bytes / (step_us * 1e-6) / 1e9,
            "step_frac": step_bytes / (step_us * 1e-6) / 1e9 / HBM_PEAK_GBS,
            "note": f"step bytes = decoder weights {DEC_PARAMS_PER_STEP * esize / 1e6:.1f} MB + 128 clips x {6144 * esize} B x (190 + mean t) (SURVEY 8d formula at this geometry)"}


def decode_roofline_record(model, x, B: int, S: int, es: int, precision: str, enc_ms: float) -> dict:
    """`roofline` of the decode path of `model` (any precision) on the encoder inputs x: the dominant kernel (decode cross-attention)
    timed live with hipEvents on the streams it runs on (m2m_bench_kernel: every chain's launch on its own stream, 600 launch sets
    cycling the 6 layers), algorithmic bytes with the precision's element size (es = 2: bf16 weights and K/V; 4: fp32), traffic
    from the newest committed PMC summary of that precision, and the whole path's fraction from one timed greedy decode."""
    from music2midi_amd import native
    dev = x.device
    t_dec = time.perf_counter()
    model.generate_from_embeds(x, max_length=MAX_LENGTH)
    torch.cuda.synchronize(dev)
    t_dec = time.perf_counter() - t_dec
    t_mid = MAX_LENGTH // 2
    model._encode(x, MAX_LENGTH)      # a greedy decode that re-packed its live rows has consumed the encode (m2m_generate_greedy)
    cross_us, cross_bytes = model.bench_kernel(native.KERNEL_DEC_CROSS_ATTN, t_mid, 600)
    self_us, self_bytes = model.bench_kernel(native.KERNEL_DEC_SELF_ATTN, t_mid, 600)
    step_us, _ = model.bench_kernel(native.KERNEL_DEC_STEP, t_mid, 200)
    achieved = cross_bytes / (cross_us * 1e-6) / 1e9
    # whole decode loop: mean algorithmic bytes per step (t averaged over the run) / mean measured step
    n_steps = MAX_LENGTH - 1
    mean_step_us = (t_dec - enc_ms * 1e-3) / n_steps * 1e6
    step_bytes = decode_bytes_per_step(B, S, (1 + n_steps) / 2.0, es)
    step_gbs = step_bytes / (mean_step_us * 1e-6) / 1e9
    n_chains = 2 if B >= 24 and not os.environ.get("M2M_GROUP_ROWS") else max(1, -(-B // int(os.environ.get("M2M_GROUP_ROWS") or B)))
    tname = "m2m::bf16_t" if precision == "bf16" else "float"
    return {"roofline": {"bound": "hbm", "kernel": f"dec_attn_kernel<{tname}> (cross-attention, decode step)",
                         "launch": f"{n_chains} co-scheduled chain launches of {B // n_chains} clips each (as the decode loop issues them) = {B} clips",
                         "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS,
                         "traffic": pmc_traffic_bytes(f"dec_attn_kernel<{tname}, false,", B, precision=precision),
                         "algorithmic_bytes_per_launch": cross_bytes, "avg_launch_us": cross_us,
                         # the PATH's fraction (all 19 kernels of a decode step, averaged over the 1023 steps of a run):
                         "step_frac": step_gbs / HBM_PEAK_GBS, "step_achieved": step_gbs,
                         "step_algorithmic_bytes": step_bytes, "step_mean_us": mean_step_us},
            "generate_from_embeds_s": t_dec, "self_attn_us_at_t512": self_us, "self_attn_GBs": self_bytes / (self_us * 1e-6) / 1e9,
            "decode_step_us_at_t512": step_us}


def decode_bytes_per_step(B: int, S: int, t_mean: float, esize: int) -> float:
    """Algorithmic HBM bytes of one decode step: the decoder weights once for the whole
    batch + per clip the cross K/V (6 layers x 2 x 512 x S) and the self K/V cache up to position t."""
    return DEC_PARAMS_PER_STEP * esize + B * 6 * 2 * 512 * (S + t_mean) * esize


# ------------------------------------------------------------------ dry mode (launcher + collectives on CPU)
def dry_run(args):
    from music2midi_amd import distributed as D
    from music2midi_amd.config import T5Geometry, default_config
    from music2midi_amd.transformer import T5Transformer

    os.environ.setdefault("M2M_DIST_BACKEND", "gloo")
    rank, local_rank, world = D.init_process_group("gloo")
    if os.environ.get("M2M_BENCH_FAIL_RANK") == str(rank):      # test hook: a rank that dies must fail the whole launch
        sys.exit(3)
    if os.environ.get("M2M_BENCH_HANG_RANK") == str(rank):      # test hook: a rank that never finishes must trip the watchdog
        print(f"[bench] rank {rank}: hanging on purpose (test hook)", file=sys.stderr, flush=True)
        time.sleep(3600)
    pin_host_threads(world)
    if args.mode == "train":
        return dry_run_train(args, rank, world)
    cfg = default_config()
    geom = T5Geometry(cfg.model.t5)
    torch.manual_seed(1234 + rank)                      # ranks start from DIFFERENT weights ...
    model = T5Transformer(cfg.to_dict(), precision=args.precision)
    bcast = D.broadcast_module_state(model, src=0)      # ... and must all end up with rank 0's
    # first-multi-GPU-run insurance: MIN / MAX all-reduce of a 64-bit checksum of every rank's replica, raising on a
    # difference; M2M_BENCH_CORRUPT_RANK (test hook) flips one weight on one rank AFTER the broadcast to prove the check bites
    if os.environ.get("M2M_BENCH_CORRUPT_RANK") == str(rank):
        with torch.no_grad():
            model.transformer.lm_head.weight[3, 5] += 1.0
    try:
        replicas = D.verify_replicas({"masters_fp32": D.module_checksum(model), "as_bf16_repack": D.module_checksum(model, torch.bfloat16)}, "cpu")
    except RuntimeError as e:
        print(f"[bench] rank {rank}: {e}", file=sys.stderr, flush=True)
        sys.exit(4)
    per_rank_ms = D.all_gather_floats(1.0 + rank, "cpu")
    probe = float(model.transformer.lm_head.weight.double().sum())
    B = args.batch
    lo = rank * B
    toks = (torch.arange(B * 4).reshape(B, 4) + 1000 * lo)
    allt = D.all_gather_tokens(toks, args.max_length, geom.pad_token_id)
    ok = allt.shape == (B * world, 4) and all(int(allt[r * B, 0]) == 1000 * r * B for r in range(world))
    pmin, pmax = -D.all_reduce_max(-probe, "cpu"), D.all_reduce_max(probe, "cpu")
    D.barrier()
    if rank == 0:
        print(json.dumps({"metric": "decoded MIDI tokens/sec/node on 10 s clips", "value": 0.0, "unit": "tokens/s",
                          "n_gpus": world, "dry_run": True, "backend": torch.distributed.get_backend() if world > 1 else "none",
                          "world": torch.distributed.get_world_size() if world > 1 else 1,
                          "gather_ok": bool(ok), "weights_identical_on_all_ranks": pmin == pmax,
                          "ranks_seen": replicas["ranks_seen"], "replica_checksums": replicas["checksums"],
                          "per_rank_ms_per_step": per_rank_ms,
                          "config": {"weight_broadcast_bytes": bcast, "global_batch": B * world}}), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()
    return 0 if ok and pmin == pmax and replicas["ranks_seen"] == world and per_rank_ms == [1.0 + r for r in range(world)] else 1


def dry_run_train(args, rank: int, world: int) -> int:
    """--mode train --dry-run: the data-parallel plumbing of a training step on CPU tensors over gloo — the flat-gradient
    average in one piece and in the overlapped form's four pieces (two early ranges of the real SIZES — shared embedding + lm_head,
    the decoder blocks — at stand-in offsets: the native trainer's own layout needs the GPU library; what is exercised here is
    the splitting, the averaging and the byte count), the sync_dist metric reduction, barrier + max-over-ranks timing — no GPU work."""
    from music2midi_amd import distributed as D
    from music2midi_amd.config import default_config
    from music2midi_amd.transformer import T5Transformer
    cfg = default_config()
    model = T5Transformer(cfg.to_dict(), precision="fp32")
    n = sum(p.numel() for p in model.parameters())
    # early ranges of the native trainer's sizes ([shared + lm_head] in front, the decoder blocks as one block further back)
    n_front = model.transformer.shared.weight.numel() + model.transformer.lm_head.weight.numel()
    n_dec = sum(p.numel() for p in model.transformer.decoder.block.parameters())
    early = [(0, n_front), (n - n_dec - 4096, n_dec)]
    g = torch.Generator().manual_seed(99)
    base = torch.randn(n, generator=g)
    t0 = time.perf_counter()
    flat = base * (rank + 1)
    b1 = D.all_reduce_gradients(flat)
    want = base * (sum(range(1, world + 1)) / world)
    ok = torch.allclose(flat, want, rtol=1e-6, atol=1e-6)
    flat = base * (rank + 1)
    b2 = D.all_reduce_gradients_overlapped(flat, early, None)
    ok = ok and torch.allclose(flat, want, rtol=1e-6, atol=1e-6) and b1 == b2 == (n * 4 if world > 1 else 0)
    logged = D.reduce_logged({"train/loss": torch.tensor(1.0 + rank), "train/score": 0.25 * rank, "batch_size": 16})
    ok = ok and abs(logged["train/loss"] - (1.0 + (world - 1) / 2)) < 1e-12 and logged["batch_size"] == 16 * world
    D.barrier()
    dt_local = time.perf_counter() - t0
    per_rank = D.all_gather_floats(dt_local, "cpu")
    dt = D.all_reduce_max(dt_local, "cpu")
    # the N > 1 fields of the real line: the averaged "parameters" must checksum alike on every rank (a test hook spoils one rank's)
    if os.environ.get("M2M_BENCH_CORRUPT_RANK") == str(rank):
        flat[0] += 1.0
    after = D.verify_replicas({"params_after_steps": D.tensor_checksum(flat)}, "cpu")
    if rank == 0:
        print(json.dumps({"metric": "training clips/sec/node (forward+backward+Adafactor step)", "value": 0.0, "unit": "clips/s", "n_gpus": world,
                          "dry_run": True, "mode": "train", "backend": torch.distributed.get_backend() if world > 1 else "none",
                          "world": torch.distributed.get_world_size() if world > 1 else 1, "grad_allreduce_bytes": b1,
                          "grad_average_ok": bool(ok), "logged": logged, "host_threads": torch.get_num_threads(), "wall_s": dt,
                          "ranks_seen": after["ranks_seen"], "replica_checksums": after["checksums"], "per_rank_ms_per_step": [e * 1e3 for e in per_rank],
                          "grad_allreduce_bytes_per_step": b1,
                          "config": {"global_batch": 16 * world, "parallelism": f"data-parallel x{world}"}}), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()
    return 0 if ok else 1


# ------------------------------------------------------------------ BASELINE configs[4]: training step
TRAIN_SAMPLES = 66150      # ref config.yaml: 3 s segments at dataset.sample_rate 22 050 Hz -> 259 frames, S = 261
TRAIN_LABELS = 256         # label tokens per clip (synthetic, none ignored)


def train_profile_summary(profiles_dir=None):
    """Launches per step and the share of a step's GPU time that is NOT a matrix product, from the newest committed rocprofv3
    kernel-stats summary of the training step (profiles/r*_train_dropout_kernel_stats.csv: `tools/train_gap.py` — the same
    16-clip / S = 261 / 256-label / dropout 0.1 step, directly issued so that every kernel is a launch of its own — under
    `rocprofv3 --kernel-trace --stats`).  Product kernels = names containing gemm / dw_group / attn_stripe / attn_head (projections, batched
    attention products, weight gradients, the attention kernels of either generation); everything else is row / element-wise work.  {} when no
    summary is committed."""
    import csv
    files = sorted(Path(profiles_dir or ROOT / "profiles").glob("*train_dropout_kernel_stats.csv"), key=lambda f: (_round_of(f.name), f.name))
    if not files:
        return {}
    rows = list(csv.DictReader(open(files[-1])))
    steps = next((int(r["Calls"]) for r in rows if "train_prologue_kernel" in r["Name"] or "step_key_kernel" in r["Name"]), 0)      # one per pass
    if not steps:
        return {}
    tot = sum(float(r["TotalDurationNs"]) for r in rows) / steps / 1e3
    gemm = sum(float(r["TotalDurationNs"]) for r in rows if any(k in r["Name"] for k in ("gemm", "dw_group", "attn_stripe", "attn_head"))) / steps / 1e3
    return {"launches_per_step": round(sum(int(r["Calls"]) for r in rows) / steps, 1), "kernel_us_per_step": round(tot, 1),
            "non_gemm_us": round(tot - gemm, 1), "profile": files[-1].name}


def cpu_train_baseline(cfg, state, B: int, threads: int = 16):
    """The CPU side of configs[4]: the oracle's training step on the host — autograd forward + backward over oracle/train.py and
    the restated Adafactor — on the same shape (B clips, S = 261, 256 labels), fp32."""
    from music2midi_amd import synth
    from music2midi_amd.config import T5Geometry
    from oracle.train import AdafactorOracle, T5TrainOracle, leaf_params
    geom = T5Geometry(cfg.model.t5)
    threads = min(threads, os.cpu_count() or threads)
    torch.set_num_threads(threads)
    F = 1 + TRAIN_SAMPLES // 256
    params = leaf_params(state)
    orc, opt = T5TrainOracle(geom, params), AdafactorOracle(params)
    feats = torch.from_numpy(synth.normal(5, "feats", (B, F, geom.d_model), 2.0))
    cond = torch.from_numpy(synth.cond_index_batch(0, B))
    labels = torch.from_numpy((synth.uniform01(0, "train_labels", B * TRAIN_LABELS) * 330).astype(np.int64).reshape(B, TRAIN_LABELS)) + 3
    t0 = time.perf_counter()
    loss, _, grads = orc.loss_and_grads(feats, cond, labels)
    opt.step(grads)
    dt = time.perf_counter() - t0
    return {"value": B / dt, "unit": "clips/s", "ms_per_step": dt * 1e3, "cores": threads, "kind": "port",
            "sample": f"ONE step: {B} clips x S={F + 2} x {TRAIN_LABELS} labels, fp32 torch-CPU autograd over the oracle + restated Adafactor "
                      f"(log-mel excluded), {dt:.1f} s wall, {threads} threads", "loss": float(loss)}


def train_step_record(model_module, cfg, geom, dev, B: int, precision: str, steps: int, warmup: int, world: int = 1, dropout: float = 0.0,
                      profile_launches: bool = False, dump: dict = None):
    """forward + backward + (gradient all-reduce) + Adafactor on B clips per GPU; returns a dict for the JSON line.
    With ``dump`` (a dict), the last timed step's results go into it: the loss and fixed samples of the weights and gradients."""
    from music2midi_amd import distributed as D
    from music2midi_amd import synth
    from music2midi_amd.input import ModelInputs
    from music2midi_amd.training import NativeTrainer
    rank = D.env_world()[0]
    F = 1 + TRAIN_SAMPLES // 256
    wav = torch.from_numpy(synth.waveform_batch(rank * B, B, TRAIN_SAMPLES)).to(dev)
    cond = torch.from_numpy(synth.cond_index_batch(rank * B, B)).to(dev)
    labels = (torch.from_numpy((synth.uniform01(rank, "train_labels", B * TRAIN_LABELS) * 330).astype(np.int64)
                               .reshape(B, TRAIN_LABELS)) + 3).to(dev)
    tr = NativeTrainer(model_module, B, F + 2, TRAIN_LABELS, precision=precision)
    if dropout > 0.0:      # T5Config.dropout_rate as the reference trains (train() mode, ref: train.py:33): masks from the counter-based hash, regenerated in the backward pass
        tr.set_dropout(dropout, seed=1)
    overlap = (world > 1 and os.environ.get("M2M_DP_OVERLAP", "1") != "0") or os.environ.get("M2M_DP_OVERLAP") == "force"   # force: the split pass on one rank
    if overlap:          # decoder-side gradients are all-reduced on their own stream while the encoder-side backward runs
        tr.set_sync_stream(torch.cuda.Stream(device=dev))

    def step():
        x = model_module.encoder_inputs(ModelInputs(input_waveform=wav, cond_index=cond))     # frontend kernel, every step
        loss, _ = tr.forward_backward(x, cond, labels)
        nbytes = (D.all_reduce_gradients_overlapped(tr.grads, tr.early_ranges, tr.sync_stream) if overlap
                  else D.all_reduce_gradients(tr.grads))
        tr.optimizer_step()
        return loss, nbytes

    for _ in range(max(1, warmup)):
        loss, nbytes = step()
    D.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        loss, nbytes = step()
    torch.cuda.synchronize(dev)
    D.barrier()
    dt_local = time.perf_counter() - t0
    if dump is not None:
        dump["loss"] = np.array([float(loss)], dtype=np.float64)
        dump["params_sample"] = dump_sample(tr.params)
        dump["grads_sample"] = dump_sample(tr.grads)
    per_rank_ms = [e / steps * 1e3 for e in D.all_gather_floats(dt_local, dev)]
    dt = D.all_reduce_max(dt_local, dev) / steps
    # every rank trained on ITS clips: after these steps the replicas are identical only if the gradient average reached every rank
    after = D.verify_replicas({"params_after_steps": D.tensor_checksum(tr.params)}, dev) if world > 1 else None
    S = F + 2
    enc = 6 * (4227072 * S + 2048 * S * S) + 4718592 * S
    dec = TRAIN_LABELS * (6 * (2 * 384 * 512 * 6 + 3 * 2 * 384 * 1152) + 2 * 384 * 400) + 6 * (4 * TRAIN_LABELS * TRAIN_LABELS * 512 + 4 * TRAIN_LABELS * S * 512)
    flops = 3 * B * (enc + dec)                                    # forward + 2x backward, dense products only (SURVEY 8d formulas)
    peak = MFMA_PEAK_TFLOPS["fp8" if precision == "fp8" else "bf16"]
    rec = {"workload": f"BASELINE configs[4]: train step (log-mel + forward + backward + Adafactor), {precision} GEMM inputs, "
                       f"{B} clips/GPU x {TRAIN_SAMPLES} samples (S={S}), {TRAIN_LABELS} labels/clip, dropout {'off' if dropout == 0.0 else dropout}"
                       + ("; NOTE: at this per-GPU batch the MXFP8 mode is SLOWER than bf16 (4.7 vs 3.9 ms: the products are latency-bound, 8-15 % matrix-core busy)"
                          if precision == "fp8" else ""),
           "ms_per_step": dt * 1e3, "clips_per_s": B * world / dt, "label_tokens_per_s": B * world * TRAIN_LABELS / dt,
           "model_TFLOPs_per_gpu": flops / dt / 1e12, "loss": float(loss), "grad_allreduce_bytes": nbytes,
           "roofline": {"bound": "mfma", "flops_per_step": flops, "achieved": flops / dt / 1e12, "peak": peak, "unit": "TFLOP/s",
                        "frac": flops / dt / 1e12 / peak, "peak_note": f"dense {'MXFP8' if precision == 'fp8' else 'bf16'} MFMA peak (MI355X_MICROARCH.md)",
                        "graph_nodes_per_step": tr.graph_nodes()},
           "optimizer": "Adafactor(warmup_init=True), native", "world": world,
           "grad_allreduce": ("4 pieces, decoder side overlapped with the encoder backward" if overlap else "one call behind the pass") if world > 1 else
                             ("none (split pass forced)" if overlap else "none")}
    if world == 1 and profile_launches:
        rec["roofline"].update(train_profile_summary())
    if world > 1:
        rec["per_rank_ms_per_step"] = per_rank_ms
        rec["replicas_after_steps"] = after
    tr.close()
    return rec


def train_surface_record(cfg, state, dev, B: int, steps: int, warmup: int):
    """The same step through the CLASS surface a reference-shaped trainer calls (ref model.py:27-43, train.py:40-41):
    ``Music2MIDI.training_step`` (host tokenisation of the notes as ref model.py:33 does it per step, log-mel, forward + backward
    enqueued, loss left on the device) + ``optimizer.step()``, driven by ``fit_batches`` — no host synchronisation inside the loop."""
    from music2midi_amd import synth
    from music2midi_amd.checkpoint import load_t5_state
    from music2midi_amd.input import ModelInputs
    from music2midi_amd.model import Music2MIDI
    c = cfg.to_dict()
    c["dataloader"]["batch_size"] = B
    c["trainer"]["log_every_n_steps"] = 10 ** 9            # the periodic train/score (a greedy decode) is not part of a step
    m = Music2MIDI(c)
    load_t5_state(m.model, state, strict=False)
    m = m.to(dev)
    m.train_precision = "bf16"
    m.train()
    notes = []
    for b in range(B):                                      # ~54 notes in 3 s per clip: 256 label positions after bucketing, as the main record
        n = 52 + (7 * b) % 4
        u = synth.uniform01(300 + b, "surface_notes", n * 3).reshape(n, 3)
        on = np.sort(u[:, 0] * 2.8)
        notes.append(np.stack([on, on + 0.05 + u[:, 1] * 0.3, np.floor(40 + u[:, 2] * 40), np.full(n, 80.0)], axis=1))
    wav = torch.from_numpy(synth.waveform_batch(0, B, TRAIN_SAMPLES)).to(dev)
    cond = torch.from_numpy(synth.cond_index_batch(0, B)).to(dev)
    batch = ModelInputs(input_waveform=wav, notes_batch=tuple(notes), cond_index=cond)
    opt = m.configure_optimizers()[0][0]
    m.fit_batches([batch] * max(2, warmup), optimizer=opt)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    losses = m.fit_batches([batch] * steps, optimizer=opt)
    torch.cuda.synchronize(dev)
    dt = (time.perf_counter() - t0) / steps
    t1 = time.perf_counter()
    for _ in range(20):
        labels = m._labels(batch.notes_batch)
    tok = (time.perf_counter() - t1) / 20
    rec = {"ms_per_step": dt * 1e3, "clips_per_s": B / dt, "label_positions": int(labels.shape[1]), "host_tokenizer_ms_per_step": tok * 1e3,
           "loss_first_last": [losses[0], losses[-1]],
           "what": "Music2MIDI.fit_batches over one repeated batch: training_step (notes tokenised on the host every step as ref model.py:33, log-mel, "
                   "forward + backward enqueued, device-resident loss) + Adafactor step; bf16, dropout 0.1 (train() mode); no host sync inside the loop"}
    if m._trainer is not None:
        m._trainer.close()
    return rec



# ------------------------------------------------------------------ main
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32", "fp8"],
                    help="fp8 (block-scaled MXFP8 projection GEMMs) exists for --mode train only")
    ap.add_argument("--batch", type=int, default=32, help="clips per GPU")
    ap.add_argument("--cpu-tokens", type=int, default=1023, help="greedy steps per clip of the CPU baseline sample (0 = skip)")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-parity", action="store_true", help="skip the fp32 parity-mode record")
    ap.add_argument("--no-frontend", action="store_true", help="skip the configs[1] frontend record")
    ap.add_argument("--no-native", action="store_true", help="skip the reference-native-geometry and ragged-EOS records")
    ap.add_argument("--mode", default="generate", choices=["generate", "train"],
                    help="train: BASELINE configs[4] (forward+backward+Adafactor, 16 clips/GPU, gradient all-reduce over RCCL)")
    ap.add_argument("--no-train", action="store_true", help="skip the configs[4] training-step record of the --full line")
    ap.add_argument("--dropout", type=float, default=0.1, help="--mode train: T5Config.dropout_rate of the step (0.1: what the reference's train() mode runs; 0 = off)")
    ap.add_argument("--dry-run", action="store_true", help="launcher + collectives on CPU tensors (gloo), no GPU work")
    ap.add_argument("--max-length", type=int, default=MAX_LENGTH,
                    help="decoder max_length (profiling runs only; the headline number uses 1024)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last step's outputs as DIR/<name>.npy (rank 0; at most 64 MB)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also the records beside it (N = 1): roofline and phase timings, configs[1] frontend, "
                         "reference-native geometry and ragged EOS, fp32 parity mode, configs[4] training step, CPU baselines")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: become the launcher (no HIP call has happened in this process)
        sys.exit(spawn_ranks(args.gpus))
    if args.dry_run:
        sys.exit(dry_run(args))

    from music2midi_amd import distributed as D
    from music2midi_amd import native, synth
    from music2midi_amd.checkpoint import load_t5_state
    from music2midi_amd.config import T5Geometry, default_config
    from music2midi_amd.input import ModelInputs
    from music2midi_amd.transformer import T5Transformer

    rank, local_rank, world = D.env_world()
    if world > torch.cuda.device_count() and os.environ.get("M2M_DIST_BACKEND", "nccl") == "nccl":
        print(f"[bench] WORLD_SIZE={world} but only {torch.cuda.device_count()} GPU(s) visible: RCCL needs one GPU per rank",
              file=sys.stderr)
        sys.exit(2)
    rank, local_rank, world = D.init_process_group()
    if world != args.gpus:
        if rank == 0:
            print(f"[bench] --gpus {args.gpus} but WORLD_SIZE={world}: reporting n_gpus={world}", file=sys.stderr)
        args.gpus = world
    native.require_gpu()
    dev = torch.device("cuda", local_rank % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    pin_host_threads(world)

    cfg = default_config()
    geom = T5Geometry(cfg.model.t5)
    B = args.batch
    S = N_FRAMES + 2

    # ---- weights: rank 0 owns them, everyone else receives them over RCCL ----
    model = T5Transformer(cfg.to_dict(), precision="bf16" if args.precision == "fp8" else args.precision)
    state = None
    if rank == 0:
        state = synth.t5_state_dict(geom, seed=0)
        load_t5_state(model, state, strict=False)
    model = model.to(dev).eval()
    # inference in the bf16 mode: the GEMM weights travel as bf16 (61 MB, SURVEY C4's figure); training and the fp32 mode need the masters
    bf16_bcast = args.mode != "train" and args.precision == "bf16" and os.environ.get("M2M_BCAST_FP32") != "1"
    bcast_bytes = D.broadcast_module_state(model, src=0, gemm_dtype=torch.bfloat16 if bf16_bcast else None)
    replicas = None
    if world > 1:
        # first-multi-GPU-run insurance: every rank's REPACKED device weights (the bytes the kernels read) and its torch-side replica
        # must checksum alike — MIN / MAX all-reduce, a difference raises on every rank before anything is timed
        sums = {"torch_replica": D.module_checksum(model, torch.bfloat16 if bf16_bcast else None)}
        if args.mode != "train":
            sums["device_repacked"] = model.device_weights_checksum()
        replicas = D.verify_replicas(sums, dev)

    if args.precision == "fp8" and args.mode != "train":
        print("[bench] --precision fp8 is a training mode (use --mode train)", file=sys.stderr)
        sys.exit(2)
    if args.mode == "train":
        Bt = 16 if args.batch == 32 else args.batch
        dumped = {} if args.dump_outputs else None
        rec = train_step_record(model, cfg, geom, dev, Bt, args.precision, args.steps, args.warmup, world, dropout=args.dropout, dump=dumped)
        if rank == 0 and args.dump_outputs:
            dump_outputs(args.dump_outputs, dumped)
        if rank == 0:
            line = {"metric": "training clips/sec/node (forward+backward+Adafactor step)", "value": rec["clips_per_s"], "unit": "clips/s",
                    "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": rec["ms_per_step"],
                    "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.precision, "data": "synthetic",
                    "config": {"workload": rec["workload"], "global_batch": Bt * world, "parallelism": f"data-parallel x{world}",
                               "grad_allreduce_bytes": rec["grad_allreduce_bytes"]}, "extras": rec}
            if world > 1:     # as the generate line: proof that the collectives saw N ranks, with identical replicas before AND after the steps
                line["ranks_seen"] = replicas["ranks_seen"]
                line["replica_checksums"] = dict(replicas["checksums"], **rec["replicas_after_steps"]["checksums"])
                line["per_rank_ms_per_step"] = rec["per_rank_ms_per_step"]
                line["grad_allreduce_bytes_per_step"] = rec["grad_allreduce_bytes"]
            print(json.dumps(line), flush=True)
        if world > 1:
            torch.distributed.destroy_process_group()
        return

    # ---- synthetic clips of this rank, resident in HBM ----
    first = rank * B
    wav = torch.from_numpy(synth.waveform_batch(first, B, N_SAMPLES)).to(dev)
    cond = torch.from_numpy(synth.cond_index_batch(first, B)).to(dev)
    inputs = ModelInputs(input_waveform=wav, cond_index=cond)

    def step():     # each rank decodes its own 32 clips (weak scaling), ids all-gathered into global clip order
        toks = model.generate(inputs, max_length=args.max_length)
        return D.all_gather_tokens(toks, args.max_length, geom.pad_token_id)

    for _ in range(args.warmup):
        step()
    if world > 1:   # communicator set-up must never land in the timed region (even with --warmup 0)
        D.all_gather_tokens(torch.zeros((B, 2), dtype=torch.long, device=dev), args.max_length, geom.pad_token_id)
        D.all_reduce_max(0.0, dev)
        D.all_reduce_sum(0.0, dev)
    D.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        toks = step()
    torch.cuda.synchronize(dev)
    D.barrier()
    elapsed = time.perf_counter() - t0
    per_rank_ms = [e / args.steps * 1e3 for e in D.all_gather_floats(elapsed, dev)]
    elapsed = D.all_reduce_max(elapsed, dev)
    assert toks.shape[0] == B * world, toks.shape
    if rank == 0 and args.dump_outputs:      # the all-gathered greedy ids of the last timed step, every rank's clips
        dump_outputs(args.dump_outputs, {"tokens": toks.cpu().numpy()})
    # tokens that count: per clip, up to and including its EOS, or the whole budget when it has none.  (Random-init weights emit EOS
    # now and then; the headline clips' trajectories have had none so far — `rows_with_eos` says so in the line — but a row that ends
    # early costs less from there on (finished-row early-out), so padding must never be counted as decoded tokens.)
    is_eos = toks[:, 1:] == geom.eos_token_id
    has_eos = is_eos.any(dim=1)
    useful = torch.where(has_eos, is_eos.float().argmax(dim=1) + 1, torch.full_like(has_eos, toks.shape[1] - 1, dtype=torch.long))
    rows_with_eos = int(has_eos.sum())
    total_tokens = float(useful.sum()) * args.steps        # `toks` is the all-gathered matrix: every rank's clips

    out = None
    es = 2 if args.precision == "bf16" else 4
    if rank == 0:
        value = total_tokens / elapsed
        out = {
            "metric": "decoded MIDI tokens/sec/node on 10 s clips",
            "value": value, "unit": "tokens/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": args.precision, "data": "synthetic",
            "config": {"workload": "BASELINE configs[2]: full generate (log-mel + encoder + KV-cached greedy decode), "
                                   f"{args.precision}, batch {B} clips/GPU x {N_SAMPLES} samples, S={S}, max_length {args.max_length}"
                                   + (f"; configs[3] sharding over {world} GPUs" if world > 1 else ""),
                       "precision_note": ("throughput mode: bf16 GEMM inputs and K/V caches; its ids follow a bf16-emulating oracle and equal the "
                                          "fp32 CPU reference's on 54-61 % of the tokens (rounds 4-5; this run's figure replaces this text when the "
                                          "parity-mode record runs: parity_mode.bf16_vs_fp32_id_agreement); the mode with "
                                          "bit-exact greedy ids is fp32: parity_mode.tokens_per_s") if args.precision == "bf16" else
                                         "fp32 parity mode: greedy ids bit-identical to the fp32 CPU reference",
                       "global_batch": B * world, "clips_per_gpu": B, "new_tokens_per_clip": toks.shape[1] - 1,
                       "rows_with_eos": rows_with_eos, "counted_tokens_per_step": int(useful.sum()),
                       "parallelism": f"clip-sharded x{world}", "weight_broadcast_bytes": bcast_bytes,
                       "weight_broadcast_dtype": ("GEMM weights bf16 + embeddings / norms / tables fp32 (receivers repack bit-identically)" if bf16_bcast
                                                  else "fp32 master weights (each rank repacks locally)"),
                       "world": torch.distributed.get_world_size() if world > 1 else 1,
                       "backend": torch.distributed.get_backend() if world > 1 else "none"},
        }
        if world > 1:     # proof that the collectives saw N ranks with identical replicas, and each rank's own clock
            out["ranks_seen"] = replicas["ranks_seen"]
            out["replica_checksums"] = replicas["checksums"]
            out["per_rank_ms_per_step"] = per_rank_ms

    # ---- --full: the records beside the headline (rank 0 only, N = 1), each after the timed steps ----
    full = rank == 0 and world == 1 and args.full

    # ---- phase timings + roofline of the dominant kernel ----
    if full and not args.no_roofline:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        x = model.encoder_inputs(inputs)
        ev[1].record()
        sess, _ = model._encode(x, MAX_LENGTH)
        ev[2].record()
        torch.cuda.synchronize(dev)
        fe_ms = ev[0].elapsed_time(ev[1])
        enc_first_ms = ev[1].elapsed_time(ev[2])          # one call, as rounds 1-4 reported it (host issue of ~60 launches included)
        for _ in range(3):                                 # warm-up: the first passes after other work run ~10 % slower
            model._encode(x, MAX_LENGTH)
        ev[1].record()
        for _ in range(ENC_PASSES):                        # mean of warm back-to-back passes (tools/enc_sustained.py: 1.81 ms over 50-500)
            model._encode(x, MAX_LENGTH)
        ev[2].record()
        torch.cuda.synchronize(dev)
        enc_ms = ev[1].elapsed_time(ev[2]) / ENC_PASSES
        # dominant kernel: decode cross-attention (6 launches per decode step, streams the
        # per-clip cross K/V: 2 * S * inner * esize bytes per clip per launch)
        rr = decode_roofline_record(model, x, B, S, es, args.precision, enc_ms)
        out["roofline"] = rr["roofline"]
        out["extras"] = {
            "frontend_ms": fe_ms, "encoder_plus_crosskv_ms": enc_ms, "encoder_plus_crosskv_single_call_ms": enc_first_ms,
            "encoder_TFLOPs": B * 35.17e9 / (enc_ms * 1e-3) / 1e12,
            "generate_from_embeds_s": rr["generate_from_embeds_s"],
            "self_attn_us_at_t512": rr["self_attn_us_at_t512"], "self_attn_GBs": rr["self_attn_GBs"],
            "decode_step_us_at_t512": rr["decode_step_us_at_t512"],
            "frontend_GBs": B * (4 * N_SAMPLES + 4 * N_FRAMES * 384) / (fe_ms * 1e-3) / 1e9,
        }

    # ---- BASELINE configs[1]: the log-mel kernel alone, 64 clips, beside torch.stft on the host ----
    if full and not args.no_frontend:
        Bf = 64
        wav64 = torch.from_numpy(synth.waveform_batch(0, Bf, N_SAMPLES)).to(dev)
        buf = torch.empty((Bf, N_FRAMES, geom.d_model), device=dev, dtype=torch.float32)
        for _ in range(3):
            model.spectrogram.forward_into(wav64, buf, 0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        iters = 50
        e0.record()      # the frontend is launched on torch's current stream, so torch events bracket it
        for _ in range(iters):
            model.spectrogram.forward_into(wav64, buf, 0)
        e1.record()
        torch.cuda.synchronize(dev)
        us = e0.elapsed_time(e1) * 1e3 / iters
        nbytes = Bf * (4 * N_SAMPLES + 4 * N_FRAMES * 384)
        rec = {"workload": f"BASELINE configs[1]: STFT + log-mel kernel only, batch {Bf} x {N_SAMPLES} samples",
               "us_per_launch": us, "clips_per_s": Bf / (us * 1e-6), "algorithmic_bytes": nbytes,
               "achieved_GBs": nbytes / (us * 1e-6) / 1e9, "hbm_frac": nbytes / (us * 1e-6) / 1e9 / HBM_PEAK_GBS,
               "fp32_TFLOPs": Bf * 56.8e6 / (us * 1e-6) / 1e12, "valu_frac_of_157TF": Bf * 56.8e6 / (us * 1e-6) / 157e12}
        if args.cpu_tokens > 0:
            rec["cpu_torch_stft"] = cpu_frontend_baseline(cfg, Bf)
            rec["gpu_over_cpu"] = rec["cpu_torch_stft"]["ms_per_batch"] * 1e3 / us
        out["frontend_configs1"] = rec
        del wav64, buf

    # ---- the reference's own geometry (128 x 3 s segments) and a batch whose rows END (finished-row early-out) ----
    if full and not args.no_native and args.precision == "bf16":
        out["reference_native"] = reference_native_record(model, cfg, geom, dev)
        out["ragged_eos"] = ragged_eos_record(cfg, geom, dev, B, S)
        out["ragged_eos_native"] = ragged_eos_record(cfg, geom, dev, int(cfg.inference.batch_size),
                                                     1 + int(cfg.model.sample_rate * cfg.dataset.segment_duration) // 256 + 2)

    # ---- parity mode: fp32 (bit-exact against the fp32 reference) on the same workload ----
    if full and not args.no_parity and args.precision == "bf16":
        ids_bf16 = model.generate(inputs, max_length=MAX_LENGTH)
        m32 = T5Transformer(cfg.to_dict(), precision="fp32")
        load_t5_state(m32, state, strict=False)
        m32 = m32.to(dev).eval()
        ids_fp32 = m32.generate(inputs, max_length=MAX_LENGTH)   # warm-up + ids
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        reps = 2
        for _ in range(reps):
            m32.generate(inputs, max_length=MAX_LENGTH)
        torch.cuda.synchronize(dev)
        dt32 = (time.perf_counter() - t1) / reps
        L = min(ids_bf16.shape[1], ids_fp32.shape[1])
        same = (ids_bf16[:, 1:L] == ids_fp32[:, 1:L])
        first_div = [int((~row).nonzero()[0, 0]) + 1 if not bool(row.all()) else -1 for row in same]
        prefix = [(d - 1 if d > 0 else L - 1) for d in first_div]
        out["parity_mode"] = {
            "dtype": "fp32", "tokens_per_s": B * (ids_fp32.shape[1] - 1) / dt32, "ms_per_step": dt32 * 1e3,
            "note": "fp32 mode = greedy ids bit-identical to the fp32 reference (tests/test_golden_gpu.py); same workload",
            "bf16_vs_fp32_id_agreement": float(same.float().mean()),
            "bf16_vs_fp32_rows_identical": int(sum(1 for d in first_div if d < 0)),
            "bf16_vs_fp32_first_divergence_step": first_div,
            "bf16_vs_fp32_mean_identical_prefix": float(np.mean(prefix)),
        }
        # the DEFAULT mode of the Python classes (what evaluate.py gets) against its own roofline: fp32 byte counts (4-byte K/V and weights)
        if not args.no_roofline:
            x32 = m32.encoder_inputs(inputs)
            for _ in range(2):
                m32._encode(x32, MAX_LENGTH)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                m32._encode(x32, MAX_LENGTH)
            e1.record()
            torch.cuda.synchronize(dev)
            enc32_ms = e0.elapsed_time(e1) / 5
            rr32 = decode_roofline_record(m32, x32, B, S, 4, "fp32", enc32_ms)
            out["parity_mode"]["roofline"] = rr32["roofline"]
            out["parity_mode"]["encoder_plus_crosskv_ms"] = enc32_ms
            out["parity_mode"]["encoder_fp32_mfma_frac_of_157TF"] = B * 35.17e9 / (enc32_ms * 1e-3) / 157e12
            del x32
        if not args.no_native:      # the reference's precision at the reference's geometry: the number a user of evaluate.py sees
            nat32 = reference_native_record(m32, cfg, geom, dev, reps=2, esize=4)
            out["parity_mode"]["reference_native"] = {k: nat32[k] for k in ("workload", "tokens_per_s", "ms_per_batch", "step_mean_us", "step_frac")}
        out["config"]["precision_note"] = (
            f"throughput mode: bf16 GEMM inputs and K/V caches; its ids follow a bf16-emulating oracle and equal the fp32 CPU reference's on "
            f"{100 * float(same.float().mean()):.0f} % of the tokens of this run (parity_mode.bf16_vs_fp32_id_agreement; {int(sum(1 for d in first_div if d < 0))} of {B} "
            f"rows identical to the end); the mode with bit-exact greedy ids is fp32: parity_mode.tokens_per_s = {B * (ids_fp32.shape[1] - 1) / dt32:.0f}")
        out["parity_mode"].update(golden_divergence(ids_bf16, ids_fp32))
        if B >= 2 and (ROOT / "tests" / "golden" / "t5_forced.npz").exists():
            try:
                out["parity_mode"].update(forced_parity_record(cfg, geom, dev, model, m32, model.encoder_inputs(inputs)[:2].contiguous()))
            except AssertionError as e:          # a parity violation must show in the line, not cost the line
                out["parity_mode"]["forced_parity_violation"] = str(e)[:600]
        del m32

    # ---- BASELINE configs[4] (per-GPU share: 128 clips / 8 GPUs): one training step, timed on this GPU ----
    if full and not args.no_train:
        mt = T5Transformer(cfg.to_dict(), precision="fp32")
        load_t5_state(mt, state, strict=False)
        mt = mt.to(dev)
        # the step as the reference runs it: train() mode (ref: train.py:33), T5Config.dropout_rate 0.1 — the main record; without dropout beside it
        out["train_configs4"] = train_step_record(mt, cfg, geom, dev, 16, "bf16", 10, 2, dropout=0.1, profile_launches=True)
        fp8 = train_step_record(mt, cfg, geom, dev, 16, "fp8", 10, 2, dropout=0.1)          # configs[4] names fp8 GEMMs: MXFP8 projections, same step
        out["train_configs4"]["fp8_mx_roofline"] = fp8["roofline"]
        nodrop = train_step_record(mt, cfg, geom, dev, 16, "bf16", 10, 2)
        out["train_configs4"]["dropout_off_ms_per_step"] = nodrop["ms_per_step"]
        out["train_configs4"]["dropout_off_clips_per_s"] = nodrop["clips_per_s"]
        out["train_configs4"]["fp8_mx_ms_per_step"] = fp8["ms_per_step"]
        out["train_configs4"]["fp8_mx_clips_per_s"] = fp8["clips_per_s"]
        out["train_configs4"]["fp8_note"] = ("projection products (forward and dX; the weight gradients take the grouped bf16 launch) on block-scaled OCP FP8 (e4m3, 32 elements per E8M0 scale, "
                                             "v_mfma_scale_f32_32x32x64_f8f6f4); activations quantised inside the product's operand staging; at 16 clips/GPU the products are latency- and "
                                             "VALU-bound, not MFMA-bound, so the faster matrix instruction does not show")
        if args.cpu_tokens > 0:
            out["train_configs4"]["cpu_baseline"] = cpu_train_baseline(cfg, state, 16)
        del mt
        out["train_configs4"]["class_surface"] = train_surface_record(cfg, state, dev, 16, 20, 3)

    if full and args.cpu_tokens > 0:
        out["cpu_baseline"] = cpu_baseline(cfg, state, args.cpu_tokens)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
