"""GPU: a plain `bench.py` run prints the headline line and nothing beside it; `--full` adds the records beside the headline.

One timed step each, the --full run without its slow records; what is checked is which records a line carries, and that a plain
run spends at most 30 s outside its warm-up and timed steps (start-up, weights, graph capture at the first step, exit)."""
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]

pytestmark = pytest.mark.gpu

HEADLINE = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config"}


def _bench(*extra_args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    t0 = time.monotonic()
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1", *extra_args],
                       env=env, capture_output=True, text=True, timeout=600)
    wall = time.monotonic() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), wall


def test_plain_run_prints_the_headline_line_only(tmp_path):
    rec, wall = _bench("--dump-outputs", str(tmp_path))
    assert set(rec) == HEADLINE, sorted(set(rec) ^ HEADLINE)
    assert rec["unit"] == "tokens/s" and rec["higher_is_better"] is True and rec["dtype"] == "bf16"
    assert rec["value"] > 0 and rec["ms_per_step"] > 0 and rec["steps"] == 1 and rec["warmup"] == 1
    assert rec["config"]["new_tokens_per_clip"] == 1023
    assert (tmp_path / "tokens.npy").exists()
    outside = wall - (rec["steps"] + rec["warmup"]) * rec["ms_per_step"] * 1e-3
    assert outside < 30.0, (wall, rec["ms_per_step"])


def test_full_run_adds_the_records_beside_the_headline():
    rec, _ = _bench("--full", "--no-native", "--no-parity", "--no-train", "--cpu-tokens", "0")
    assert HEADLINE <= set(rec)
    assert {"roofline", "extras", "frontend_configs1"} <= set(rec)
    assert not ({"reference_native", "ragged_eos", "parity_mode", "train_configs4", "cpu_baseline"} & set(rec))
    assert rec["roofline"]["unit"] == "GB/s" and rec["roofline"]["achieved"] > 0
    assert rec["frontend_configs1"]["us_per_launch"] > 0 and "cpu_torch_stft" not in rec["frontend_configs1"]
