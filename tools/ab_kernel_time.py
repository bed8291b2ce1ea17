#!/usr/bin/env python3
"""Kernel time of one workload under two or more builds of the library, alternating in ONE job: the protocol for a device-code
change that must not cost time.

    python tools/ab_kernel_time.py [--runs 5] [--match dec_attn_mc_kernel] [--timeout 300] P=<parent .so> N=<new .so> [X=...] -- <command>

Round r runs the command once per library, in the order given (P N P N ...), each run a process of its own under
`rocprofv3 --kernel-trace --stats` with the library in M2M_LIBRARY and no other tracing; every other variable (M2M_GROUP_ROWS, ...)
comes from the caller's environment.  Per kernel name that contains --match, tools/kernel_stats.py gives the average us per launch of
the run.  Printed: every run as it ends, then per instantiation every build's runs, its median, and the verdict against the FIRST
build: "ok" if the median is no higher than the first build's highest run.  A first build whose own range exceeds 1 % of its median
is marked: that job measured the neighbours.  The first run that fails ends the job (nothing is started behind a failure).
"""
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

TOOLS = Path(__file__).resolve().parent


def main() -> int:
    args = sys.argv[1:]
    cmd = args[args.index("--") + 1:]
    args = args[:args.index("--")]
    runs, match, limit, libs = 5, "dec_attn_mc_kernel", 300, []
    while args:
        x = args.pop(0)
        if x == "--runs": runs = int(args.pop(0))
        elif x == "--match": match = args.pop(0)
        elif x == "--timeout": limit = int(args.pop(0))
        else: libs.append(tuple(x.split("=", 1)))
    for tag, lib in libs:
        assert Path(lib).exists(), lib
    figures = {}        # kernel name -> tag -> [us per launch, one per run]
    tmp = Path(tempfile.mkdtemp(prefix="ab_kernel_time_"))
    try:
        for r in range(runs):
            for tag, lib in libs:
                d = tmp / f"{tag}_{r}"
                env = dict(os.environ, M2M_LIBRARY=str(Path(lib).resolve()))
                p = subprocess.run(["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "-d", str(d), "-o", "run", "--", *cmd],
                                   env=env, capture_output=True, text=True)
                if p.returncode != 0:
                    print(f"run {r} of {tag} ended with status {p.returncode}; nothing more is started\n{p.stdout[-1500:]}\n{p.stderr[-1500:]}", flush=True)
                    return 1
                s = subprocess.run([sys.executable, str(TOOLS / "kernel_stats.py"), str(d), "1000"], capture_output=True, text=True, check=True)
                shutil.rmtree(d)
                line = []
                for m in re.finditer(r"^(.*?)\s+n=\s*(\d+) avg\s+([\d.]+) us", s.stdout, re.M):
                    if match in m.group(1):
                        figures.setdefault(m.group(1), {}).setdefault(tag, []).append(float(m.group(3)))
                        line.append(f"{m.group(3)} (n={m.group(2)})")
                print(f"run {r} {tag}: {'  '.join(line)}", flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    first = libs[0][0]
    for name in sorted(figures):
        print(name)
        ref = figures[name].get(first, [])
        for tag, _ in libs:
            v = figures[name].get(tag, [])
            if not v:
                continue
            med = statistics.median(v)
            note = ""
            if tag == first:
                note = f"range {min(v):.3f}-{max(v):.3f}" + ("  RANGE OVER 1 % OF THE MEDIAN" if max(v) - min(v) > 0.01 * med else "")
            elif ref:
                note = "ok" if med <= max(ref) else f"OVER the highest run of {first} ({max(ref):.3f})"
            print(f"  {tag:6s} {', '.join(f'{x:.3f}' for x in v)}  median {med:.3f}  {note}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
