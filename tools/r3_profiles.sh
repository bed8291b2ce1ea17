#!/bin/bash
# Round-3 profile set, run on the GPU box from the repo root:  bash tools/r3_profiles.sh <tag>   (writes gpurun_out/prof_<tag>/)
#   bench.json                       the full bench line of this build (--full)
#   kernel_stats.csv                 rocprofv3 --kernel-trace --stats of the headline bench command (decode kernels)
#   pmc_traffic_summary.txt          FETCH_SIZE / WRITE_SIZE per decode-kernel launch, separate passes, WITH the clips/launch header
#   pmc_mfma_summary.txt             matrix-core counters of the inference kernels
#   frontend_*                       configs[1]: log-mel kernel stats + traffic
#   train_dropout_kernel_stats.csv   configs[4] share: 23 directly issued 16-clip steps with dropout 0.1 (tools/train_gap.py)
#   train_pmc_l1_l2_summary.txt      per kernel of that step: L2 hit rate, L1 accesses per cycle and CU, matrix-core busy
TAG=${1:-r3}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
D=gpurun_out/prof_$TAG
mkdir -p $D
python3 bench.py --full > $D/bench.json 2> $D/bench.err
echo "bench done"
rocprofv3 --kernel-trace --stats --output-format csv -d $D/ks -o ks -- python3 bench.py --steps 3 --warmup 1 --no-roofline --no-parity --no-frontend --no-train --cpu-tokens 0 > $D/ks.log 2>&1
cp $D/ks/ks_kernel_stats.csv $D/kernel_stats.csv 2>/dev/null
echo "kernel stats done"
export PMC_OUT=$D/pmc_traffic; bash tools/pmc_traffic.sh > $D/pmc_traffic.log 2>&1; cp $PMC_OUT/summary.txt $D/pmc_traffic_summary.txt 2>/dev/null
export PMC_OUT=$D/pmc_mfma; bash tools/pmc_mfma.sh > $D/pmc_mfma.log 2>&1; cp $PMC_OUT/summary.txt $D/pmc_mfma_summary.txt 2>/dev/null
unset PMC_OUT
echo "pmc done"
rocprofv3 --kernel-trace --stats --output-format csv -d $D/fe -o fe -- python3 tools/frontend_bench.py 64 > $D/fe.log 2>&1
cp $D/fe/fe_kernel_stats.csv $D/frontend_kernel_stats.csv 2>/dev/null
for C in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --kernel-trace --pmc $C --output-format csv -d $D/fe_pmc -o $C -- python3 tools/frontend_bench.py 64 > $D/fe_$C.log 2>&1
done
python3 - "$D" <<'PY' > $D/frontend_pmc_traffic_summary.txt
import csv, glob, sys
d = sys.argv[1]
for c in ("FETCH_SIZE", "WRITE_SIZE"):
    f = glob.glob(f"{d}/fe_pmc/{c}_counter_collection.csv")
    if not f: print("missing", c); continue
    n, tot = 0, 0.0
    for r in csv.DictReader(open(f[0])):
        if r["Counter_Name"] == c and "logmel_kernel" in r["Kernel_Name"]:
            n += 1; tot += float(r["Counter_Value"])
    corr = 2.0 if c == "FETCH_SIZE" else 1.0
    print(f"logmel_kernel B=64  {c}/launch {tot / max(n, 1):10.1f} KiB over {n} launches  ({'x2 corrected ' if corr == 2 else ''}{corr * tot / max(n, 1) * 1024 / 1e6:8.2f} MB)")
PY
echo "frontend done"
M2M_GAP_DROPOUT=0.1 M2M_TRAIN_GRAPH=0 rocprofv3 --kernel-trace --stats --output-format csv -d $D/tr -o tr -- python3 tools/train_gap.py > $D/tr.log 2>&1
cp $D/tr/tr_kernel_stats.csv $D/train_dropout_kernel_stats.csv 2>/dev/null
grep WALL $D/tr.log
M2M_GAP_DROPOUT=0.1 bash tools/pmc_train_l2.sh > $D/train_pmc_l1_l2_summary.txt 2> $D/pmc_train.err
rm -rf $D/ks $D/fe $D/tr $D/fe_pmc $D/pmc_traffic/*.csv $D/pmc_mfma/*.csv gpurun_out/pmc_train_l2/*.csv 2>/dev/null
ls -la $D; head -3 $D/pmc_traffic_summary.txt | cut -c1-200; cat $D/frontend_pmc_traffic_summary.txt; head -12 $D/train_pmc_l1_l2_summary.txt | cut -c1-230
