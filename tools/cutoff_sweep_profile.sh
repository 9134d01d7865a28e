#!/bin/bash
# What a sweeping filter costs: tools/cutoff_sweep_timing.py on two builds of liba2amd.so.
#   usage: tools/cutoff_sweep_profile.sh PARENT_LIB [OUT_DIR]
# PARENT_LIB: liba2amd.so built from the commit before the sweep pass.  Writes OUT_DIR/cutoff_sweep.jsonl: for 1 and for
# 16 384 sweeping filters three interleaved pairs "parent, every fragment walked by calls" / "this tree through
# a2amd_fragment_repeat" (recording time and kernel time per batch of 64 fragments), one run of this tree walked by calls
# (same sums as the repeat path: the two ways render the same audio), and - a run of its own under
# rocprofv3 --kernel-trace --stats - OUT_DIR/cutoff_sweep_kernel_stats.csv with the pass's own time.
# Every GPU step under a time limit; the first failure ends the script.
set -o pipefail
P=${1:?parent liba2amd.so}
OUT=${2:-profiles/out}
HERE=$(cd "$(dirname "$0")/.." && pwd)
B=$HERE/audiality2_amd/liba2amd.so
T=$HERE/tools/cutoff_sweep_timing.py
mkdir -p "$OUT" || exit 1
: > "$OUT/cutoff_sweep.jsonl"
for n in 1 16384; do
	for k in 1 2 3; do
		timeout -k 10 150 python "$T" "$P" calls $n 2 1 | tee -a "$OUT/cutoff_sweep.jsonl" || exit 1
		timeout -k 10 150 python "$T" "$B" repeat $n 3 1 | tee -a "$OUT/cutoff_sweep.jsonl" || exit 1
	done
	timeout -k 10 150 python "$T" "$B" calls $n 2 1 | tee -a "$OUT/cutoff_sweep.jsonl" || exit 1
done
timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof" -o sweep -- python "$T" "$B" repeat 16384 3 1 > "$OUT/prof_run.txt" 2>&1 || exit 1
f=$(find "$OUT/prof" -name '*kernel_stats.csv' | head -1)
[ -n "$f" ] || { echo "no kernel_stats.csv under $OUT/prof" >&2; exit 1; }
cp "$f" "$OUT/cutoff_sweep_kernel_stats.csv" && head -14 "$OUT/cutoff_sweep_kernel_stats.csv"
