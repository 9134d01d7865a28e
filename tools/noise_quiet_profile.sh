#!/bin/bash
# What the quiet noise kernel saves: tools/noise_repeat_timing.py in mode repeat_only on two builds
# of liba2amd.so.
#   usage: tools/noise_quiet_profile.sh PARENT_LIB [OUT_DIR]
# PARENT_LIB: liba2amd.so built from the commit before k_leaf_noisepan.  Writes OUT_DIR/noise_quiet.jsonl: three
# interleaved pairs parent / this tree, 16 384 noise-pan voices, batches of 64 repeat fragments; and - a run of its own
# under rocprofv3 --kernel-trace --stats - OUT_DIR/noise_quiet_kernel_stats.csv with k_leaf_noisepan's own time.
# Every GPU step under a time limit; the first failure ends the script.
set -o pipefail
P=${1:?parent liba2amd.so}
OUT=${2:-profiles/out}
HERE=$(cd "$(dirname "$0")/.." && pwd)
B=$HERE/audiality2_amd/liba2amd.so
T=$HERE/tools/noise_repeat_timing.py
mkdir -p "$OUT" || exit 1
: > "$OUT/noise_quiet.jsonl"
for k in 1 2 3; do
	timeout -k 10 150 python "$T" "$P" repeat_only 12 4 | tee -a "$OUT/noise_quiet.jsonl" || exit 1
	timeout -k 10 150 python "$T" "$B" repeat_only 12 4 | tee -a "$OUT/noise_quiet.jsonl" || exit 1
done
timeout -k 10 200 rocprofv3 --kernel-trace --stats -d "$OUT/prof_quiet" -o quiet -- python "$T" "$B" repeat_only 6 2 > "$OUT/prof_quiet_run.txt" 2>&1 || exit 1
f=$(find "$OUT/prof_quiet" -name '*kernel_stats.csv' | head -1)
[ -n "$f" ] && cp "$f" "$OUT/noise_quiet_kernel_stats.csv" && head -12 "$OUT/noise_quiet_kernel_stats.csv"
