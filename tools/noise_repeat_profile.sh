#!/bin/bash
# What a noise voice costs: tools/noise_repeat_timing.py on two builds of liba2amd.so.
#   usage: tools/noise_repeat_profile.sh PARENT_LIB [OUT_DIR]
# PARENT_LIB: liba2amd.so built from the commit before a2amd_fragment_repeat_noise.  Writes OUT_DIR/noise_repeat.jsonl:
#   three interleaved pairs "every fragment walked by calls" parent / this tree (the call path's spread),
#   one run through a2amd_fragment_repeat_noise, and - a run of its own under rocprofv3 --kernel-trace --stats -
#   OUT_DIR/noise_repeat_kernel_stats.csv with k_noise_seeds' own time.
# Every GPU step under a time limit; the first failure ends the script.
set -o pipefail
P=${1:?parent liba2amd.so}
OUT=${2:-profiles/out}
HERE=$(cd "$(dirname "$0")/.." && pwd)
B=$HERE/audiality2_amd/liba2amd.so
T=$HERE/tools/noise_repeat_timing.py
mkdir -p "$OUT" || exit 1
: > "$OUT/noise_repeat.jsonl"
for k in 1 2 3; do
	timeout -k 10 150 python "$T" "$P" calls 4 2 | tee -a "$OUT/noise_repeat.jsonl" || exit 1
	timeout -k 10 150 python "$T" "$B" calls 4 2 | tee -a "$OUT/noise_repeat.jsonl" || exit 1
done
timeout -k 10 150 python "$T" "$B" repeat 12 4 | tee -a "$OUT/noise_repeat.jsonl" || exit 1
timeout -k 10 200 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o seed -- python "$T" "$B" repeat 6 2 > "$OUT/prof_run.txt" 2>&1 || exit 1
f=$(find "$OUT/prof" -name '*kernel_stats.csv' | head -1)
[ -n "$f" ] && cp "$f" "$OUT/noise_repeat_kernel_stats.csv" && head -12 "$OUT/noise_repeat_kernel_stats.csv"
