#!/bin/bash
# What the quiet noise-filter kernel saves and from how many voices on (profiles/noise_filt_quiet.md):
# tools/noise_repeat_timing.py, chain noisefilt-pan, mode repeat_only, on two builds of liba2amd.so.
#   usage: tools/noise_filt_quiet_profile.sh PARENT_LIB [OUT_DIR]
# PARENT_LIB: liba2amd.so built from the commit before k_leaf_noisefiltpan.  Writes OUT_DIR/noise_filt_quiet.jsonl: three
# interleaved pairs parent / this tree at 16 384 voices, batches of 64 repeat fragments; OUT_DIR/noise_filt_threshold.jsonl:
# the same pairs at 16 .. 1024 voices with A2AMD_NZF_MIN=1 (the compiled threshold is the smallest count from which this
# tree is faster by more than the spread, there and at every larger count); and - a run of its own under rocprofv3
# --kernel-trace --stats - OUT_DIR/noise_filt_quiet_kernel_stats.csv with k_leaf_noisefiltpan's own time.  The outputs'
# sum, peak and noise fields must be equal between the two libraries at every size: checked at the end, a mismatch is
# exit status 2.
# Every GPU step under a time limit; the first failure ends the script.
set -o pipefail
P=${1:?parent liba2amd.so}
OUT=${2:-profiles/out}
HERE=$(cd "$(dirname "$0")/.." && pwd)
B=$HERE/audiality2_amd/liba2amd.so
T=$HERE/tools/noise_repeat_timing.py
mkdir -p "$OUT" || exit 1
: > "$OUT/noise_filt_quiet.jsonl"
: > "$OUT/noise_filt_threshold.jsonl"
for k in 1 2 3; do
	timeout -k 10 150 python "$T" "$P" repeat_only 12 4 noisefilt-pan 16384 | tee -a "$OUT/noise_filt_quiet.jsonl" || exit 1
	timeout -k 10 150 python "$T" "$B" repeat_only 12 4 noisefilt-pan 16384 | tee -a "$OUT/noise_filt_quiet.jsonl" || exit 1
done
for n in 16 32 64 128 256 512 1024; do
	for k in 1 2 3; do
		A2AMD_NZF_MIN=1 timeout -k 10 60 python "$T" "$P" repeat_only 12 4 noisefilt-pan $n | tee -a "$OUT/noise_filt_threshold.jsonl" || exit 1
		A2AMD_NZF_MIN=1 timeout -k 10 60 python "$T" "$B" repeat_only 12 4 noisefilt-pan $n | tee -a "$OUT/noise_filt_threshold.jsonl" || exit 1
	done
done
timeout -k 10 200 rocprofv3 --kernel-trace --stats -d "$OUT/prof_filt_quiet" -o quiet -- python "$T" "$B" repeat_only 6 2 noisefilt-pan 16384 > "$OUT/prof_filt_quiet_run.txt" 2>&1 || exit 1
f=$(find "$OUT/prof_filt_quiet" -name '*kernel_stats.csv' | head -1)
[ -n "$f" ] && cp "$f" "$OUT/noise_filt_quiet_kernel_stats.csv" && head -12 "$OUT/noise_filt_quiet_kernel_stats.csv"
python - "$OUT/noise_filt_quiet.jsonl" "$OUT/noise_filt_threshold.jsonl" <<'PY' || exit 2
import json, sys
bad = 0
for path in sys.argv[1:]:
    by_n = {}
    for line in open(path):
        r = json.loads(line)
        by_n.setdefault(r["voices"], set()).add((r["sum"], r["peak"], r["noise"]))
    for n, seen in sorted(by_n.items()):
        if len(seen) != 1:
            print(f"{path}: {n} voices: sum / peak / noise differ between the runs: {sorted(seen)}")
            bad = 1
print("outputs equal between the two libraries" if not bad else "OUTPUTS DIFFER")
sys.exit(bad)
PY
