#!/bin/bash
# A/B record of the symbolic hierarchy build: scripts/hierarchy_build_report.py on two builds of libsns.so in one session, then
# the diff of what they print (it must be empty; the wall times of the last step are reported, not diffed).
#   scripts/hierarchy_build_compare.sh PARENT/libsns.so BRANCH/libsns.so OUTDIR
# Every GPU step is a fresh process under its own time limit and the steps are chained: a step that fails, faults or hangs ends
# the script there, and nothing more is started on the GPU.
set -o pipefail
A=$1; B=$2; OUT=$3
HERE=$(cd "$(dirname "$0")" && pwd)
R="$HERE/hierarchy_build_report.py"
mkdir -p "$OUT" && : > "$OUT/parent.txt" && : > "$OUT/branch.txt" &&
timeout -k 10 240 python "$R" --lib "$A" serial      >> "$OUT/parent.txt" &&
timeout -k 10 240 python "$R" --lib "$B" serial      >> "$OUT/branch.txt" &&
timeout -k 10 300 python "$R" --lib "$A" team-duct   >> "$OUT/parent.txt" &&
timeout -k 10 300 python "$R" --lib "$B" team-duct   >> "$OUT/branch.txt" &&
timeout -k 10 300 python "$R" --lib "$A" team-cavity >> "$OUT/parent.txt" &&
timeout -k 10 300 python "$R" --lib "$B" team-cavity >> "$OUT/branch.txt" &&
timeout -k 10 300 python "$R" --lib "$A" team-window >> "$OUT/parent.txt" &&
timeout -k 10 300 python "$R" --lib "$B" team-window >> "$OUT/branch.txt" &&
{ diff "$OUT/parent.txt" "$OUT/branch.txt" > "$OUT/diff.txt"; echo "diff exit $? ($(wc -l < "$OUT/diff.txt") lines; $(wc -l < "$OUT/parent.txt") lines compared)" | tee -a "$OUT/diff.txt"; } &&
if [ "${SETUP_TIME:-1}" = 1 ]; then
    timeout -k 10 420 python "$R" --lib "$A" setup-time > "$OUT/setup_parent.txt" &&
    timeout -k 10 420 python "$R" --lib "$B" setup-time > "$OUT/setup_branch.txt" &&
    tail -n 2 "$OUT/setup_parent.txt" "$OUT/setup_branch.txt"
fi
