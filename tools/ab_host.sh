#!/bin/bash
# Host-layer A/B: two checkouts of the repository (each built the same way,
# `make -C gym-simpletetris_amd/csrc`), timed alternately on one box with the
# host-bound tools: tools/vec_env_bench.py and tools/single_env_bench.py,
# ROUNDS alternations each, then PAIRS pairs of `bench.py --full` (its
# vec_env / single_env variants).  Raw lines and ranges go to OUT.
#   tools/ab_host.sh PARENT_DIR RESULT_DIR OUT [ROUNDS=4] [PAIRS=1]
set -o pipefail
parent=$1 result=$2 out=$3 rounds=${4:-4} pairs=${5:-1}
here=$(cd "$(dirname "$0")" && pwd)
mkdir -p "$(dirname "$out")"
raw=$out.raw
: > "$raw"
run() {  # run LABEL SECONDS DIR CMD...: one step under its own time limit; the first failure ends the A/B
    local label=$1 secs=$2 dir=$3
    shift 3
    echo "## $label: $*" >> "$raw"
    (cd "$dir" && timeout -k 10 "$secs" "$@") >> "$raw" 2>> "$out.stderr"
    local rc=$?
    if [ $rc -ne 0 ]; then
        echo "## $label FAILED rc=$rc" | tee -a "$raw"
        tail -20 "$out.stderr"
        exit $rc
    fi
}
for i in $(seq 1 "$rounds"); do
    run "parent vec_env_bench #$i" 120 "$parent" python tools/vec_env_bench.py
    run "result vec_env_bench #$i" 120 "$result" python tools/vec_env_bench.py
    run "parent single_env_bench #$i" 120 "$parent" python tools/single_env_bench.py
    run "result single_env_bench #$i" 120 "$result" python tools/single_env_bench.py
done
for i in $(seq 1 "$pairs"); do
    run "parent bench --full #$i" 400 "$parent" python bench.py --gpus 1 --full --no-cpu-baseline
    run "result bench --full #$i" 400 "$result" python bench.py --gpus 1 --full --no-cpu-baseline
done
python "$here/ab_host_summary.py" "$raw" > "$out"
cat "$out"
