#!/bin/bash
# GPU check + bench lines (TAG=r04 bash tools/gpu_final.sh): the -m gpu suite, smoke, the whole
# bench (--full, K = 4,000) and the driver's shape (a plain run at K = 20).  Logs and lines go to
# $OUT_DIR (default: build/gpu_final under the repository).
set -o pipefail
R="$(cd "$(dirname "$0")/.." && pwd)"; cd "$R"
O="${OUT_DIR:-$R/build/gpu_final}"
mkdir -p "$O"; TAG=${TAG:-r04}
timeout -k 10 1000 python -u -m pytest tests -x -v -m gpu --timeout 200 --timeout-method thread > "$O/pytest_gpu_$TAG.log" 2>&1 \
 && echo "pytest ok" \
 && timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$O/smoke_$TAG.log" 2>&1 \
 && echo "smoke ok" \
 && timeout -k 10 600 python bench.py --full > "$O/bench_$TAG.json" 2> "$O/bench_$TAG.err" \
 && echo "bench ok" \
 && timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 5 > "$O/bench_k20_$TAG.json" 2>> "$O/bench_$TAG.err" \
 && echo "bench k20 ok"
rc=$?
tail -3 "$O/pytest_gpu_$TAG.log"
grep -m5 -E "^(E |FAILED)" "$O/pytest_gpu_$TAG.log"
exit $rc
