#!/bin/bash
# Round-end verification on the GPU box: the whole `-m gpu` suite, smoke(), the bench line with --full.
#   usage (from the repo root):  bash tools/gpu_final.sh TAG      -> $OUT/TAG_{gpu_tests,smoke,bench}.log/json (OUT default build/logs)
set -u
TAG=${1:-final}
OUT=${OUT:-build/logs}
mkdir -p "$OUT"
export PYTHONUNBUFFERED=1
timeout -k 10 1500 python -m pytest tests -q -m gpu -x -p no:cacheprovider > "$OUT/${TAG}_gpu_tests.log" 2>&1
rc=$?
tail -3 "$OUT/${TAG}_gpu_tests.log"
[ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$OUT/${TAG}_smoke.log" 2>&1 || { tail -20 "$OUT/${TAG}_smoke.log"; exit 1; }
tail -1 "$OUT/${TAG}_smoke.log"
timeout -k 10 900 python bench.py --full > "$OUT/${TAG}_bench.json" 2> "$OUT/${TAG}_bench.err" || { tail -20 "$OUT/${TAG}_bench.err"; exit 1; }
python tools/bench_summary.py "$OUT/${TAG}_bench.json" 2>/dev/null | head -60
