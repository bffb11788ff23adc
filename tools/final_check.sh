#!/bin/bash
# GPU-box: the full -m gpu suite + smoke() (tools/gpu_check.sh), then one
# bench --full run that keeps its rocprofv3 summaries (--prof-dir).
#   usage: tools/final_check.sh TAG
ROOT="${GRAFT_REPO_ROOT:-$(pwd)}"
TAG="$1"
cd "$ROOT"
OUT="${EK_OUT_DIR:-$ROOT/check_out}"  # where this run's bench files go
mkdir -p "$OUT"
bash tools/gpu_check.sh "$TAG" "" nobench
rc=$?
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 900 python -u bench.py --full --prof-dir "$OUT/${TAG}_prof" > "$OUT/${TAG}_bench.json" 2> "$OUT/${TAG}_bench.err"
brc=$?
tail -c 1500 "$OUT/${TAG}_bench.json"
echo "pytest rc $rc bench rc $brc"
[ $rc -eq 0 ] && exit $brc
exit $rc
