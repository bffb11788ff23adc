# GPU box: bench.py --gpus 2 on the one GPU (host-staged seam: RCCL refuses two
# ranks on one device): the N>1 code path end to end.
cd $GRAFT_REPO_ROOT
OUT="${EK_OUT_DIR:-check_out}"  # where this run's bench files go
mkdir -p "$OUT"
timeout -k 10 900 python3 -u bench.py --gpus 2 --steps 3 --warmup 1 --full > "$OUT/n2_bench.json" 2> "$OUT/n2_bench.err"
rc=$?
tail -c 1500 "$OUT/n2_bench.json"
tail -5 "$OUT/n2_bench.err"
exit $rc
