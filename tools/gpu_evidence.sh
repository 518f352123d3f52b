# A round's GPU evidence in one call: the -m gpu suite, the N = 1 bench line,
# its rocprofv3 kernel trace and the two PMC passes (separate runs, as the
# MI355X guide prescribes), then on the host: python tools/pmc_summary.py rNN "$OUT"
# (writes profiles/rNN_pmc.json + latest_pmc.json, which bench.py's
# roofline.traffic reads when its kernels.hip hash matches).
#   /usr/local/graft/bin/gpurun --timeout 1150 -- 'bash tools/gpu_evidence.sh'
set -o pipefail
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
OUT=${OUT:-profile_out}   # where the JSON lines and profiler passes go
mkdir -p "$OUT"
rm -rf "$OUT/prof" "$OUT/pmc_fetch" "$OUT/pmc_write"
bash tools/gpu_steps.sh \
 "suite:700:python -u -m pytest tests -m gpu -x -q --timeout 600 --timeout-method thread -p no:cacheprovider --durations=15" \
 "smoke:120:python -c 'import __graft_entry__ as g; g.smoke()'" \
 "bench:240:python -u bench.py --full > $OUT/bench.json" \
 "prof:200:rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o run -- python3 bench.py --full --no-cpu-baseline" \
 "pmcf:70:BENCH_NO_SMALL_WINDOWS=1 timeout -s KILL 60 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch -o run -- python3 bench.py --full --steps 5 --no-cpu-baseline" \
 "pmcw:70:BENCH_NO_SMALL_WINDOWS=1 timeout -s KILL 60 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write -o run -- python3 bench.py --full --steps 5 --no-cpu-baseline"
