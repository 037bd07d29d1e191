set -eu; cd /tmp && export TMPDIR=/tmp && cd "${GRAFT_REPO_ROOT:?}"
O=${OUT:-build/profile}; mkdir -p $O; export O     # where the traces and tables go
python bench.py --full > $O/bench_r1f.json 2> $O/bench_r1f.err; tail -c 600 $O/bench_r1f.err
CMD="python bench.py --full --no-cpu-baseline --no-train"
rocprofv3 --kernel-trace --stats --output-format csv -d $O/f_stats -o f -- $CMD > /dev/null 2>&1
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $O/f_fetch -o f -- $CMD --steps 20 --warmup 2 --ramp 0 > /dev/null 2>&1
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $O/f_write -o f -- $CMD --steps 20 --warmup 2 --ramp 0 > /dev/null 2>&1
find $O/f_stats $O/f_fetch $O/f_write -name "*.csv" | head
