# kernel trace of the acquisition leg (eval forward [4,3,1024,2048] + scan), steady-state per-step table
set -eu; cd /tmp && export TMPDIR=/tmp && cd "${GRAFT_REPO_ROOT:?}"
O=${OUT:-build/profile}; mkdir -p $O; export O     # where the traces and tables go
rm -rf $O/pf && rocprofv3 --kernel-trace --output-format csv -d $O/pf -o t -- python bench.py --full --no-cpu-baseline --no-pool --no-trainleg --steps 2 --warmup 1 --ramp 0 --acq-steps 8 > $O/pf_bench.json 2>/dev/null
python profiles/steady.py $O/pf/t_kernel_trace.csv k_cosine_fwd 5 $O/pool_forward_steady.md "rocprofv3 --kernel-trace -- python bench.py --full --no-cpu-baseline --no-pool --no-trainleg --steps 2 --warmup 1 --ramp 0 --acq-steps 8" > /dev/null
head -36 $O/pool_forward_steady.md | cut -c1-130
