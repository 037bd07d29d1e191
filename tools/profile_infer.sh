set -eu; cd /tmp && export TMPDIR=/tmp && cd "${GRAFT_REPO_ROOT:?}"
O=${OUT:-build/profile}; mkdir -p $O; export O     # where the traces and tables go
rm -rf $O/inf && rocprofv3 --kernel-trace --output-format csv -d $O/inf -o t -- python bench.py --full --no-cpu-baseline --steps 2 --warmup 1 --ramp 0 --train-steps 1 --acq-steps 8 > /dev/null 2>&1
python profiles/steady.py $O/inf/t_kernel_trace.csv k_single_pass 5 $O/infer_steady.md "bench.py acquisition_with_model leg" | head -40
