# rocprofv3 kernel trace of the stage-1 train step and of the inference forward + scan (bench.py's secondary legs);
# steady-state per-step breakdowns (MIOpen's find phase excluded) -> $OUT/*.md (default build/profile)
set -eu; cd /tmp && export TMPDIR=/tmp && cd "${GRAFT_REPO_ROOT:?}"
O=${OUT:-build/profile}; mkdir -p $O; export O     # where the traces and tables go
rm -rf $O/tr && rocprofv3 --kernel-trace --output-format csv -d $O/tr -o t -- python bench.py --full --no-cpu-baseline --steps 2 --warmup 1 --ramp 0 --train-steps 10 --acq-steps 8 > $O/tr_bench.json 2>/dev/null
python profiles/steady.py $O/tr/t_kernel_trace.csv multi_tensor_apply 6 $O/h_train_step_steady.md "rocprofv3 --kernel-trace -- python bench.py --full --no-cpu-baseline --steps 2 --warmup 1 --ramp 0 --train-steps 10 --acq-steps 8 (train_iter leg)" > /dev/null
python profiles/steady.py $O/tr/t_kernel_trace.csv k_single_pass 5 $O/i_acquisition_forward_steady.md "same run, acquisition_with_model leg (eval forward [4,3,1024,2048] + scan)" > /dev/null
head -12 $O/h_train_step_steady.md; head -8 $O/i_acquisition_forward_steady.md
