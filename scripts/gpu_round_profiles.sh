# Round profiles: the bench line and the rocprofv3 kernel-trace summary of the SAME
# `bench.py --full --steps K` invocation (the program after `--`; --full so that every
# mode's kernels are in the trace), then PMC HBM traffic passes
# (FETCH_SIZE / WRITE_SIZE in separate runs) for the listed targets.
# Output goes to $PROFILE_OUT/rp (default: profile_out/rp, which git ignores).
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
RP=${PROFILE_OUT:-profile_out}/rp
mkdir -p $RP
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $RP -o bench -- python3 bench.py --full --steps ${STEPS:-20} --warmup 3 > $RP/bench_line.log 2> $RP/bench_err.log
rc=$?; echo "[$rc] profiled bench"; if [ $rc -ne 0 ]; then tail -5 $RP/bench_err.log; exit $rc; fi
tail -1 $RP/bench_line.log | cut -c1-300
PMC_KERNELS="${PMC_KERNELS:-tsp_fused_teacher cvrp_stepwise}" bash scripts/gpu_pmc.sh
