#!/bin/bash
# the round's record: bench lines of every workload (gpurun), then the rocprofv3 passes (collect_r03.sh)
cd "$GRAFT_REPO_ROOT" || exit 1
mkdir -p gpurun_out
b() { tag=$1; shift; timeout -k 10 600 python bench.py "$@" > gpurun_out/r03_bench_$tag.json 2> gpurun_out/r03_bench_$tag.err; echo "bench $tag rc=$?"; }
b c2a_f32 --full
b c2a_f32_force_dist --full --force-dist --no-variants --no-cpu-baseline
b c3_csr --full --workload c3
b c4_csr --full --workload c4
b c5_csr --full --workload c5
b c5_1000_csr --full --workload c5 --cities 1000 --replicas 256 --steps 2 --warmup 1
b c5_implicit --full --workload c5 --implicit
b c5_1000_implicit --full --workload c5 --implicit --cities 1000 --replicas 256 --steps 2 --warmup 1
# the headline profile is taken at the geometry the committed headline line ran (its autotuner's pick)
PICK_FROM=gpurun_out/r03_bench_c2a_f32.json timeout -k 10 900 bash profiles/collect_r03.sh headline c3 cached energy > gpurun_out/r03_collect_all.log 2>&1; echo "collect rc=$?"
