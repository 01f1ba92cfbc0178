#!/bin/bash
# End-of-round validation on the GPU box (run from the repo root: bash tools/final_run.sh OUT_DIR):
# the -m gpu test suite, the full bench line, a rocprofv3 kernel-stats pass, the PMC traffic passes, the 2-rank gloo
# launch path, and one calibration each of the other model families / bit widths.  Everything lands under
# OUT_DIR; the summaries that are kept go to profiles/r06_* (tools/collect_profiles.sh r06 OUT_DIR).
out=${1:?usage: bash tools/final_run.sh OUT_DIR}
cd /tmp && export TMPDIR=/tmp && cd - >/dev/null
mkdir -p "$out"
rm -f gpurun_out/trace_parity.jsonl gpurun_out/fullshape_parity.jsonl gpurun_out/golden_forward_parity.jsonl gpurun_out/wrapper_flow_parity.jsonl gpurun_out/brecq_traj_parity.jsonl
(time timeout 2400 python -m pytest tests -m gpu -q) > $out/pytest_gpu.log 2>&1; echo "pytest rc=$?"; tail -4 $out/pytest_gpu.log
timeout 900 python bench.py --full > $out/bench.json 2> $out/bench.err; head -c 300 $out/bench.json; echo
timeout 400 rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof -o p -- python3 bench.py --steps 2 --warmup 1 --no-cpu-baseline --schedule product --no-rerun-all > $out/prof.log 2>&1
rm -f $out/prof/p_kernel_trace.csv $out/prof/*/p_kernel_trace.csv
# the same three calibrations on the reference's schedule (every search of every round: what `value` is measured on)
timeout 400 rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_all -o p -- python3 bench.py --steps 2 --warmup 1 --no-cpu-baseline --schedule reference --no-rerun-all > $out/prof_all.log 2>&1
rm -f $out/prof_all/p_kernel_trace.csv $out/prof_all/*/p_kernel_trace.csv
timeout 600 bash tools/pmc_bench.sh $out/pmc > $out/pmc.log 2>&1; tail -5 $out/pmc.log
timeout 300 bash tools/pmc_fused.sh $out/pmc_fused > $out/pmc_fused.log 2>&1
PROF_DT=fp8 timeout 600 bash tools/pmc_gemm.sh $out/pmc_slab "qkv fc1" > $out/pmc_slab.log 2>&1
timeout 600 bash tools/pmc_gram.sh $out/pmc_gram > $out/pmc_gram.log 2>&1
ADALOG_DIST_BACKEND=gloo timeout 300 python bench.py --full --gpus 2 --steps 1 --warmup 0 --no-cpu-baseline > $out/bench_gloo2.json 2> $out/bench_gloo2.err; head -c 200 $out/bench_gloo2.json; echo
for m in deit_tiny vit_base swin_small swin_base; do timeout 300 python bench.py --full --model $m --steps 1 --warmup 1 --no-cpu-baseline > $out/bench_$m.json 2> $out/bench_$m.err; head -c 200 $out/bench_$m.json; echo; done
for b in 3 6; do timeout 300 python bench.py --full --bits $b --steps 1 --warmup 1 --no-cpu-baseline > $out/bench_w${b}.json 2> $out/bench_w${b}.err; head -c 200 $out/bench_w${b}.json; echo; done
timeout 900 python bench.py --full --model swin_base --bits 3 --images-per-gpu 128 --steps 1 --warmup 0 --no-cpu-baseline > $out/bench_swin_base_w3_128img.json 2> $out/bench_swin128.err; head -c 200 $out/bench_swin_base_w3_128img.json; echo
# per-model kernel statistics of the two larger BASELINE models (one warm calibration each)
for m in vit_base swin_base; do
  timeout 400 rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_$m -o p -- python3 bench.py --model $m --steps 1 --warmup 1 --no-cpu-baseline --schedule product --no-rerun-all > $out/prof_$m.log 2>&1
  rm -f $out/prof_$m/p_kernel_trace.csv $out/prof_$m/*/p_kernel_trace.csv
done
# BRECQ: kernel statistics of the reconstruct_single_block call alone (300 iterations, graph replay; torch.profiler around the call:
# rocprofv3 around the whole script would mix in the FP model's forward and the block's calibration), then the products one by one
timeout 400 python tools/bench_brecq.py --iters 300 --kernel-stats $out/kernel_stats_brecq_deit_small_block.csv > $out/prof_brecq.log 2>&1; tail -2 $out/prof_brecq.log
timeout 400 python tools/bench_brecq.py --model vit_base --iters 300 --kernel-stats $out/kernel_stats_brecq_vit_base_block.csv > $out/prof_brecq_vit_base.log 2>&1; tail -2 $out/prof_brecq_vit_base.log
timeout 300 python tools/lab/bq_gemm_bench.py --terms 2 --int-act --out $out/bq_gemm_bench.json > $out/bq_gemm_bench.log 2>&1; tail -2 $out/bq_gemm_bench.log
timeout 300 python tools/lab/bq_gemm_bench.py --model vit_base --terms 2 --int-act --out $out/bq_gemm_bench_vit_base.json > $out/bq_gemm_bench_vit_base.log 2>&1; tail -1 $out/bq_gemm_bench_vit_base.log
