# round-6 lab: GPU tests touched by the FPCS-tail work, then a same-box A/B of ADALOG_FUSED_TAIL and a kernel-stats profile
# (bash tools/lab/r6_ab_tail.sh OUT_DIR)
out=${1:?usage: bash tools/lab/r6_ab_tail.sh OUT_DIR}
mkdir -p $out
python -m pytest tests/test_gpu_kernels.py tests/test_gpu_traces.py tests/test_gpu_layers.py tests/test_gpu_distributed.py -x -q > $out/pytest.log 2>&1; tail -3 $out/pytest.log
for i in 1 2; do for v in 1 0; do
  ADALOG_FUSED_TAIL=$v python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $out/b_${v}_$i.json 2>/dev/null
  python -c "
import json,sys;d=json.load(open('$out/b_${v}_$i.json'));print('FUSED_TAIL=$v', round(d['ms_per_step'],1), round(d['config']['other_schedule']['ms_per_step'],1))"
done; done
cd /tmp && export TMPDIR=/tmp && cd - >/dev/null && rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof -o ks -- python3 bench.py --steps 3 --warmup 0 --no-cpu-baseline --no-rerun-all > $out/bench_prof.json 2> $out/prof.err; find $out/prof -name "*kernel_stats.csv" -exec cp {} $out/kernel_stats_ref.csv \; ; rm -rf $out/prof
