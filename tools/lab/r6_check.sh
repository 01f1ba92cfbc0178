# final tree: whole GPU suite + the full bench line (bash tools/lab/r6_check.sh OUT_DIR)
out=${1:?usage: bash tools/lab/r6_check.sh OUT_DIR}
mkdir -p $out
(time timeout 2400 python -m pytest tests -m gpu -q) > $out/pytest_gpu.log 2>&1; tail -4 $out/pytest_gpu.log
timeout 900 python bench.py --full > $out/bench.json 2> $out/bench.err; head -c 300 $out/bench.json; echo
