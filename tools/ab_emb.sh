set -e
# bash tools/ab_emb.sh [outdir]   (default bench_out/ab)
O=${1:-bench_out/ab}
mkdir -p $O
timeout -k 10 300 python -u -m pytest -x -q --timeout 200 --timeout-method thread tests/test_embed_bwd_gpu.py tests/test_parity_gpu.py tests/test_stages_gpu.py tests/test_dp_gpu.py > $O/t.log 2>&1
for r in 1 2; do
  DCNR_LIB=$PWD/tools/lab_bin/libdcnr_old.so timeout -k 10 200 python -u bench.py --full --steps 50 --warmup 10 --no-cpu-baseline --no-serving --no-fp32 > $O/old$r.log 2>&1
  timeout -k 10 200 python -u bench.py --full --steps 50 --warmup 10 --no-cpu-baseline --no-serving --no-fp32 > $O/new$r.log 2>&1
done
