# The bench records (--full) and the rocprofv3 trace and PMC passes of both map sizes.
# Output under $OUT (default bench_out/ in the repository root).
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 300 python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err || { tail $OUT/bench_default.err; exit 1; }
timeout -k 10 300 python bench.py --full --map 256 --agents 4096 > $OUT/bench256.json 2> $OUT/bench256.err || { tail $OUT/bench256.err; exit 1; }
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_bench -o run --output-format csv -- python3 bench.py --steps 60 --warmup 5 > $OUT/prof_bench.json 2> $OUT/prof_bench.err || exit 1
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_big -o run --output-format csv -- python3 bench.py --map 256 --agents 4096 --steps 30 --warmup 3 > $OUT/prof_big.json 2> $OUT/prof_big.err || exit 1
timeout -s KILL 120 rocprofv3 --pmc FETCH_SIZE -d $OUT/pmc_fetch -o run --output-format csv -- python3 bench.py --steps 20 --warmup 2 > $OUT/pmc_fetch.json 2> $OUT/pmc_fetch.err || exit 1
timeout -s KILL 120 rocprofv3 --pmc WRITE_SIZE -d $OUT/pmc_write -o run --output-format csv -- python3 bench.py --steps 20 --warmup 2 > $OUT/pmc_write.json 2> $OUT/pmc_write.err || exit 1
timeout -s KILL 120 rocprofv3 --pmc FETCH_SIZE -d $OUT/pmc_f_big -o run --output-format csv -- python3 bench.py --map 256 --agents 4096 --steps 20 --warmup 2 > /dev/null 2> $OUT/pmc_f_big.err || exit 1
timeout -s KILL 120 rocprofv3 --pmc WRITE_SIZE -d $OUT/pmc_w_big -o run --output-format csv -- python3 bench.py --map 256 --agents 4096 --steps 20 --warmup 2 > /dev/null 2> $OUT/pmc_w_big.err || exit 1
