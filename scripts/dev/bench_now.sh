out=${BENCH_OUT:-build/bench}   # results directory (build/ is not tracked)
mkdir -p "$out"
timeout -s KILL 900 python bench.py --steps 3 --warmup 1 --full > "$out/bench_now.json" 2> "$out/bench_now.err"
tail -c 3000 "$out/bench_now.json"
tail -3 "$out/bench_now.err"
