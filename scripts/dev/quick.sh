timeout -s KILL 900 python -m pytest tests/test_parity_map_gpu.py tests/test_parity_process_gpu.py -m gpu -x -q 2>&1 | tail -4
out=${BENCH_OUT:-build/bench}   # results directory (build/ is not tracked)
mkdir -p "$out"
timeout -s KILL 600 python bench.py --steps 3 --warmup 1 --full --no-cpu-baseline > "$out/bench_q.json" 2> "$out/bench_q.err"
python - "$out" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1] + '/bench_q.json').read().strip().splitlines()[-1])
print('ms_per_step %.1f value %.0f err %.5f closed %d' % (d['ms_per_step'], d['value'], d['config']['consensus_error_rate'], d['config']['gaps_closed']))
print({k: round(v, 1) for k, v in d['stages_ms'].items()})
print('cells/s %.3g' % d['roofline']['wave_cells_per_s'])
PY
tail -2 "$out/bench_q.err"
