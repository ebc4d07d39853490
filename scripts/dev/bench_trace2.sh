# dev: traced bench (2 steps) -> the per-call lines of the process stage and the stage table
OUT=${1:-r4_t}
out=${BENCH_OUT:-build/bench}   # results directory (build/ is not tracked)
mkdir -p "$out"
DH_TRACE=1 timeout -s KILL 600 python bench.py --steps 2 --warmup 1 --full --no-cpu-baseline > "$out/$OUT.json" 2> "$out/$OUT.err"
grep "dh_align_db\]" "$out/$OUT.err" | tail -12 | cut -c1-420
grep "dh_process\]" "$out/$OUT.err" | tail -20
python - <<PY
import json
d = json.loads(open('$out/$OUT.json').read().strip().splitlines()[-1])
print('ms_per_step %.1f value %.0f err %.5f closed %d' % (d['ms_per_step'], d['value'], d['config']['consensus_error_rate'], d['config']['gaps_closed']))
print({k: round(v, 1) for k, v in d['stages_ms'].items()})
PY
tail -3 "$out/$OUT.err"
