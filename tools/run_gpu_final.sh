# final check of HEAD: whole GPU suite, smoke, the full bench line (bench.py --full), then a kernel trace of a short bench run; a failing step ends the script
#   OUT=<directory for the results> bash tools/run_gpu_final.sh
set -eo pipefail
: "${OUT:?set OUT to the directory that collects the results}"
mkdir -p "$OUT"
export OUT="$(cd "$OUT" && pwd)" PYTHONUNBUFFERED=1
cd "$(dirname "$0")/.."
rc=0; timeout -k 10 3000 python -m pytest tests -m gpu -q --tb=short -p no:cacheprovider 2>&1 | tail -12 > "$OUT/final_pytest.log" || rc=$?; tail -6 "$OUT/final_pytest.log"; [ $rc -eq 0 ]
timeout -k 10 600 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -4
timeout -k 10 1200 python bench.py --full > "$OUT/final_bench.json" 2> "$OUT/final_bench.err"
python - <<'PY'
import json, os
d = json.loads(open(os.path.join(os.environ['OUT'], 'final_bench.json')).read().strip().splitlines()[-1])
print(round(d['value'], 1), 'frames/s', round(d['ms_per_step'], 3), 'ms  roofline', round(d['roofline']['frac'], 4), round(d['roofline'].get('frac_issued', 0), 4), 'batched', d.get('batched', {}).get('value'),
      'parity', d.get('parity_path', {}).get('value'), 'fast', (d.get('parity_path_fast') or {}).get('value'), 'cpu', d.get('cpu_baseline', {}).get('value'))
print('other', [(o['config'][:20], round(o['value'], 1)) for o in d.get('other_configs', [])])
PY
# kernel trace of the same bench command (profiles/r03_kernel_stats.csv is summarised from it by tools/summarize_prof.py)
export TMPDIR=/tmp
rm -rf "$OUT/kt"
timeout -k 10 900 rocprofv3 --kernel-trace --stats -d "$OUT/kt" -o kt --output-format csv -- python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-breakdown --no-batched --no-parity-path --no-other-configs > "$OUT/final_prof_bench.json" 2> "$OUT/final_prof.err"
for f in $(find "$OUT/kt" -mindepth 2 -name "kt_*.csv"); do cp "$f" "$OUT/kt/"; done
find "$OUT/kt" -mindepth 1 -type d -exec rm -rf {} + 2>/dev/null || true
ls "$OUT/kt" | head
