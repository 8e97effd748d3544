# full bench line (bench.py --full), whole GPU suite, smoke; every step stops the script when it fails
#   OUT=<directory for the results> bash tools/gpu/suite_bench.sh
set -eo pipefail
: "${OUT:?set OUT to the directory that collects the results}"
mkdir -p "$OUT"
export OUT="$(cd "$OUT" && pwd)" PYTHONUNBUFFERED=1
cd "$(dirname "$0")/../.."
T0=$(date +%s); timeout -k 10 1500 python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err"; echo "bench.py --full wall time: $(( $(date +%s) - T0 )) s"; tail -3 "$OUT/bench.err"
python - <<'PY'
import json, os
d = json.loads(open(os.path.join(os.environ['OUT'], 'bench.json')).read().strip().splitlines()[-1])
print(round(d['value'], 1), 'frames/s', d['repetitions']['ms_per_step_each'])
print('calibration', d.get('calibration'))
r = d['roofline']; print('roofline', {k: r[k] for k in ('frac', 'frac_issued', 'frac_event_timed', 'avg_launch_ms', 'avg_launch_ms_event_timed', 'event_pair_cost_ms', 'traffic')})
print('hbm', {k: (round(v['avg_us_event_timed'], 1), round(v['frac_of_8tb_s'], 3)) for k, v in r['hbm_kernels'].items()})
print('ab', d.get('ab_norm2_fold'))
print('batched', d.get('batched', {}).get('value'), 'parity', d.get('parity_path', {}).get('value'), 'fast', (d.get('parity_path_fast') or {}).get('value'))
print('cpu', d.get('cpu_baseline'), d.get('cpu_baseline_configs0'))
print('other', [(o['config'][:20], round(o['value'], 1)) for o in d.get('other_configs', [])])
PY
rc=0; timeout -k 10 3000 python -m pytest tests -m gpu -q --tb=short -p no:cacheprovider 2>&1 | tail -15 > "$OUT/pytest.log" || rc=$?; tail -8 "$OUT/pytest.log"; [ $rc -eq 0 ]
timeout -k 10 600 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -4
