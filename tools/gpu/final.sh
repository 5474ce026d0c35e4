# round-end check: GPU test suite, smoke, and the full bench line with the
# CPU baseline and every secondary line (-> $BENCH_OUT/bench_full.json)
set -o pipefail
mkdir -p gpurun_out
D=${BENCH_OUT:-bench_out}
mkdir -p "$D"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > gpurun_out/tgpu.log 2>&1 || { tail -30 gpurun_out/tgpu.log; exit 1; }
tail -1 gpurun_out/tgpu.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > gpurun_out/smoke.log 2>&1 || { tail -20 gpurun_out/smoke.log; exit 2; }
tail -1 gpurun_out/smoke.log
timeout -k 10 600 python bench.py --full > "$D/bench_full.json" 2> "$D/bench_full.err" || { tail -20 "$D/bench_full.err"; exit 3; }
python -c "import json, sys; d=json.load(open(sys.argv[1])); print(d['value']/1e9, 'G', d['roofline']); print({k: round(v.get('env_steps_per_sec', v.get('rays_per_sec', 0))/1e6, 1) for k, v in d['secondary'].items() if isinstance(v, dict)})" "$D/bench_full.json"
