# NEEDS an experimental build: the LS_PROJECT_* / LS_TRACE_* knobs are only read by a library built with -DLS_EXPERIMENTAL
# (make -C lidarshooter_amd/csrc clean all EXPERIMENTAL=1, or tools/exp_build.sh + LS_LIB_PATH); the shipped library ignores them.
run() { python bench.py --full --workload xt32 --steps 100 --warmup 10 --no-cpu-baseline > /tmp/o.json 2>/dev/null; python3 -c "
import json,os; d=json.load(open('/tmp/o.json')); r=d['roofline']; print('$1', 'frame', round(d['ms_per_step'],4), 'kernel', round(r['kernel_ms'],4), 'tests', r.get('candidate_tests_per_launch'), d['stage_ms']['trace_aux'])"; }
LS_PROJECT_BIG_CELLS=16 run big16
LS_PROJECT_BIG_CELLS=128 run big128
LS_PROJECT_BIG_CELLS=100000 run nobig
