#!/bin/bash
# full GPU check of a commit: every -m gpu test, smoke(), the bench line with all legs (bench.py --full), and the rocprofv3
# kernel summary of the same bench command; results under <out dir> (copy what is to be kept into profiles/)
# usage, on the GPU machine: bash tools/gpu/full_check.sh <tag> <out dir>
tag=${1:-check}
out=$(realpath -m "${2:?usage: full_check.sh <tag> <out dir>}")
root=$(cd "$(dirname "$0")/../.." && pwd)
cd "$root"
mkdir -p "$out"
timeout 1500 python -m pytest tests -q -m gpu 2>&1 | tail -4 | tee "$out/${tag}_gputests.txt"
timeout 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -2
timeout 1200 python bench.py --full --steps 5 --warmup 1 > "$out/${tag}_bench.json" 2> "$out/${tag}_bench.err"
python - "$out/${tag}_bench.json" <<'PY'
import json, sys
d=json.load(open(sys.argv[1]))
print('keyframes/s %.0f  ms/step %.2f  roofline frac %.3f' % (d['value'], d['ms_per_step'], d['roofline']['frac']))
print(d['stage_ms_per_512_keyframes']); print(d['parity_check']['frames_bit_exact'], d['parity_check']['icp_max_pose_diff_vs_f64_sums'])
print({k: d['live_latency'][k] for k in d['live_latency'] if k.endswith('_us')})
print({k: v for k, v in d['real_size'].items() if not isinstance(v, (dict, list, str))})
print({k: v for k, v in d['configs4_hires'].items() if not isinstance(v, (dict, list, str))})
PY
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d "$out/prof_$tag" -- python "$root/bench.py" --full --no-legs --steps 5 --warmup 1 > /dev/null 2>&1
cd "$root"
python tools/rocpd_summary.py $(ls "$out"/prof_$tag/*/*.db | head -1) > "$out/${tag}_bench_kernels.txt" 2>&1
rm -rf "$out/prof_$tag"
head -16 "$out/${tag}_bench_kernels.txt" | cut -c1-150
