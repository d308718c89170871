#!/bin/bash
# Round-end evidence: the full bench line, rocprofv3 kernel stats of the same command,
# the sequential (--no-overlap) variant, and HBM traffic (FETCH_SIZE / WRITE_SIZE passes).
# usage: gpu_round_profiles.sh <root>, the directory gpu_traffic.sh writes to and collect_profiles.py reads
set -o pipefail
root=${1:?usage: gpu_round_profiles.sh <output root>}
export TMPDIR=/tmp
rm -rf "$root/round"  # start clean: stale outputs of an earlier run must not be collected
mkdir -p "$root/round"
python3 bench.py --full > "$root/round/bench_default.log" 2>&1 || exit 1
tail -1 "$root/round/bench_default.log" > "$root/round/bench_line.json"
python3 bench.py --full --no-overlap --no-cpu-baseline --no-secondary > "$root/round/bench_seq.log" 2>&1 || exit 1
tail -1 "$root/round/bench_seq.log" > "$root/round/bench_line_no_overlap.json"
rocprofv3 --kernel-trace --stats --output-format csv -d "$root/round/stats" -- python3 bench.py --no-cpu-baseline --no-secondary > "$root/round/stats.log" 2>&1 || exit 1
rocprofv3 --kernel-trace --stats --output-format csv -d "$root/round/stats_seq" -- python3 bench.py --no-cpu-baseline --no-secondary --no-overlap > "$root/round/stats_seq.log" 2>&1 || exit 1
bash scripts/gpu_traffic.sh round/traffic > "$root/round/traffic.txt" 2>&1 || exit 1
cat "$root/round/traffic.txt" | tail -16
cut -c1-300 "$root/round/bench_line.json"
