#!/bin/bash
# One round's tracked evidence (run on an MI355X machine from the repo root):  bash tools/profile_round.sh r02 OUTDIR
#   rocprofv3 --kernel-trace --stats of bench.py (VGG; FPN fp32; FPN bf16) -> per-step kernel summaries (tools/profile_summary.py)
#   PMC FETCH_SIZE / WRITE_SIZE passes over the same commands (tools/pmc_traffic.sh)
#   the bench.py --full lines of the same session (live HIP-event roofline + CPU baseline), reading this session's PMC traffic
# Everything lands under OUTDIR/<tag>_* (OUTDIR relative to the repo root, as tools/pmc_traffic.sh takes it); copy what is to be judged into profiles/.
set -e
TAG=${1:-rXX}
R=$(pwd)
D=${2:?usage: bash tools/profile_round.sh TAG OUTDIR}
O="$R/$D"
mkdir -p "$O"
cd /tmp && export TMPDIR=/tmp
prof() {   # name, bench args...
    local name=$1; shift
    timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/${TAG}_prof_$name" -- python3 "$R/bench.py" "$@" --steps 12 --warmup 3 > "$O/${TAG}_prof_$name.log" 2>&1
    python3 "$R/tools/profile_summary.py" $(ls "$O"/${TAG}_prof_$name/*/*_kernel_trace.csv | head -1) --steps 10 > "$O/${TAG}_${name}_kernel_summary.csv"
    cp $(ls "$O"/${TAG}_prof_$name/*/*_kernel_stats.csv | head -1) "$O/${TAG}_${name}_rocprofv3_kernel_stats.csv"
    grep '^{"metric"' "$O/${TAG}_prof_$name.log" | tail -1 > "$O/${TAG}_${name}_bench_under_rocprof.json"
    rm -rf "$O/${TAG}_prof_$name"                  # the raw trace (tens of MB) is not kept
    echo "$name done"
}
prof vgg
prof fpn --config fpn
prof fpn_bf16 --config fpn --amp bf16
cd "$R"
for c in vgg fpn fpn_bf16; do
    bash tools/pmc_traffic.sh "$D/${TAG}_pmc_$c" $c > /dev/null
    cp "$O/${TAG}_pmc_$c/traffic.json" "$O/${TAG}_pmc_traffic_$c.json"; rm -rf "$O/${TAG}_pmc_$c"
done
echo "pmc done"
mkdir -p profiles
for c in vgg fpn fpn_bf16; do cp "$O/${TAG}_pmc_traffic_$c.json" profiles/${TAG}_pmc_traffic_$c.json; done
bench() {  # name, bench args...: the --full line, its stderr and its bench_detail.json
    local name=$1; shift
    timeout -k 10 900 python3 bench.py --full "$@" > "$O/${TAG}_bench_$name.json" 2> "$O/${TAG}_bench_$name.err"
    cp bench_detail.json "$O/${TAG}_bench_detail_$name.json"
}
bench vgg --no-also
bench fpn --config fpn
bench fpn_bf16 --config fpn --amp bf16
bench default                                      # headline + the graph-replay and FPN figures in `also`
echo "bench done"
