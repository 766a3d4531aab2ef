#!/bin/bash
# Store-shape microbenchmark of the world matrices (tools/ubench_world_rows.hip), run on the GPU box:
#   bash tools/ubench_world_rows.sh [OUT_DIR]
# 1. event timing of every kernel, plain and non-temporal stores, 1 M and 16 M slots  -> times.jsonl
# 2. rocprofv3 --kernel-trace --stats                                                      -> stats/
# 3. rocprofv3 --pmc FETCH_SIZE, then --pmc WRITE_SIZE, each a run of its own              -> pmc_FETCH_SIZE/, pmc_WRITE_SIZE/
# then a per-kernel digest of all three (tools/ubench_world_rows_digest.py), which also prints the gates of kernel (h) against (f)
# of kernel (i) against (h), and of the sequences "(j), then T - 1 x (k)" against (i).
#   UBENCH_FUSED_ONLY=1 bash tools/ubench_world_rows.sh [OUT_DIR]   runs (i), (j) and (k) alone
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(realpath -m "${1:-$R/build/ubench_world_rows_out}")
mkdir -p "$OUT" "$R/build"
BIN=$R/build/ubench_world_rows
if [ ! -x "$BIN" ] || [ "$R/tools/ubench_world_rows.hip" -nt "$BIN" ]; then
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o "$BIN" "$R/tools/ubench_world_rows.hip" || exit 1
fi
cd /tmp && export TMPDIR=/tmp
timeout -k 10 120 "$BIN" > "$OUT/times.jsonl" || { echo "timing run failed: $?"; exit 1; }
cat "$OUT/times.jsonl"
UBENCH_REPS=50 timeout -k 10 180 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/stats" -o run -- "$BIN" > "$OUT/stats.log" 2>&1 \
    || { echo "kernel-trace run failed: $?"; tail -5 "$OUT/stats.log"; exit 1; }
for c in FETCH_SIZE WRITE_SIZE; do
    UBENCH_REPS=10 timeout -k 10 300 rocprofv3 --pmc $c --output-format csv -d "$OUT/pmc_$c" -o run -- "$BIN" > "$OUT/pmc_$c.log" 2>&1 \
        || { echo "pmc $c run failed: $?"; tail -5 "$OUT/pmc_$c.log"; exit 1; }
done
python3 "$R/tools/ubench_world_rows_digest.py" "$OUT"
