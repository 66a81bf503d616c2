#!/bin/bash
# tools/point_order_timing.py for the bench's three point orders, each GPU step under its own time limit and chained with &&: nothing more
# starts after a step that failed or ran out of time.
#   bash tools/point_order_timing.sh OUT_DIR [PARENT_LIB]      PARENT_LIB: a libmot_hip.so built from the parent commit (optional)
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${1:?usage: point_order_timing.sh OUT_DIR [PARENT_LIB]}
PARENT=${2:+--parent-lib $2}
mkdir -p "$OUT"
timeout -k 10 280 python tools/point_order_timing.py --order random $PARENT 2>&1 | tee "$OUT/random.txt" | tail -8 &&
timeout -k 10 280 python tools/point_order_timing.py --order firing $PARENT 2>&1 | tee "$OUT/firing.txt" | tail -8 &&
timeout -k 10 280 python tools/point_order_timing.py --order beam $PARENT 2>&1 | tee "$OUT/beam.txt" | tail -8
