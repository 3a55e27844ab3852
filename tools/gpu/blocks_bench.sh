#!/bin/bash
# block pipeline through bench.py: single-device line, the sharded per-rank program at one rank (rehearsal), and the same
# under torch.distributed.run with a world of one (RCCL initialised).  --full: each line carries the same job through the
# single-device entry points.  Usage: tools/gpu/blocks_bench.sh [OUT_DIR]  (default bench_out/blocks)
set -e
export TMPDIR=/tmp
OUT=${1:-bench_out/blocks}
mkdir -p "$OUT"
ARGS="--mode blocks --steps 10 --full --no-cpu-baseline --no-extras"
timeout -k 10 300 python bench.py $ARGS > "$OUT/bb_single.json" 2> "$OUT/bb_single.err" || (tail -20 "$OUT/bb_single.err"; exit 1)
timeout -k 10 300 python bench.py $ARGS --force-sharded > "$OUT/bb_sharded1.json" 2> "$OUT/bb_sharded1.err" || (tail -20 "$OUT/bb_sharded1.err"; exit 1)
timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29771 bench.py --gpus 1 $ARGS --force-sharded > "$OUT/bb_rccl1.json" 2> "$OUT/bb_rccl1.err" || (tail -20 "$OUT/bb_rccl1.err"; exit 1)
OUT="$OUT" python - <<'PY'
import json, os
for f in ("bb_single","bb_sharded1","bb_rccl1"):
    d=json.loads(open(os.path.join(os.environ["OUT"], "%s.json"%f)).read().strip().splitlines()[-1])
    print(f, "ms/step %.3f"%d["ms_per_step"], "single_same %.3f"%d.get("single_gpu_same_workload_ms",0), "speedup %.2f"%d.get("speedup_vs_single_gpu_same_workload",0), d.get("labels_identical_to_single_gpu_run"), d["config"]["clusters"])
PY
