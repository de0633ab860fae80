#!/bin/bash
R=$(cd "$(dirname "$0")/.." && pwd); cd $R; export OUT=${OUT:-$R/build/r4_check1}; mkdir -p $OUT
timeout -k 10 900 python -m pytest tests/test_gpu_rccl.py tests/test_gpu_encoder.py tests/test_gpu_parity.py -x -q -m gpu > $OUT/r4_t2.log 2>&1 || { tail -15 $OUT/r4_t2.log; exit 1; }; tail -15 $OUT/r4_t2.log
timeout -k 10 600 python bench.py --full > $OUT/r4_bench1.json 2> $OUT/r4_bench1.err || { tail -3 $OUT/r4_bench1.err; exit 2; }
python - <<'PY'
import json, os
d = json.load(open(os.path.join(os.environ["OUT"], "r4_bench1.json")))
print(d["value"], d["ms_per_step"], d["dtype"])
print(json.dumps(d["roofline"])[:900])
print(json.dumps(d["cpu_baseline"])[:2500])
print(d["encoder"]["frac"], d.get("value_f32_gemm_mode"))
print(json.dumps(d["knn_1m"]["roofline"])[:600])
PY
