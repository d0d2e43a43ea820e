#!/bin/bash
# A/B of environment knobs inside ONE GPU-box call: bash tools/ab_knobs.sh "X=1" "DOTRING_PROVE_PARTS=2" ...
tmp=$(mktemp -d)
for cfg in "$@"; do
  env $cfg python bench.py --full --extras 0 --msm-log2n 0 --cpu-proofs 2 --cpu-workers 0 --steps ${AB_STEPS:-4} > "$tmp/ab.json" 2> "$tmp/ab.err"
  python - "$cfg" "$tmp/ab.json" <<PY
import json,sys
l=json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
k=l["gpu_kernel_ms_per_step"]
print(sys.argv[1], "value=%.0f prove_only=%.0f verify_only=%.0f parity=%s" % (l["value"], l["prove_only_proofs_per_s"], l["verify_only_proofs_per_s"], l["parity_ok"]), {n:k.get(n) for n in ("k_g1_accumulate","k_g1_reduce_chunks","k_g1_reduce_windows","k_g1_sort_sets")})
PY
done
