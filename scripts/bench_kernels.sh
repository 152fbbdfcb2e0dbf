#!/bin/bash
# prints the per-kernel table of a short bench run (instrumented pass) -- for A/B experiments on the GPU box
LINE=$(python bench.py --full --no-variants --no-other-configs --no-cpu-baseline --no-live-pmc --rounds 4 --steps 50 "$@" | tail -1)
python - "$LINE" <<'PY'
import json, sys
d = json.loads(sys.argv[1])
print("ms_per_step", round(d["ms_per_step"], 5), {k[:40]: round(1e3 * v["ms_per_step"], 2) for k, v in d["roofline"].get("kernels", {}).items()})
PY
