#!/usr/bin/env python3
"""EM step time (`HipEMTrainer`, DESIGN.md section 11 "EM training") at BASELINE config 2 (QuadTree-2, Categorical-256,
K = 32; 4096 rows) and config 4 (Poon-Domingos, Gaussian, K = 64; 1024 rows), the lower half of the variables missing,
following scripts/bench_expected_statistics.py's protocol.

    python scripts/bench_em.py [--reps 20] [--warmup 5]

HIP events around each timed call after `--warmup` untimed ones; the median is reported.  Per config: the whole `step`, the
E-step (`accumulate`, each timed call after an untimed `update`, as inside a step) and the M-step (`update`, each timed call
after an untimed `accumulate`).  The M-step is set against its byte floor -- one read of the statistics plus one read and one write of the raw
tensors at the copy rate DESIGN.md section 4 measured (6.0 TB/s) -- and, for context, `HipTrainer.step` (Adam) runs on the
same circuit and rows.  A config whose plan the trainer refuses is reported with the refusal.  One JSON line per config.
"""

from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cirkit_amd.em import HipEMTrainer  # noqa: E402
from cirkit_amd.initializers import init_plan_tensors  # noqa: E402
from cirkit_amd.plan import Plan  # noqa: E402
from cirkit_amd.training import HipTrainer  # noqa: E402

CONFIGS = {"cfg2_qt784": ("config 2", 4096), "cfg4_pd784": ("config 4", 1024)}
HBM_BYTES_PER_S = 6.0e12


def _time(fn, reps: int, warmup: int, before=None) -> float:
    for _ in range(warmup):
        if before is not None:
            before()
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in args.configs.split(","):
        label, B = CONFIGS[name]
        plan = Plan.load(os.path.join(ROOT, "tests", "golden", name))
        tensors = init_plan_tensors(plan)
        row = {"config": label, "plan": name, "B": B}
        try:
            # (a pseudocount keeps every step of the timing loop on live rows: with 0 the parameters reach point masses)
            tr = HipEMTrainer(plan, tensors, device=dev, pseudocount=1e-3)
        except NotImplementedError as e:
            row["refused"] = str(e)
            print(json.dumps(row), flush=True)
            continue
        D = plan.num_variables
        lower = list(range(D // 2, D))
        x = tr.circuit.sample(B, seed=2)
        tr.step(x, lower)  # (binds the chunk sizes, builds every table)
        row["missing"] = len(lower)
        row["step_ms"] = round(_time(lambda: tr.step(x, lower), args.reps, args.warmup), 4)
        # the E-step as a step runs it: after an update, so with the tables of the new parameter state to rebuild
        row["e_step_ms"] = round(_time(lambda: tr.accumulate(x, lower), args.reps, args.warmup, before=tr.update), 4)
        tr.update()
        # the M-step as a step runs it: the launch, the zeroing of the sums and, on a padded plan, the copies' refresh
        row["m_step_ms"] = round(_time(tr.update, args.reps, args.warmup, before=lambda: tr.accumulate(x, lower)), 4)
        stats_bytes, raw_bytes = tr.m_step_bytes()
        floor = (stats_bytes + 2.0 * raw_bytes) / HBM_BYTES_PER_S * 1e3
        row.update({"jobs": tr.num_jobs, "statistics_bytes": stats_bytes, "raw_bytes": raw_bytes, "m_step_floor_ms": round(floor, 5),
                    "m_step_over_floor": round(row["m_step_ms"] / floor, 2),
                    "m_step_over_e_step": round(row["m_step_ms"] / row["e_step_ms"], 4)})
        del tr
        torch.cuda.empty_cache()
        ht = HipTrainer(plan, tensors, device=dev)
        row["adam_step_ms"] = round(_time(lambda: ht.step(x), args.reps, args.warmup), 4)
        row["em_step_over_adam_step"] = round(row["step_ms"] / row["adam_step_ms"], 2)
        print(json.dumps(row), flush=True)
        del ht
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
