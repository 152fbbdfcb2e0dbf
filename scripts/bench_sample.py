#!/usr/bin/env python3
"""Sampling throughput (`HipCircuit.sample`): the prepare step (partition functions + CDF tables, once
per parameter state) and the walk (one launch per call) at BASELINE config 2 (QuadTree-2, Categorical-256, K = 32) and
config 4 (Poon-Domingos, Gaussian, K = 64), N = 4096 and 65 536.

    python scripts/bench_sample.py [--reps 20] [--warmup 5]

HIP events around each timed call after `--warmup` untimed ones; the median is reported.  Prints one JSON line per
(config, N) with the walk's bytes: the output written (N x D x itemsize) and the CDF row entries the binary searches touch
(N x visited draws x log2(M) x 4 bytes, an upper bound on the L2 traffic: rows are shared between samples of a tile).
"""

from __future__ import annotations

import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cirkit_amd.circuit import HipCircuit  # noqa: E402
from cirkit_amd.initializers import init_plan_tensors  # noqa: E402
from cirkit_amd.plan import Plan  # noqa: E402

CONFIGS = {"cfg2_qt784": "config 2", "cfg4_pd784": "config 4"}


def _time(fn, reps: int, warmup: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
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
    ap.add_argument("--sizes", default="4096,65536")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name, label in CONFIGS.items():
        plan = Plan.load(os.path.join(ROOT, "tests", "golden", name))
        hc = HipCircuit(plan, init_plan_tensors(plan), device=dev)
        hc.sample(16, seed=0)
        s = hc._sampler

        def prepare():
            s._key = None
            s.prepare()

        t_prep = _time(prepare, max(3, args.reps // 4), 2)
        itemsize = 4 if s.float_out else 8
        draws = sum(d["F"] * math.ceil(math.log2(max(d["M"], 2))) for d in s.layers if "cdf" in d)
        for n in (int(v) for v in args.sizes.split(",")):
            t = _time(lambda: hc.sample(n, seed=1), args.reps, args.warmup)
            out_b = n * s.D * itemsize
            cdf_b = n * draws * 4
            print(json.dumps({
                "config": label, "plan": name, "N": n, "prepare_ms": round(t_prep, 4), "walk_ms": round(t, 4),
                "samples_per_s": round(n / (t * 1e-3)), "samples_per_wg": s.S, "total_folds": s.total_folds,
                "output_bytes": out_b, "output_TBps": round(out_b / (t * 1e-3) / 1e12, 3),
                "cdf_search_bytes_upper": cdf_b, "cdf_search_TBps": round(cdf_b / (t * 1e-3) / 1e12, 3),
            }), flush=True)


if __name__ == "__main__":
    main()
