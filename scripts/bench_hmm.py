#!/usr/bin/env python3
"""The forward algorithm of a hidden Markov model (`HipHMM.log_prob`: one launch, DESIGN.md section 11 "Hidden Markov models")
next to `HipCircuit.forward` on the SAME plan and batch (one launch per position), following scripts/bench_leave_one_out.py's
protocol.

    python scripts/bench_hmm.py --T 256 --K 256 --C 256 --B 4096 [--reps 20] [--warmup 5]

HIP events around each timed call after `--warmup` untimed ones; the median is reported, with the spread (min, max) of the
chain launch.  Both paths re-use the parameters evaluated by the warm-up: `HipHMM` keeps its tables while the store does not
change, `HipCircuit` is built with `cache_params=True`, so neither time holds the softmax of T K x K matrices (the default
`HipCircuit`, which re-evaluates them in every forward, is timed as well).  The two results are compared before anything is timed.  Operations: 2 B K^2 per position but the last (2 B K there), over the chain launch's time
and against the 157.3 TFLOP/s fp32 matrix peak.  Prints one JSON line.
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

from cirkit_amd.circuit import HipCircuit  # noqa: E402
from cirkit_amd.hmm import HipHMM  # noqa: E402
from cirkit_amd.templates import hmm  # noqa: E402

PEAK_F32_MATRIX = 157.3e12


def _time(fn, reps: int, warmup: int) -> list[float]:
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
    return ts


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=256)
    ap.add_argument("--K", type=int, default=256)
    ap.add_argument("--C", type=int, default=256)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    T, K, C, B = args.T, args.K, args.C, args.B
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    plan = hmm(list(range(T)), "categorical", K, input_layer_kwargs={"num_categories": C})
    tensors = {n: rng.standard_normal(s).astype(np.float32) for n, (s, _) in plan.tensors.items()}
    x = torch.from_numpy(rng.integers(0, C, (B, T))).to(dev)
    chain = HipHMM(plan, tensors, device=dev)
    hc = HipCircuit(plan, tensors, device=dev, cache_params=True)
    got, ref = chain.log_prob(x), hc(x)[:, 0, 0]
    err = float(((got - ref).abs() / ref.abs().clamp(min=1)).max())
    if not err <= 2e-4:
        raise SystemExit(f"HipHMM and HipCircuit disagree: largest relative difference {err}")
    n_layers = hc.num_launches(B)
    t_chain = _time(lambda: chain.log_prob(x), args.reps, args.warmup)
    t_layers = _time(lambda: hc(x), args.reps, args.warmup)
    del hc
    torch.cuda.empty_cache()
    hd = HipCircuit(plan, tensors, device=dev)  # the default: the parameter graphs re-evaluated by every forward, as the reference does
    ms_default = float(np.median(_time(lambda: hd(x), args.reps, args.warmup)))
    ms, ms_layers = float(np.median(t_chain)), float(np.median(t_layers))
    flops = 2.0 * B * K * K * (T - 1) + 2.0 * B * K
    print(json.dumps({
        "T": T, "K": K, "C": C, "B": B, "reps": args.reps,
        "hmm_ms": round(ms, 4), "hmm_ms_min": round(min(t_chain), 4), "hmm_ms_max": round(max(t_chain), 4),
        "hmm_launches": chain.last_launches,
        "hipcircuit_ms": round(ms_layers, 4), "hipcircuit_launches": n_layers, "hipcircuit_default_ms": round(ms_default, 4),
        "hipcircuit_default_launches": hd.num_launches(B),
        "speedup": round(ms_layers / ms, 2), "max_rel_difference": err,
        "hmm_tflops": round(flops / (ms * 1e-3) / 1e12, 2), "hmm_share_of_f32_matrix_peak": round(flops / (ms * 1e-3) / PEAK_F32_MATRIX, 4),
        "hipcircuit_tflops": round(flops / (ms_layers * 1e-3) / 1e12, 2),
        "weight_stream_bytes_per_workgroup_step": 4 * K * K, "workgroups": (B + 31) // 32,
    }), flush=True)


if __name__ == "__main__":
    main()
