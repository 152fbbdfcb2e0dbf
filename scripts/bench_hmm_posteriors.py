#!/usr/bin/env python3
"""Forward-backward smoothing of a hidden Markov model (`HipHMM.state_posteriors`: two launches, DESIGN.md section 11 "Smoothing
posteriors") next to `HipHMM.log_prob` on the SAME plan, batch and build, following scripts/bench_hmm.py's protocol.

    python scripts/bench_hmm_posteriors.py --T 256 --K 256 --C 256 --B 4096 [--reps 20] [--warmup 5]

HIP events around each timed call after `--warmup` untimed ones, medians reported.  Before anything is timed the result is held
to its invariants (rows sum to 1, the log-likelihood of the pass equals `log_prob`'s) -- the values themselves are what
tests/test_hmm_posteriors.py checks against fp64.  The two passes
are also timed one by one through their entry points (`ck_hmm_forward_keep`; `ck_hmm_backward` after an untimed forward, since it
works in place).  The result buffer moves 3 x 4 B T K bytes -- written by the forward, read and written by the backward pass --
reported against the 8 TB/s HBM peak over the time of both passes.  Prints one JSON line.
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

from cirkit_amd import _capi as capi  # noqa: E402
from cirkit_amd.hmm import HipHMM  # noqa: E402
from cirkit_amd.templates import hmm  # noqa: E402

PEAK_HBM = 8.0e12


def _time(fn, reps: int, warmup: int, before=None) -> list[float]:
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
    post, lp = chain.state_posteriors(x, return_log_prob=True)
    launches = chain.last_launches
    ref = chain.log_prob(x)
    err_lp = float(((lp - ref).abs() / ref.abs().clamp(min=1)).max())
    err_sum = float((post.sum(-1) - 1).abs().max())
    if not (err_lp <= 1e-6 and err_sum <= 1e-4):
        raise SystemExit(f"state_posteriors: log-likelihood off by {err_lp} (relative), row sums off by {err_sum}")

    tab = chain.tables()
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = torch.empty(B, dtype=torch.float32, device=dev)
    keep = torch.empty((B, T, chain.K), dtype=torch.float32, device=dev)
    operands = (tab["w"].data_ptr(), tab["fold"].data_ptr(), tab["var"].data_ptr(), T, chain.K, tab["rows"].data_ptr(), x.data_ptr(), T, C,
                None, B, out.data_ptr(), keep.data_ptr(), stream)
    fwd = lambda: capi.call("ck_hmm_forward_keep", *operands)  # noqa: E731
    bwd = lambda: capi.call("ck_hmm_backward", *operands)  # noqa: E731

    t_lp = _time(lambda: chain.log_prob(x), args.reps, args.warmup)
    t_post = _time(lambda: chain.state_posteriors(x), args.reps, args.warmup)
    t_fwd = _time(fwd, args.reps, args.warmup)
    t_bwd = _time(bwd, args.reps, args.warmup, before=fwd)
    ms_lp, ms_post, ms_fwd, ms_bwd = (float(np.median(t)) for t in (t_lp, t_post, t_fwd, t_bwd))
    traffic = 3.0 * 4 * B * T * chain.K
    print(json.dumps({
        "T": T, "K": K, "C": C, "B": B, "reps": args.reps,
        "log_prob_ms": round(ms_lp, 4), "log_prob_ms_min": round(min(t_lp), 4), "log_prob_ms_max": round(max(t_lp), 4),
        "state_posteriors_ms": round(ms_post, 4), "state_posteriors_ms_min": round(min(t_post), 4),
        "state_posteriors_ms_max": round(max(t_post), 4), "state_posteriors_launches": launches,
        "forward_keep_ms": round(ms_fwd, 4), "backward_ms": round(ms_bwd, 4),
        "forward_keep_over_log_prob": round(ms_fwd / ms_lp, 3), "backward_over_log_prob": round(ms_bwd / ms_lp, 3),
        "result_traffic_bytes": traffic, "result_traffic_ms_at_hbm_peak": round(traffic / PEAK_HBM * 1e3, 4),
        "result_traffic_share_of_hbm_peak": round(traffic / ((ms_fwd + ms_bwd) * 1e-3) / PEAK_HBM, 4),
        "log_prob_relative_difference": err_lp, "row_sum_error": err_sum,
    }), flush=True)


if __name__ == "__main__":
    main()
