#!/usr/bin/env python3
"""The chain-rule decomposition of a hidden Markov model (`HipHMM.autoregressive_log_probs` and `autoregressive_conditionals`: one
launch, DESIGN.md section 11 "Autoregressive conditionals of chains") next to `HipHMM.log_prob`, the backward pass of
`state_posteriors` and `HipCircuit.autoregressive_log_probs` of the owned circuit on the SAME plan and build, following
scripts/bench_hmm_posteriors.py's protocol.

    python scripts/bench_hmm_autoregressive.py --T 256 --K 256 --C 256 --B 4096 [--rows 4] [--reps 20] [--warmup 5]

HIP events around each timed call after `--warmup` untimed ones, medians reported.  Before anything is timed the results are held
to their invariants: the log-probabilities of a row sum to `log_prob`, the conditionals of a position sum to 1 and hold the
log-probability of the observed category, and `HipCircuit.autoregressive_log_probs` along the generative order agrees on the
first `--rows` rows -- the values themselves are what tests/test_hmm_autoregressive.py checks against fp64.  The layer-wise path
expands every row into T rows of T layers, so it is timed on `--rows` rows only and reported per row; the chain launches cost a
workgroup of 32 rows what they cost the batch, so their per-row figure is the whole batch's time over B.  `ck_hmm_backward` is
timed through its entry point after an untimed keeping forward, since it works in place.  Prints one JSON line.
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
    ap.add_argument("--rows", type=int, default=4, help="rows of the batch that the layer-wise path is run and timed on")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    T, K, C, B, R = args.T, args.K, args.C, args.B, min(args.rows, args.B)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    plan = hmm(list(range(T)), "categorical", K, input_layer_kwargs={"num_categories": C})
    tensors = {n: rng.standard_normal(s).astype(np.float32) for n, (s, _) in plan.tensors.items()}
    x = torch.from_numpy(rng.integers(0, C, (B, T))).to(dev)
    chain = HipHMM(plan, tensors, device=dev)
    order = chain.generative_order

    lp = chain.autoregressive_log_probs(x)
    p, lp2 = chain.autoregressive_conditionals(x, return_log_probs=True)
    ref = chain.log_prob(x)
    rel = lambda a, b: float(((a - b).abs() / b.abs().clamp(min=1)).max())  # noqa: E731
    own = torch.gather(p, 2, x[:, order, None])[:, :, 0].log()
    layerwise = chain.hc.autoregressive_log_probs(x[:R], order=order)
    checks = {"row_sum_vs_log_prob": rel(lp.sum(1), ref), "conditional_sum_error": float((p.sum(-1) - 1).abs().max()),
              "conditional_vs_log_probs": rel(own, lp), "layerwise_vs_chain": rel(lp[:R], layerwise)}
    if not (torch.equal(lp, lp2) and checks["row_sum_vs_log_prob"] <= 1e-4 and checks["conditional_sum_error"] <= 1e-4
            and checks["conditional_vs_log_probs"] <= 2e-4 and checks["layerwise_vs_chain"] <= 2e-4):
        raise SystemExit(f"autoregressive results fail their invariants: {checks}")
    del p, lp2, own

    tab = chain.tables()
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = torch.empty(B, dtype=torch.float32, device=dev)
    keep = torch.empty((B, T, chain.K), dtype=torch.float32, device=dev)
    operands = (tab["w"].data_ptr(), tab["fold"].data_ptr(), tab["var"].data_ptr(), T, chain.K, tab["rows"].data_ptr(), x.data_ptr(), T, C,
                None, B, out.data_ptr(), keep.data_ptr(), stream)
    fwd = lambda: capi.call("ck_hmm_forward_keep", *operands)  # noqa: E731
    bwd = lambda: capi.call("ck_hmm_backward", *operands)  # noqa: E731

    t = {"log_prob": _time(lambda: chain.log_prob(x), args.reps, args.warmup),
         "backward": _time(bwd, args.reps, args.warmup, before=fwd),
         "autoregressive_log_probs": _time(lambda: chain.autoregressive_log_probs(x), args.reps, args.warmup),
         "autoregressive_conditionals": _time(lambda: chain.autoregressive_conditionals(x), args.reps, args.warmup)}
    del keep
    t["hipcircuit_autoregressive_log_probs"] = _time(lambda: chain.hc.autoregressive_log_probs(x[:R], order=order), args.reps, args.warmup)
    ms = {k: float(np.median(v)) for k, v in t.items()}
    res = {"T": T, "K": K, "C": C, "B": B, "reps": args.reps, "hipcircuit_rows": R}
    for k, v in t.items():
        res[k + "_ms"], res[k + "_ms_min"], res[k + "_ms_max"] = round(ms[k], 4), round(min(v), 4), round(max(v), 4)
    res.update({
        "log_probs_over_backward": round(ms["autoregressive_log_probs"] / ms["backward"], 3),
        "log_probs_over_log_prob": round(ms["autoregressive_log_probs"] / ms["log_prob"], 3),
        "conditionals_over_log_probs": round(ms["autoregressive_conditionals"] / ms["autoregressive_log_probs"], 3),
        "chain_us_per_row": round(1e3 * ms["autoregressive_log_probs"] / B, 4),
        "hipcircuit_us_per_row": round(1e3 * ms["hipcircuit_autoregressive_log_probs"] / R, 4),
        "conditionals_bytes": 4 * B * T * (-(-C // 32) * 32), **checks})
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
