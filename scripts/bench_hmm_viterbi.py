#!/usr/bin/env python3
"""Viterbi decoding of a hidden Markov model (`HipHMM.viterbi`: two launches, DESIGN.md section 11 "Viterbi decoding") next to
`HipHMM.log_prob` and `HipHMM.state_posteriors` on the SAME plan, batch and build, following scripts/bench_hmm_posteriors.py's
protocol.

    python scripts/bench_hmm_viterbi.py --T 256 --K 256 --C 256 --B 4096 [--reps 20] [--warmup 5]

HIP events around each timed call after `--warmup` untimed ones, medians reported.  Before anything is timed the result is held to
its invariants (states in range, the score at or below `log_prob`'s log-likelihood) -- the values themselves are what
tests/test_hmm_viterbi.py checks against fp64.  The two launches are also timed one by one through their entry points, and
`ck_hmm_forward` beside them: the max-product pass does 32 K^2 multiply-max pairs a workgroup and step on the vector ALU where
the forward does as many multiply-adds on the matrix pipe.  Prints one JSON line.
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
from bench_hmm_posteriors import _time  # noqa: E402


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
    states, score = chain.viterbi(x)
    launches = chain.last_launches
    lp = chain.log_prob(x)
    if not (int(states.min()) >= 0 and int(states.max()) < chain.num_states and bool((score <= lp + 1e-4 * lp.abs()).all())):
        raise SystemExit("viterbi: a state out of range, or a path more probable than the evidence")

    tab = chain.tables()
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = torch.empty(B, dtype=torch.float32, device=dev)
    keep = torch.empty((B, T, chain.K), dtype=torch.float32, device=dev)
    path = torch.empty((B, T), dtype=torch.int64, device=dev)
    head = (tab["w"].data_ptr(), tab["fold"].data_ptr(), tab["var"].data_ptr(), T, chain.K, tab["rows"].data_ptr(), x.data_ptr(), T, C,
            None, B, out.data_ptr())
    fwd = lambda: capi.call("ck_hmm_forward", *head, stream)  # noqa: E731
    vfwd = lambda: capi.call("ck_hmm_viterbi_forward", *head, keep.data_ptr(), stream)  # noqa: E731
    back = lambda: capi.call("ck_hmm_viterbi_backtrack", tab["w"].data_ptr(), tab["var"].data_ptr(), T, chain.K, chain.num_states, T, B,  # noqa: E731
                             out.data_ptr(), keep.data_ptr(), path.data_ptr(), stream)

    t = {"log_prob": _time(lambda: chain.log_prob(x), args.reps, args.warmup),
         "state_posteriors": _time(lambda: chain.state_posteriors(x), args.reps, args.warmup),
         "viterbi": _time(lambda: chain.viterbi(x), args.reps, args.warmup)}
    vfwd()
    t["viterbi_forward"] = _time(vfwd, args.reps, args.warmup)
    t["viterbi_backtrack"] = _time(back, args.reps, args.warmup)
    t["forward"] = _time(fwd, args.reps, args.warmup)
    ms = {k: float(np.median(v)) for k, v in t.items()}
    products = 32.0 * chain.K * chain.K * (T - 1) * -(-B // 32)
    res = {"T": T, "K": K, "C": C, "B": B, "reps": args.reps, "viterbi_launches": launches}
    for k, v in t.items():
        res.update({f"{k}_ms": round(ms[k], 4), f"{k}_ms_min": round(min(v), 4), f"{k}_ms_max": round(max(v), 4)})
    res.update({"viterbi_forward_over_forward": round(ms["viterbi_forward"] / ms["forward"], 3),
                "viterbi_over_log_prob": round(ms["viterbi"] / ms["log_prob"], 3),
                "multiply_max_pairs": products, "pairs_per_ns": round(products / (ms["viterbi_forward"] * 1e6), 2),
                "kept_bytes": 4.0 * B * T * chain.K})
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
