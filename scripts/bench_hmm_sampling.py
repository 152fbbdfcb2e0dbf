#!/usr/bin/env python3
"""Posterior path sampling of a hidden Markov model (`HipHMM.sample_posterior`, `HipHMM.sample`: two launches a chunk, DESIGN.md
section 11 "Sampling paths") next to `HipCircuit.sample_conditional` on the SAME plan and evidence, and to `HipHMM.log_prob`,
`state_posteriors` and `viterbi` on the same build, following scripts/bench_hmm_posteriors.py's protocol.

    python scripts/bench_hmm_sampling.py --T 256 --K 256 --C 256 --B 4096 [--reps 20] [--warmup 5] [--no-layerwise]

A quarter of the entries are missing.  HIP events around each timed call after `--warmup` untimed ones, medians reported (the
layer-wise path: 5 after 2).  Before anything is timed the results are held to their invariants: states in range, observed entries
copied, completions in range, the same bits from chunks of rows, and the layer-wise path's output of the same shape and range with
the same observed entries.  The walk back is also timed through its own entry point after an untimed forward, beside the keeping
forward and `ck_hmm_forward`.  Prints one JSON line.
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
    ap.add_argument("--no-layerwise", action="store_true")
    args = ap.parse_args()
    T, K, C, B = args.T, args.K, args.C, args.B
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    plan = hmm(list(range(T)), "categorical", K, input_layer_kwargs={"num_categories": C})
    tensors = {n: rng.standard_normal(s).astype(np.float32) for n, (s, _) in plan.tensors.items()}
    xh = rng.integers(0, C, (B, T))
    xh[rng.random((B, T)) < 0.25] = -1
    x = torch.from_numpy(xh).to(dev)
    chain = HipHMM(plan, tensors, device=dev)

    def held(states, completed, S):
        seen = (x >= 0)[:, None, :].expand(B, S, T)
        return (int(states.min()) >= 0 and int(states.max()) < chain.num_states and int(completed.min()) >= 0
                and int(completed.max()) < C and bool((completed[seen] == x[:, None, :].expand(B, S, T)[seen]).all()))

    res = {"T": T, "K": K, "C": C, "B": B, "reps": args.reps, "missing": 0.25}
    states, completed = chain.sample_posterior(x, num_samples=8, seed=1)
    res["first_call_launches"] = chain.last_launches
    again = chain.sample_posterior(x, num_samples=8, seed=1, rows_per_chunk=-(-B // 3))
    res["launches_three_chunks"] = chain.last_launches
    if not (held(states, completed, 8) and torch.equal(again[0], states) and torch.equal(again[1], completed)):
        raise SystemExit("sample_posterior: an invariant does not hold")
    xs, zs = chain.sample(B, seed=1)
    if not (tuple(xs.shape) == (B, T) and int(xs.min()) >= 0 and int(xs.max()) < C and int(zs.max()) < chain.num_states):
        raise SystemExit("sample: out of range")

    t = {"log_prob": _time(lambda: chain.log_prob(x), args.reps, args.warmup),
         "state_posteriors": _time(lambda: chain.state_posteriors(x), args.reps, args.warmup),
         "viterbi": _time(lambda: chain.viterbi(x), args.reps, args.warmup),
         "sample_posterior_S1": _time(lambda: chain.sample_posterior(x, num_samples=1, seed=1), args.reps, args.warmup),
         "sample_posterior_S8": _time(lambda: chain.sample_posterior(x, num_samples=8, seed=1), args.reps, args.warmup),
         "sample_B": _time(lambda: chain.sample(B, seed=1), args.reps, args.warmup)}

    tab = chain.tables()
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = torch.empty(B, dtype=torch.float32, device=dev)
    keep = torch.empty((B, T, chain.K), dtype=torch.float32, device=dev)
    head = (tab["w"].data_ptr(), tab["fold"].data_ptr(), tab["var"].data_ptr(), T, chain.K)
    source = (tab["rows"].data_ptr(), x.data_ptr(), T, C, None, B, out.data_ptr())
    fwd = lambda: capi.call("ck_hmm_forward", *head, *source, stream)  # noqa: E731
    kfwd = lambda: capi.call("ck_hmm_forward_keep", *head, *source, keep.data_ptr(), stream)  # noqa: E731
    kfwd()
    for S in (1, 8):
        zs, cs = (torch.empty((B, S, T), dtype=torch.int64, device=dev) for _ in range(2))
        walk = lambda: capi.call("ck_hmm_sample_paths", *head, chain.num_states, tab["cdf"].data_ptr(), x.data_ptr(), T, C, None, B, S,  # noqa: E731
                                 0, 1, out.data_ptr(), keep.data_ptr(), zs.data_ptr(), cs.data_ptr(), stream)
        t[f"walk_back_S{S}"] = _time(walk, args.reps, args.warmup)
    t["forward_keep"] = _time(kfwd, args.reps, args.warmup)
    t["forward"] = _time(fwd, args.reps, args.warmup)
    cdf = torch.empty_like(tab["cdf"])
    t["emission_cdf"] = _time(lambda: capi.call("ck_hmm_emission_cdf", tab["rows"].data_ptr(), int(cdf.shape[0]), chain.K, C,
                                                cdf.data_ptr(), stream), args.reps, args.warmup)
    res["emission_cdf_bytes"] = cdf.numel() * 4

    if not args.no_layerwise:  # what users had: the layer-wise conditional sampler, B * S rows
        from cirkit_amd.circuit import HipCircuit

        hc = HipCircuit(plan, tensors, device=dev)
        for S in (1, 8):
            xr = x.repeat_interleave(S, dim=0)
            got = hc.sample_conditional(xr, [], seed=1)
            if not (tuple(got.shape) == (B * S, T) and int(got.min()) >= 0 and int(got.max()) < C
                    and bool((got[xr >= 0] == xr[xr >= 0]).all())):
                raise SystemExit("sample_conditional: shape, range or observed entries")
            t[f"layerwise_S{S}"] = _time(lambda: hc.sample_conditional(xr, [], seed=1), 5, 2)

    ms = {k: float(np.median(v)) for k, v in t.items()}
    for k, v in t.items():
        res.update({f"{k}_ms": round(ms[k], 4), f"{k}_ms_min": round(min(v), 4), f"{k}_ms_max": round(max(v), 4)})
    for S in (1, 8):
        res[f"walk_back_S{S}_ns_per_sample_step"] = round(ms[f"walk_back_S{S}"] * 1e6 / (B * S * T), 3)
        if f"layerwise_S{S}" in ms:
            res[f"layerwise_over_sample_posterior_S{S}"] = round(ms[f"layerwise_S{S}"] / ms[f"sample_posterior_S{S}"], 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
