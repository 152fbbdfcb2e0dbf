#!/usr/bin/env python3
"""Soft (likelihood) evidence on a hidden Markov model (`HipHMM.soft_evidence_log_prob` and its three companions, DESIGN.md section
11 "Soft evidence on chains") with every variable soft, following scripts/bench_hmm_posteriors.py's protocol.

    python scripts/bench_hmm_soft.py --T 256 --K 256 --C 256 --B 4096 [--reps 20] [--warmup 5] [--no-circuit]

HIP events around each timed call after `--warmup` untimed ones, medians reported.  Before anything is timed the results are held
to their invariants (the four queries agree on log Z, state posteriors and soft posteriors sum to 1 per position) -- the values
themselves are what tests/test_hmm_soft.py checks against fp64.  The new launches are also timed one by one through their entry
points (`ck_hmm_soft_rows`, `ck_hmm_soft_flag`, `ck_hmm_soft_leaf` after an untimed forward and backward), `ck_hmm_forward` on the
block beside them, and the two contractions (2 B T Cp K flops each) are reported against the 157.3 TFLOP/s fp32 matrix peak.
Unless `--no-circuit`, `HipCircuit.soft_evidence_log_prob` / `soft_posterior_marginals` of the owned circuit run on the same plan
and batch, results compared first.  Prints one JSON line.
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

sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_hmm_posteriors import _time  # noqa: E402

PEAK_FP32_MATRIX = 157.3e12


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=256)
    ap.add_argument("--K", type=int, default=256)
    ap.add_argument("--C", type=int, default=256)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-circuit", action="store_true")
    args = ap.parse_args()
    T, K, C, B = args.T, args.K, args.C, args.B
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    plan = hmm(list(range(T)), "categorical", K, input_layer_kwargs={"num_categories": C})
    tensors = {n: rng.standard_normal(s).astype(np.float32) for n, (s, _) in plan.tensors.items()}
    gen = torch.Generator(device=dev).manual_seed(0)
    ll = 2.0 * torch.randn((B, T, C), device=dev, generator=gen)
    chain = HipHMM(plan, tensors, device=dev)
    queries = {"soft_evidence_log_prob": lambda: chain.soft_evidence_log_prob(ll),
               "soft_state_posteriors": lambda: chain.soft_state_posteriors(ll, return_log_evidence=True),
               "soft_posterior_marginals": lambda: chain.soft_posterior_marginals(ll, return_log_evidence=True),
               "soft_viterbi": lambda: chain.soft_viterbi(ll)}
    chain.soft_evidence_log_prob(ll[:1])  # (the emission table's launch)
    logz, launches = queries["soft_evidence_log_prob"](), {}
    for name, fn in queries.items():
        res = fn()
        launches[name] = chain.last_launches
        if name in ("soft_state_posteriors", "soft_posterior_marginals"):
            err_z = float(((res[1] - logz).abs() / logz.abs().clamp(min=1)).max())
            err_sum = float((res[0].sum(-1) - 1).abs().max())
            if not (err_z <= 1e-6 and err_sum <= 2e-4):
                raise SystemExit(f"{name}: log Z off by {err_z} (relative), sums off by {err_sum}")
        del res
    out = {"T": T, "K": K, "C": C, "B": B, "reps": args.reps, "launches": launches}
    for name, fn in queries.items():
        ts = _time(fn, args.reps, args.warmup)
        out[name + "_ms"], out[name + "_ms_min"], out[name + "_ms_max"] = round(float(np.median(ts)), 4), round(min(ts), 4), round(max(ts), 4)

    # the launches one by one, a chunk of rows as the calls above take it
    tab = chain.tables()
    stream = torch.cuda.current_stream(dev).cuda_stream
    Kp, Cp, F = chain.K, -(-C // 32) * 32, int(tab["rows"].shape[0])
    n = min(B, max(1, (1 << 30) // (4 * Kp * max(F, T))))
    new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)  # noqa: E731
    block, m, flags, z, gamma, marg = new(F, n, Kp), new(T, n), new(T, n, dtype=torch.int32), new(n), new(n, T, Kp), new(n, T, Cp)
    ident = torch.arange(T, dtype=torch.int32, device=dev)
    steps = (tab["fold"].data_ptr(), tab["var"].data_ptr(), T, Kp)
    head = (tab["w"].data_ptr(), *steps, block.data_ptr(), None, T, 0, None, n, z.data_ptr())
    em = tab["emission"].data_ptr()
    rows = lambda: capi.call("ck_hmm_soft_rows", ll.data_ptr(), T, C, ident.data_ptr(), *steps, tab["rows"].data_ptr(), em, None, 0, C,  # noqa: E731
                             None, n, block.data_ptr(), m.data_ptr(), flags.data_ptr(), stream)
    fwd = lambda: capi.call("ck_hmm_forward", *head, stream)  # noqa: E731
    flag = lambda: capi.call("ck_hmm_soft_flag", flags.data_ptr(), T, n, z.data_ptr(), stream)  # noqa: E731

    def smooth():
        capi.call("ck_hmm_forward_keep", *head, gamma.data_ptr(), stream)
        capi.call("ck_hmm_backward", *head, gamma.data_ptr(), stream)

    leaf = lambda: capi.call("ck_hmm_soft_leaf", ll.data_ptr(), T, C, ident.data_ptr(), *steps, em, C, block.data_ptr(), m.data_ptr(),  # noqa: E731
                             gamma.data_ptr(), T, n, z.data_ptr(), marg.data_ptr(), stream)
    rows()
    ms = {"rows": _time(rows, args.reps, args.warmup), "forward": _time(fwd, args.reps, args.warmup),
          "flag": _time(flag, args.reps, args.warmup)}
    smooth()
    ms["leaf"] = _time(leaf, args.reps, args.warmup)
    flops = 2.0 * n * T * Cp * Kp
    out["rows_per_chunk"] = n
    for name, ts in ms.items():
        out[f"{name}_ms"], out[f"{name}_ms_min"], out[f"{name}_ms_max"] = round(float(np.median(ts)), 4), round(min(ts), 4), round(max(ts), 4)
    for name in ("rows", "leaf"):
        out[f"{name}_share_of_fp32_matrix_peak"] = round(flops / (out[f"{name}_ms"] * 1e-3) / PEAK_FP32_MATRIX, 4)
    del block, gamma, marg

    if not args.no_circuit:
        hc = chain.hc
        ref = hc.soft_evidence_log_prob(ll).reshape(-1)
        out["circuit_log_z_relative_difference"] = float(((ref - logz).abs() / logz.abs().clamp(min=1)).max())
        pm = hc.soft_posterior_marginals(ll)
        out["circuit_posterior_difference"] = float((pm[:, :, :C] - chain.soft_posterior_marginals(ll)).abs().max())
        del pm
        for name, fn in (("circuit_soft_evidence_log_prob", lambda: hc.soft_evidence_log_prob(ll)),
                         ("circuit_soft_posterior_marginals", lambda: hc.soft_posterior_marginals(ll))):
            ts = _time(fn, args.reps, args.warmup)
            out[name + "_ms"] = round(float(np.median(ts)), 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
