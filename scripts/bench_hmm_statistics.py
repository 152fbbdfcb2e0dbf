#!/usr/bin/env python3
"""The Baum-Welch E-step of a hidden Markov model (`HipHMM.expected_statistics`: four launches a chunk, DESIGN.md section 11
"Expected statistics (Baum-Welch E-step)") next to `HipCircuit.expected_statistics` -- the layer-wise path -- and to
`HipHMM.log_prob` / `state_posteriors` on the SAME plan, batch and build, following scripts/bench_hmm_posteriors.py's protocol.

    python scripts/bench_hmm_statistics.py --T 256 --K 256 --C 256 --B 4096 [--reps 20] [--warmup 5] [--layerwise-reps 20]

HIP events around each timed call after `--warmup` untimed ones, medians reported.  Before anything is timed the result is held to
its invariants (every ``edge[s]`` sums to ``rows``, so does every fold of ``leaf``; ``log_evidence`` equals `log_prob`'s result) and
compared with the layer-wise path's -- the values themselves are what tests/test_hmm_statistics.py checks against fp64.  The four
launches are also timed one by one through their entry points, each after the untimed launches it reads from.  The pair sum is
``2 B K^2 (T - 1)`` operations against the 157.3 TFLOP/s fp32 matrix peak.  ``--layerwise-reps 0`` leaves the layer-wise path out.
Prints one JSON line.
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
from cirkit_amd.circuit import HipCircuit  # noqa: E402
from cirkit_amd.hmm import HipHMM  # noqa: E402
from cirkit_amd.templates import hmm  # noqa: E402

PEAK_FP32_MATRIX = 157.3e12


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
    ap.add_argument("--layerwise-reps", type=int, default=20)
    args = ap.parse_args()
    T, K, C, B = args.T, args.K, args.C, args.B
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    plan = hmm(list(range(T)), "categorical", K, input_layer_kwargs={"num_categories": C})
    tensors = {n: rng.standard_normal(s).astype(np.float32) for n, (s, _) in plan.tensors.items()}
    x = torch.from_numpy(rng.integers(0, C, (B, T))).to(dev)
    chain = HipHMM(plan, tensors, device=dev)
    res = chain.expected_statistics(x)
    launches = chain.last_launches
    ref = chain.log_prob(x)
    rows = float(res.rows)
    err_lp = float(((res.log_evidence - ref).abs() / ref.abs().clamp(min=1)).max())
    err_edge = max(abs(float(e.double().sum()) - rows) for e in res.edge.values()) / rows
    err_leaf = float((res.leaf[chain.input_layer].double().sum((1, 2)) - rows).abs().max()) / rows
    if not (rows == B and err_lp <= 1e-6 and err_edge <= 1e-4 and err_leaf <= 1e-4):
        raise SystemExit(f"expected_statistics: {rows} live rows of {B}, log-evidence off by {err_lp} (relative), edge sums off by "
                         f"{err_edge}, leaf sums by {err_leaf} (relative to the rows)")
    out = {"T": T, "K": K, "C": C, "B": B, "reps": args.reps, "launches": launches, "log_evidence_relative_difference": err_lp,
           "edge_sum_error": err_edge, "leaf_sum_error": err_leaf}

    if args.layerwise_reps:
        hc = HipCircuit(plan, tensors, device=dev)
        other = hc.expected_statistics(x)
        worst = 0.0
        for j, e in res.edge.items():  # (relative to the mean entry of a matrix that sums to the rows)
            worst = max(worst, float((e - other.edge[j]).abs().max()) * e[0].numel() / rows)
        out["largest_difference_to_layerwise_over_mean_entry"] = worst
        if not worst <= 1e-2:
            raise SystemExit(f"expected_statistics: the two paths differ by {worst} of a mean entry")
        t_lw = _time(lambda: hc.expected_statistics(x), args.layerwise_reps, min(args.warmup, args.layerwise_reps))
        out.update(layerwise_ms=round(float(np.median(t_lw)), 4), layerwise_ms_min=round(min(t_lw), 4), layerwise_reps=args.layerwise_reps)
        del hc, other

    # the four launches one by one, as `expected_statistics` issues them for one chunk
    tab = chain.tables()
    stream = torch.cuda.current_stream(dev).cuda_stream
    Kp = chain.K
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
    lp, gamma, pa, pr = new(B), new(B, T, Kp), new(B, T, Kp), new(B, T, Kp)
    edge, leaf = torch.zeros((T - 1) * Kp * Kp + Kp, device=dev), torch.zeros((T, Kp, C), device=dev)
    units = capi.load().ck_hmm_stats_scratch(T, Kp, C, B)
    scratch = new(max(units, 1) * 1024)
    sp, sn = (scratch.data_ptr(), scratch.numel()) if units else (None, 0)
    head = (tab["w"].data_ptr(), tab["fold"].data_ptr(), tab["var"].data_ptr(), T, Kp)
    source = (tab["rows"].data_ptr(), x.data_ptr(), T, C, None, B, lp.data_ptr(), gamma.data_ptr())
    fwd = lambda: capi.call("ck_hmm_forward_keep", *head, *source, stream)  # noqa: E731
    bwd = lambda: capi.call("ck_hmm_backward_stats", *head, *source, pa.data_ptr(), pr.data_ptr(), stream)  # noqa: E731
    pair = lambda: capi.call("ck_hmm_pair_sum", tab["w"].data_ptr(), tab["var"].data_ptr(), T, Kp, T, B, pa.data_ptr(), pr.data_ptr(),  # noqa: E731
                             gamma.data_ptr(), edge.data_ptr(), sp, sn, stream)
    leafs = lambda: capi.call("ck_hmm_leaf_sum", tab["fold"].data_ptr(), tab["var"].data_ptr(), T, Kp, tab["rows"].data_ptr(),  # noqa: E731
                              x.data_ptr(), T, C, None, B, gamma.data_ptr(), leaf.data_ptr(), sp, sn, stream)
    t_lp = _time(lambda: chain.log_prob(x), args.reps, args.warmup)
    t_post = _time(lambda: chain.state_posteriors(x), args.reps, args.warmup)
    t_all = _time(lambda: chain.expected_statistics(x), args.reps, args.warmup)
    t_fwd = _time(fwd, args.reps, args.warmup)
    t_bwd = _time(bwd, args.reps, args.warmup, before=fwd)  # (in place: each run needs the forward's hand-off)
    t_pair = _time(pair, args.reps, args.warmup)
    t_leaf = _time(leafs, args.reps, args.warmup)
    med = lambda t: round(float(np.median(t)), 4)  # noqa: E731
    flops = 2.0 * B * Kp * Kp * (T - 1)
    out.update(log_prob_ms=med(t_lp), log_prob_ms_min=round(min(t_lp), 4), log_prob_ms_max=round(max(t_lp), 4),
               state_posteriors_ms=med(t_post), state_posteriors_ms_min=round(min(t_post), 4), state_posteriors_ms_max=round(max(t_post), 4),
               expected_statistics_ms=med(t_all), expected_statistics_ms_min=round(min(t_all), 4), expected_statistics_ms_max=round(max(t_all), 4),
               forward_keep_ms=med(t_fwd), backward_stats_ms=med(t_bwd), pair_sum_ms=med(t_pair), leaf_sum_ms=med(t_leaf),
               pair_sum_tflops=round(flops / (med(t_pair) * 1e-3) / 1e12, 2) if T > 1 else 0.0,
               pair_sum_share_of_fp32_matrix_peak=round(flops / (med(t_pair) * 1e-3) / PEAK_FP32_MATRIX, 4) if T > 1 else 0.0)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
