#!/usr/bin/env python3
"""The time-parallel forward of a hidden Markov model (`HipHMM.log_prob(segments=P)`: two launches, DESIGN.md section 11
"Time-parallel forward") next to the sequential walk (`segments=None`: one launch) on the SAME model and batch, following
scripts/bench_hmm.py's protocol.

    python scripts/bench_hmm_scan.py --T 784 --K 32 --C 256 [--B 1 8 32 128 512] [--P 14 28 56] [--reps 20] [--warmup 5]

HIP events around each timed call after `--warmup` untimed ones; the median is reported.  Per batch size the scan's result is
compared with the sequential one before anything is timed.  Each of the two launches is also timed through its own entry point
(`ck_hmm_scan_segments`, `ck_hmm_scan_combine`) on scratch of the call's shapes.  `--P` defaults to about sqrt(T) / 2, sqrt(T) and
2 sqrt(T).  Prints one JSON line per (B, P) and, per B, what `auto_segments` picks and how that compares with the faster of the
measured paths.
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


def _median_ms(fn, reps: int, warmup: int) -> float:
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


def _launches(chain: HipHMM, x: torch.Tensor, P: int):
    """The two launches of one unchunked call as callables, on scratch of their own."""
    tab, dev = chain.tables(), chain.device
    B, D, T, K, ns = int(x.shape[0]), chain.plan.num_variables, len(chain.steps), chain.K, chain.num_states
    C = chain.plan.layers[chain.input_layer].config["num_categories"]
    new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)  # noqa: E731
    lg = new(B, P - 2, -(-ns // 32) * 32, K) if P > 2 else None
    first, last, flags, out = new(B, K), new(B, K), new(B, P, dtype=torch.int32), new(B)
    scratch = (first.data_ptr(), None if lg is None else lg.data_ptr(), last.data_ptr(), flags.data_ptr())
    stream = torch.cuda.current_stream(dev).cuda_stream
    keep = (lg, first, last, flags, out)

    def segments(_keep=keep):
        capi.call("ck_hmm_scan_segments", tab["w"].data_ptr(), tab["fold"].data_ptr(), tab["var"].data_ptr(), T, K, ns,
                  tab["rows"].data_ptr(), x.data_ptr(), D, C, None, B, P, *scratch, stream)

    def combine(_keep=keep):
        capi.call("ck_hmm_scan_combine", T, K, ns, B, P, *scratch, out.data_ptr(), stream)

    return segments, combine


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=784)
    ap.add_argument("--K", type=int, default=32)
    ap.add_argument("--C", type=int, default=256)
    ap.add_argument("--B", type=int, nargs="+", default=[1, 8, 32, 128, 512])
    ap.add_argument("--P", type=int, nargs="+", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    T, K, C = args.T, args.K, args.C
    root = T ** 0.5
    Ps = args.P or sorted({max(2, min(T, round(f * root))) for f in (0.5, 1.0, 2.0)})
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    plan = hmm(list(range(T)), "categorical", K, input_layer_kwargs={"num_categories": C})
    tensors = {n: rng.standard_normal(s).astype(np.float32) for n, (s, _) in plan.tensors.items()}
    chain = HipHMM(plan, tensors, device=dev)
    for B in args.B:
        x = torch.from_numpy(rng.integers(0, C, (B, T))).to(dev)
        ref = chain.log_prob(x).clone()
        seq_ms = _median_ms(lambda: chain.log_prob(x), args.reps, args.warmup)
        best = (seq_ms, None)
        for P in Ps:
            got = chain.log_prob(x, segments=P)
            err = float(((got - ref).abs() / ref.abs().clamp(min=1)).max())
            if not err <= 2e-4:
                raise SystemExit(f"B = {B}, P = {P}: the scan and the sequential walk disagree, largest relative difference {err}")
            ms = _median_ms(lambda: chain.log_prob(x, segments=P), args.reps, args.warmup)
            launches = chain.last_launches
            seg_ms = com_ms = None  # (a call in several chunks: its launches are not timed alone)
            if launches == 2:
                segments, combine = _launches(chain, x, P)
                seg_ms = round(_median_ms(segments, args.reps, args.warmup), 4)
                com_ms = round(_median_ms(combine, args.reps, args.warmup), 4)
            row = {"T": T, "K": K, "C": C, "B": B, "P": P, "reps": args.reps, "sequential_ms": round(seq_ms, 4), "scan_ms": round(ms, 4),
                   "scan_launches": launches, "segments_ms": seg_ms, "combine_ms": com_ms, "speedup": round(seq_ms / ms, 2),
                   "max_rel_difference": err}
            print(json.dumps(row), flush=True)
            best = min(best, (ms, P), key=lambda t: t[0])
        pick = chain.auto_segments(B)
        pick_ms = seq_ms if pick is None else _median_ms(lambda: chain.log_prob(x, segments=pick), args.reps, args.warmup)
        print(json.dumps({"T": T, "K": K, "B": B, "auto": pick, "auto_ms": round(pick_ms, 4), "best": best[1], "best_ms": round(best[0], 4),
                          "auto_within_10_percent_of_best": bool(pick_ms <= 1.1 * best[0])}), flush=True)


if __name__ == "__main__":
    main()
