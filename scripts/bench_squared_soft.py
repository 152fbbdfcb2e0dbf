#!/usr/bin/env python3
"""Soft and interval evidence of squared circuits (`HipSquaredCircuit.soft_evidence_log_prob`, `interval_log_prob`; DESIGN.md section 11
"Soft and interval evidence of squared circuits") on BASELINE config 5 (`cfg5_sos_c_k32`: 784 pixels, Embedding-256, K = 32,
complex-lse-sum) at 256 rows.

    python scripts/bench_squared_soft.py [--reps 10] [--warmup 3] [--rows 256]

The method of scripts/bench_squared_loo.py: HIP events around each timed call after `--warmup` untimed ones, in one process; the
median is reported.  One JSON line each:

(a) the leaf launch alone (`ck_squared_soft_leaf`, all 784 pixels, the rows of one chunk), soft weights and bounds, against its own
    roofline: 2 K^2 C flop per (pixel, row) at the fp32 MFMA rate and K^2 values written per (pixel, row) at the HBM rate;
(b) the same launch with the plain VALU form forced at K = 32 (`form` 1);
(c) `soft_evidence_log_prob` and `interval_log_prob` with S = the lower half of the image and S = all pixels;
(d) for scale, `log_marginal` with the same set integrated out, in the same run.
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

from cirkit_amd import squared_soft as ss  # noqa: E402
from cirkit_amd.initializers import init_plan_tensors  # noqa: E402
from cirkit_amd.plan import Plan  # noqa: E402
from cirkit_amd.squared import HipSquaredCircuit  # noqa: E402

MFMA_F32_TFLOPS = 157.3  # v_mfma_f32_32x32x2_f32 at 2.4 GHz on 256 CUs: 256 flop per CU and cycle
HBM_TBPS = 8.0  # the MI355X's HBM3E peak


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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=256)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    golden = os.path.join(ROOT, "tests", "golden")
    plan = Plan.load(os.path.join(golden, "cfg5_sos_c_k32"))
    with np.load(os.path.join(golden, "cfg5_sos_c_k32_golden.npz")) as z:  # (the committed weights: signed, trained scale)
        tensors = {k[2:]: z[k] for k in z.files if k.startswith("w_")}
    if not tensors:
        tensors = init_plan_tensors(plan)
    D, B, C, K = plan.num_variables, args.rows, 256, 32
    sq = HipSquaredCircuit(plan, tensors, device=dev)
    rng = np.random.default_rng(4)
    x = torch.from_numpy(rng.integers(0, C, size=(B, D))).to(dev)
    ll = torch.from_numpy(rng.uniform(-4.0, 4.0, size=(B, D, C)).astype(np.float32)).to(dev)
    lo = torch.from_numpy(rng.integers(0, C - 40, size=(B, D))).to(dev)
    hi = lo + 40  # ("pixel within 40 grey levels": 41 of 256 states)
    every, none = np.ones(D, dtype=bool), np.zeros(D, dtype=bool)
    lower = np.zeros(D, dtype=bool)
    lower[D // 2:] = True
    base = {"plan": "cfg5_sos_c_k32", "B": B, "states": C, "K": K}

    # (a), (b): the leaf launch alone, on the tables of one chunk of the S = all call
    mp = ss.soft_plan(sq, none, every)
    rows = min(B, sq._chunk_rows(None, lambda: sq._row_bytes(mp)))
    xw, _ = sq._clean(x[:rows], every)
    tb = sq._tables(mp, rows, sq.c._run(xw), sq._z_binding())
    out_bytes = float(K * K * sq._esize) * D * rows
    leaf = {}
    for what, states, a in (("soft", C, (ll[:rows].contiguous(), None, None)), ("box", 41, (None, lo[:rows].contiguous(), hi[:rows].contiguous()))):
        flop = 2.0 * K * K * states * D * rows  # (a box takes the states inside its bounds only)
        floor_ms = max(flop / (MFMA_F32_TFLOPS * 1e9), out_bytes / (HBM_TBPS * 1e9))
        for form in (0, 1):
            t = _time(lambda: ss.launch_leaves(sq, tb, rows, *a, form), args.reps, args.warmup)
            leaf[(what, form)] = t
            print(json.dumps(dict(base, what=f"leaf launch alone, {what}, {'MFMA' if form == 0 else 'VALU'} form", rows=rows, pixels=D, ms=round(t, 3),
                                  tflops=round(flop / t / 1e9, 2), out_tbps=round(out_bytes / t / 1e9, 3), flop=flop, out_bytes=out_bytes,
                                  roofline_ms=round(floor_ms, 3), of_roofline=round(floor_ms / t, 3))), flush=True)
    print(json.dumps(dict(base, what="VALU form over MFMA form at K = 32", soft=round(leaf[("soft", 1)] / leaf[("soft", 0)], 2),
                          box=round(leaf[("box", 1)] / leaf[("box", 0)], 2))), flush=True)
    del tb
    mp.dev.clear()

    # (c), (d): the calls
    for name, mask in (("lower half", lower), ("all pixels", every)):
        ids = torch.from_numpy(mask)
        lls = ll[:, ids, :].contiguous()
        mps = ss.soft_plan(sq, none, mask)
        calls = (("soft_evidence_log_prob", lambda: sq.soft_evidence_log_prob(lls, x, soft_vars=ids)),
                 ("interval_log_prob", lambda: sq.interval_log_prob(lo, hi, x, box_vars=ids)),
                 ("log_marginal", lambda: sq.log_marginal(x, ids)))
        for what, fn in calls:
            t = _time(fn, args.reps, args.warmup)
            out = fn()
            line = dict(base, what=what, S=name, soft_vars=int(mask.sum()), call_ms=round(t, 3), mixed_launches=sq.last_launches,
                        finite=bool(torch.isfinite(out).all()))
            if what != "log_marginal":
                line.update(soft_launches=sq.last_soft_launches, row_bytes=sq._row_bytes(mps),
                            rows_per_chunk=sq._chunk_rows(None, lambda: sq._row_bytes(mps)))
            print(json.dumps(line), flush=True)
        mps.dev.clear()


if __name__ == "__main__":
    main()
