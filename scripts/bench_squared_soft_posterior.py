#!/usr/bin/env python3
"""Posteriors and sampling under soft evidence of squared circuits (`HipSquaredCircuit.soft_posterior_marginals`, `sample_soft`;
DESIGN.md section 11 "Posteriors and sampling under soft evidence of squared circuits") on BASELINE config 5 (`cfg5_sos_c_k32`:
784 pixels, Embedding-256, K = 32, complex-lse-sum) at 256 rows, the lower half of the image soft and the upper half observed.

    python scripts/bench_squared_soft_posterior.py [--reps 10] [--warmup 3] [--rows 256] [--sample-pixels 56]

HIP events around each timed call after `--warmup` untimed ones, in one process; the median is reported.  One JSON line each:

(a) `soft_posterior_marginals`: the whole call, its launch counts, and the same call split by events between its phases (c's
    forward, the leaf Gram launches, the mixed launches, the down launches, the leaf launch; summed over the chunks of rows), with
    the MFMA leaf form and with the plain one (`form` 1);
(b) `posterior_marginals` over the same set in the same run, split the same way, for scale;
(c) the leaf launch alone on one chunk, both forms, on the down arena the last call left;
(d) `sample_soft` over the last `--sample-pixels` pixels against `sample_conditional` over the same pixels, per drawn pixel.
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
from cirkit_amd import squared_posterior as sp  # noqa: E402
from cirkit_amd import squared_soft_posterior as ssp  # noqa: E402
from cirkit_amd.initializers import init_plan_tensors  # noqa: E402
from cirkit_amd.plan import Plan  # noqa: E402
from cirkit_amd.squared import HipSquaredCircuit  # noqa: E402


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


def _phases(call, reps: int, warmup: int) -> dict:
    """Median over `reps` calls of the time between the events recorded after each phase, summed over the chunks of a call."""
    runs = []
    for i in range(warmup + reps):
        marks = []

        def mark(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append((name, e))

        mark("start")
        call(mark)
        torch.cuda.synchronize()
        if i < warmup:
            continue
        tot: dict = {}
        for (_, e0), (name, e1) in zip(marks, marks[1:]):
            tot[name] = tot.get(name, 0.0) + e0.elapsed_time(e1)
        runs.append(tot)
    return {k + "_ms": round(float(np.median([r[k] for r in runs])), 4) for k in runs[0]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--sample-pixels", type=int, default=56)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    golden = os.path.join(ROOT, "tests", "golden")
    plan = Plan.load(os.path.join(golden, "cfg5_sos_c_k32"))
    with np.load(os.path.join(golden, "cfg5_sos_c_k32_golden.npz")) as z:  # (the committed weights: signed, trained scale)
        tensors = {k[2:]: z[k] for k in z.files if k.startswith("w_")}
    if not tensors:
        tensors = init_plan_tensors(plan)
    D, B, C = plan.num_variables, args.rows, 256
    sq = HipSquaredCircuit(plan, tensors, device=dev)
    rng = np.random.default_rng(4)
    x = torch.from_numpy(rng.integers(0, C, size=(B, D))).to(dev)
    lower = list(range(D // 2, D))
    ll = torch.from_numpy(rng.uniform(-1.0, 1.0, size=(B, len(lower), C)).astype(np.float32)).to(dev)
    base = {"plan": "cfg5_sos_c_k32", "B": B, "soft_vars": len(lower), "states": C}
    tables = {}
    for form in (0, 1):
        call = lambda mark=None: ssp.soft_posterior_marginals(sq, ll, x, soft_vars=lower, form=form)  # noqa: E731
        t = _time(call, args.reps, args.warmup)
        tables[form] = call()
        soft, integrate = np.zeros(D, dtype=bool), np.zeros(D, dtype=bool)
        soft[lower] = True
        dp = ssp.plan_of(sq, soft, integrate)
        line = dict(base, what="soft_posterior_marginals", leaf_form="mfma" if form == 0 else "plain", call_ms=round(t, 3),
                    soft_launches=sq.last_soft_launches, mixed_launches=sq.last_launches, down_launches=sq.last_down_launches,
                    row_bytes=ssp.row_bytes(sq, dp), rows_per_chunk=sq._chunk_rows(None, lambda: ssp.row_bytes(sq, dp)),
                    finite=bool(torch.isfinite(tables[form]).all()))
        line.update(_phases(lambda mark: ssp.soft_query_log_marginals(sq, ll, x, soft_vars=lower, normalized=False, form=form, mark=mark),
                            args.reps, args.warmup))
        print(json.dumps(line), flush=True)
    print(json.dumps(dict(base, what="mfma against plain", max_abs_probability_difference=float((tables[0].exp() - tables[1].exp()).abs().max()))),
          flush=True)
    # (c) the leaf launch alone, on the down arena and the tables of the last chunk of the call above
    step = sq._chunk_rows(None, lambda: ssp.row_bytes(sq, dp))
    Bc = B - (B - 1) // step * step  # rows of the last chunk
    bt = dp.dev[Bc]
    down = sq._down_buf
    out = torch.empty((Bc, len(lower), C), dtype=torch.float32, device=dev)
    llc = ll[B - Bc:].contiguous()
    stream = torch.cuda.current_stream(dev).cuda_stream
    leaf = {}
    for form in (0, 1):
        leaf[form] = _time(lambda: capi.call("ck_squared_soft_down_leaf", down.data_ptr(), down.numel(), bt.vars_host.ctypes.data, bt.vars_dev.data_ptr(),
                                             len(lower), C, llc.data_ptr(), len(lower), C, out.data_ptr(), Bc, sq.rows_per_block, 1, form, stream),
                           args.reps, args.warmup)
    print(json.dumps(dict(base, what="leaf launch alone", rows=Bc, mfma_ms=round(leaf[0], 4), plain_ms=round(leaf[1], 4),
                          plain_over_mfma=round(leaf[1] / leaf[0], 2))), flush=True)
    # (b) posterior_marginals over the same set, for scale
    t = _time(lambda: sq.posterior_marginals(x, lower), args.reps, args.warmup)
    line = dict(base, what="posterior_marginals", call_ms=round(t, 3), mixed_launches=sq.last_mixed_launches, down_launches=sq.last_down_launches)
    line.update(_phases(lambda mark: sp.query_log_marginals(sq, x, lower, normalized=False, mark=mark), args.reps, args.warmup))
    print(json.dumps(line), flush=True)
    # (d) sampling
    n = args.sample_pixels
    if n > 0:
        pix = list(range(D - n, D))
        lls = ll[:, len(lower) - n:].contiguous()
        reps = max(1, args.reps // 3)
        t_soft = _time(lambda: sq.sample_soft(lls, x, soft_vars=pix, seed=1), reps, 1)
        counts = (sq.last_soft_launches, sq.last_launches, sq.last_mixed_launches)
        t_cond = _time(lambda: sq.sample_conditional(x, pix, seed=1), reps, 1)
        print(json.dumps(dict(base, what="sampling", pixels=n, sample_soft_ms=round(t_soft, 2), sample_soft_per_pixel_ms=round(t_soft / n, 4),
                              sample_conditional_ms=round(t_cond, 2), sample_conditional_per_pixel_ms=round(t_cond / n, 4),
                              soft_launches=counts[0], soft_pass_mixed_launches=counts[1], step_mixed_launches=counts[2])), flush=True)


if __name__ == "__main__":
    main()
