#!/usr/bin/env python3
"""Most-probable-explanation throughput (`HipCircuit.mpe`, DESIGN.md section 11 "Most probable explanation") at BASELINE
config 2 (QuadTree-2, Categorical-256, K = 32) and config 4 (Poon-Domingos, Gaussian, K = 64), B = 4096 and 65 536 rows,
half-image evidence (the upper 392 pixels observed, the lower 392 maximised).

    python scripts/bench_mpe.py [--reps 20] [--warmup 5] [--sizes 4096,65536]

HIP events around each timed call after `--warmup` untimed ones; the median is reported.  Three timings per (config, B):
the whole call, the upward max-product passes alone (every layer's launch, every chunk) and the walks alone (`ck_mpe_walk`
of every chunk, replayed on the arena the last upward pass left).  Prints one JSON line each.
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
from cirkit_amd.initializers import init_plan_tensors  # noqa: E402
from cirkit_amd.plan import Plan  # noqa: E402
from cirkit_amd.sampling import chunk_rows  # noqa: E402

CONFIGS = {"cfg2_qt784": "config 2", "cfg4_pd784": "config 4"}


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="4096,65536")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name, label in CONFIGS.items():
        plan = Plan.load(os.path.join(ROOT, "tests", "golden", name))
        hc = HipCircuit(plan, init_plan_tensors(plan), device=dev)
        D = plan.num_variables
        mask = torch.from_numpy(np.arange(D) >= D // 2).to(dev)
        for B in (int(v) for v in args.sizes.split(",")):
            x = hc.sample(B, seed=2)
            call = lambda: hc.mpe(x, mask)  # noqa: E731
            t_call = _time(call, args.reps, args.warmup)
            s = hc._sampler
            m = s._mpe
            chunks = chunk_rows(B, None, m.bytes_per_row)
            xm = hc._apply_integration_mask(x, mask).to(s.dtype).contiguous()
            out = xm.clone()
            logv = torch.empty(B, dtype=torch.float32, device=dev)
            bad = torch.zeros(B, dtype=torch.int32, device=dev)

            def upward():
                stream = torch.cuda.current_stream(dev).cuda_stream
                for r0, nb in chunks:
                    m._upward(xm[r0 : r0 + nb], nb, None, bad[r0:], stream)

            def walks():
                stream = torch.cuda.current_stream(dev).cuda_stream
                for r0, nb in chunks:
                    arena, val_off, _ = m._arena(nb)
                    capi.call("ck_mpe_walk", s._table.data_ptr(), m._logw_tab.data_ptr(), m._amax_tab.data_ptr(),
                              len(s.layers), s.root_fold, 0, s.total_folds, s.S, arena.data_ptr(), val_off.data_ptr(),
                              bad.data_ptr(), r0, nb, B, D, xm[r0].data_ptr(), out[r0].data_ptr(), 1 if s.float_out else 0,
                              logv.data_ptr(), stream)

            t_up = _time(upward, args.reps, args.warmup)
            t_walk = _time(walks, args.reps, args.warmup)
            print(json.dumps({
                "config": label, "plan": name, "B": B, "observed": D - D // 2, "rows_per_chunk": chunks[0][1],
                "chunks": len(chunks), "call_ms": round(t_call, 4), "upward_ms": round(t_up, 4), "walk_ms": round(t_walk, 4),
                "rows_per_s": round(B / (t_call * 1e-3)), "rows_per_wg": s.S, "total_folds": s.total_folds,
                "arena_bytes_per_row": m.bytes_per_row,
            }), flush=True)
            del xm, out
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
