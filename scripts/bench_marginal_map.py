#!/usr/bin/env python3
"""Marginal MAP throughput (`HipCircuit.marginal_map`, DESIGN.md section 11 "Marginal MAP") at BASELINE config 2 (QuadTree-2,
Categorical-256, K = 32) and config 4 (Poon-Domingos, Gaussian, K = 64), B = 4096 rows: the lower 392 pixels are the query,
the upper 392 the evidence, 30 % of it missing (summed out).

    python scripts/bench_marginal_map.py [--reps 20] [--warmup 5] [--sizes 4096]

HIP events around each timed call after `--warmup` untimed ones, in one process; the median is reported.  Per (config, B):
the whole call, the call with `return_log_prob` (one more marginal forward), the mixed sum / max upward passes alone and the
walks alone (`ck_mmap_walk`, replayed on the arena the last upward pass left) -- and beside them `mpe`'s call, upward pass
and walk on the same batch in the same run, where the missing evidence is maximised too.  Prints one JSON line each.
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
from cirkit_amd.marginal_map import _state  # noqa: E402
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
    ap.add_argument("--sizes", default="4096")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name, label in CONFIGS.items():
        plan = Plan.load(os.path.join(ROOT, "tests", "golden", name))
        hc = HipCircuit(plan, init_plan_tensors(plan), device=dev)
        D = plan.num_variables
        q = np.arange(D) >= D // 2
        mask = torch.from_numpy(q)
        for B in (int(v) for v in args.sizes.split(",")):
            x = hc.sample(B, seed=2)
            miss = torch.from_numpy((np.random.default_rng(3).random((B, D)) < 0.3) & ~q).to(dev)
            sentinel = float("nan") if x.dtype == torch.float32 else -1
            x = torch.where(miss, torch.full((), sentinel, dtype=x.dtype, device=dev), x)
            t_call = _time(lambda: hc.marginal_map(x, mask), args.reps, args.warmup)
            t_prob = _time(lambda: hc.marginal_map(x, mask, return_log_prob=True), args.reps, args.warmup)
            t_mpe = _time(lambda: hc.mpe(x, mask), args.reps, args.warmup)
            s = hc._sampler
            st, m = _state(hc), s._mpe
            is_query, max_fold, _ = st.query_tables(q)
            chunks = chunk_rows(B, None, m.bytes_per_row)
            xm = hc._apply_integration_mask(x, mask).to(s.dtype).contiguous()
            out = xm.clone()
            logv = torch.empty(B, dtype=torch.float32, device=dev)
            bad = torch.zeros(B, dtype=torch.int32, device=dev)

            def stream():
                return torch.cuda.current_stream(dev).cuda_stream

            def upward():
                for r0, nb in chunks:
                    st._upward(xm[r0 : r0 + nb], nb, is_query, max_fold, None, bad[r0:], stream())

            def walks():
                for r0, nb in chunks:
                    arena, val_off, _ = m._arena(nb)
                    st._walk(s._table, arena, val_off, is_query, max_fold, bad, r0, nb, B, xm[r0 : r0 + nb], out, logv, stream())

            def mpe_upward():
                for r0, nb in chunks:
                    m._upward(xm[r0 : r0 + nb], nb, None, bad[r0:], stream())

            def mpe_walks():
                for r0, nb in chunks:
                    arena, val_off, _ = m._arena(nb)
                    capi.call("ck_mpe_walk", s._table.data_ptr(), m._logw_tab.data_ptr(), m._amax_tab.data_ptr(),
                              len(s.layers), s.root_fold, 0, s.total_folds, s.S, arena.data_ptr(), val_off.data_ptr(),
                              bad.data_ptr(), r0, nb, B, D, xm[r0].data_ptr(), out[r0].data_ptr(), 1 if s.float_out else 0,
                              logv.data_ptr(), stream())

            t_up, t_walk = _time(upward, args.reps, args.warmup), _time(walks, args.reps, args.warmup)
            t_mup, t_mwalk = _time(mpe_upward, args.reps, args.warmup), _time(mpe_walks, args.reps, args.warmup)
            print(json.dumps({
                "config": label, "plan": name, "B": B, "query": int(q.sum()), "missing": round(float(miss.float().mean()), 3),
                "max_folds": int(max_fold.sum()), "total_folds": s.total_folds, "chunks": len(chunks),
                "call_ms": round(t_call, 4), "call_with_log_prob_ms": round(t_prob, 4), "upward_ms": round(t_up, 4),
                "walk_ms": round(t_walk, 4), "mpe_call_ms": round(t_mpe, 4), "mpe_upward_ms": round(t_mup, 4),
                "mpe_walk_ms": round(t_mwalk, 4), "rows_per_s": round(B / (t_call * 1e-3)),
            }), flush=True)
            del xm, out
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
