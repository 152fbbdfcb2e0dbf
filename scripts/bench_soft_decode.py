#!/usr/bin/env python3
"""Throughput of decoding under soft evidence (`HipCircuit.soft_mpe`, `HipCircuit.sample_soft`, DESIGN.md section 11
"Decoding under soft evidence") at BASELINE config 2 (QuadTree-2, Categorical-256, K = 32): 4096 rows, the lower half of
the image soft with the noisy-channel evidence log_lik = -(c - y)^2 / 8 around a sampled pixel y, the upper half observed;
scripts/bench_soft_evidence.py's inputs and protocol.

    python scripts/bench_soft_decode.py [--reps 20] [--warmup 5] [--rows 4096]

HIP events around each timed call after `--warmup` untimed ones; the median is reported.  Timed: both calls end to end; the
max leaf, the two walks and the decode leaf in both modes alone (replayed on the arenas and the node buffer the calls left);
and, for scale, `mpe`, `sample_conditional` and `soft_evidence_log_prob` on the same rows.  The max leaf's time goes beside
its add-and-max pairs (B F_soft K C), the decode leaf's beside the B S C 4 bytes of log_lik it must stream.  Prints one JSON
line.
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
from cirkit_amd.soft_decode import ARGMAX, DRAW, _state  # noqa: E402


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
    ap.add_argument("--rows", type=int, default=4096)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    name, B, seed = "cfg2_qt784", args.rows, 11
    plan = Plan.load(os.path.join(ROOT, "tests", "golden", name))
    hc = HipCircuit(plan, init_plan_tensors(plan), device=dev)
    D = plan.num_variables
    soft = list(range(D // 2, D))  # the lower half of the 28 x 28 image
    x = hc.sample(B, seed=2)
    c = torch.arange(256, device=dev, dtype=torch.float32)
    ll = (-((c[None, None, :] - x[:, soft].to(torch.float32)[:, :, None]) ** 2) / 8.0).contiguous()
    S = len(soft)

    def soft_mpe():
        return hc.soft_mpe(ll, x, soft_vars=soft, return_log_value=True)

    def sample_soft():
        return hc.sample_soft(ll, x, soft_vars=soft, seed=seed, return_log_evidence=True)

    mo, mv = soft_mpe()
    so, sv = sample_soft()  # (binds the chunks, builds the tables)
    st, ids = _state(hc, ll, x, soft)
    s, m = st.s, st.mpe
    zc = s._z_circuit()
    stream = torch.cuda.current_stream(dev).cuda_stream
    q, d = st._set(ids)
    xm, _ = st.soft._evidence(ll, x, ids)
    bad = torch.zeros(B, dtype=torch.int32, device=dev)
    val = torch.empty(B, dtype=torch.float32, device=dev)
    node = torch.full((B, S), -1, dtype=torch.int32, device=dev)
    out = xm.clone()
    xf = 1 if s.float_out else 0
    mchunks = chunk_rows(B, None, m.bytes_per_row)
    schunks = chunk_rows(B, None, hc.arena_bytes(1))

    def max_leaf():
        for r0, nb in mchunks:
            for j in q["spos"]:
                st.max_leaf(j, q, ll[r0 : r0 + nb], nb, bad[r0:], stream)

    def mpe_walk():
        for r0, nb in mchunks:
            arena, val_off, _ = m._arena(nb)
            capi.call("ck_soft_mpe_walk", s._table.data_ptr(), m._logw_tab.data_ptr(), m._amax_tab.data_ptr(),
                      d["spos_tab"].data_ptr(), len(s.layers), s.root_fold, 0, s.total_folds, s.S, arena.data_ptr(),
                      val_off.data_ptr(), bad.data_ptr(), r0, nb, B, D, S, node.data_ptr(), xm[r0].data_ptr(), out[r0].data_ptr(),
                      xf, val.data_ptr(), stream)

    def sample_walk():
        for r0, nb in schunks:
            bd = zc._bindings[nb]
            capi.call("ck_soft_sample_walk", s._table.data_ptr(), s._weight_table().data_ptr(), d["spos_tab"].data_ptr(),
                      len(s.layers), s.root_fold, 0, s.total_folds, s.S, bd.arena.data_ptr(), s._val_off_table(bd).data_ptr(),
                      bad.data_ptr(), r0, nb, B, D, seed, S, node.data_ptr(), xm[r0].data_ptr(), out[r0].data_ptr(), xf,
                      val.data_ptr(), stream)

    def leaf(mode, chunks):
        def run():
            for r0, nb in chunks:
                st.decode_leaf(mode, q, d, ll[r0 : r0 + nb], node, r0, nb, seed, out[r0], stream)

        return run

    r, w = args.reps, args.warmup
    t_mpe_all = _time(soft_mpe, r, w)
    t_max_leaf = _time(max_leaf, r, w)  # (on the arenas the last soft_mpe left)
    t_mpe_walk = _time(mpe_walk, r, w)
    t_leaf_argmax = _time(leaf(ARGMAX, mchunks), r, w)  # (on the nodes the walk above recorded)
    same_argmax = bool(torch.equal(out, mo)) if len(mchunks) == 1 else None
    t_sample_all = _time(sample_soft, r, w)
    t_sample_walk = _time(sample_walk, r, w)  # (on the bindings the last sample_soft left)
    t_leaf_draw = _time(leaf(DRAW, schunks), r, w)
    same_draw = bool(torch.equal(out, so)) if len(schunks) == 1 else None
    t_hard_mpe = _time(lambda: hc.mpe(x, soft), r, w)
    t_cond = _time(lambda: hc.sample_conditional(x, soft, seed=seed), r, w)
    t_lp = _time(lambda: hc.soft_evidence_log_prob(ll, x, soft_vars=soft), r, w)
    pairs = B * sum(int((sp >= 0).sum()) * zc.layers[j].num_output_units * zc.layers[j].num_categories
                    for j, sp in q["spos"].items())
    nbytes = ll.numel() * 4
    row = {"config": "config 2", "plan": name, "B": B, "soft_vars": S, "log_lik_bytes": nbytes,
           "soft_mpe_chunks": len(mchunks), "sample_soft_chunks": len(schunks),
           "soft_mpe_ms": round(t_mpe_all, 4), "sample_soft_ms": round(t_sample_all, 4),
           "max_leaf_ms": round(t_max_leaf, 4), "max_leaf_pairs": pairs, "max_leaf_Gpairs_per_s": round(pairs / t_max_leaf / 1e6, 1),
           "max_leaf_GBps_read": round(nbytes / t_max_leaf / 1e6, 1),
           "mpe_walk_ms": round(t_mpe_walk, 4), "sample_walk_ms": round(t_sample_walk, 4),
           "decode_leaf_argmax_ms": round(t_leaf_argmax, 4), "decode_leaf_argmax_GBps": round(nbytes / t_leaf_argmax / 1e6, 1),
           "decode_leaf_draw_ms": round(t_leaf_draw, 4), "decode_leaf_draw_GBps": round(nbytes / t_leaf_draw / 1e6, 1),
           "mpe_ms": round(t_hard_mpe, 4), "sample_conditional_ms": round(t_cond, 4), "soft_evidence_log_prob_ms": round(t_lp, 4),
           "finite_rows": int(torch.isfinite(mv).sum()), "replay_equals_call": [same_argmax, same_draw],
           "soft_mpe_returns_y": float((mo[:, soft] == x[:, soft]).float().mean()),
           "sample_soft_returns_y": float((so[:, soft] == x[:, soft]).float().mean())}
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
