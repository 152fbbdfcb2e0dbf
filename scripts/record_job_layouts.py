"""Record the launch cost model of the training step's job form over a grid into tests/golden/job_layouts.json (no device needed).

    python scripts/record_job_layouts.py [--out tests/golden/job_layouts.json]

How a level's jobs are cut into units -- row splits per job and waves per workgroup of a sum launch, row split of a mixing
launch -- is arithmetic on (jobs, tiles or rows, CUs, direction): `sum_layout` and `mix_split` of cirkit_amd/job_layout.py.
This script carries its own copy of that arithmetic as it stood inside `JobStep.bind` when the fixture was first recorded
(`parent_sum_layout`, `parent_mix_split`: the closures verbatim, their free variables turned into arguments), so that it runs
unchanged on any commit; tests/test_job_graph.py compares the module's functions with what it recorded.  Splits are stored
run-length encoded: [[splits, jobs], ...]."""

from __future__ import annotations

import argparse
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "job_layouts.json")

N_JOBS = (1, 2, 20, 36, 255, 256, 257, 512, 513, 560, 1040, 1060, 6272)
TILES = (1, 2, 5, 8, 10, 32, 128)
N_CU = (256, 304)
MIX_N_JOBS = (1, 4, 59, 344, 1119)
MIX_B = (32, 150, 256, 320, 1024)
MIX_FWD_WG = 8  # the default of CK_MIX_FWD_WG


def parent_sum_layout(n_jobs: int, tiles: int, n_cu: int, backward: bool) -> tuple[list[int], int]:
    def sum_config(n_jobs: int, backward: bool) -> tuple[int, int]:
        best, best_t = (1, 4), None
        for waves in ((4, 8) if backward else (4,)):
            slots = n_cu * ((2 if waves == 4 else 1) if backward else 4)
            for sp in (1, 2, 3, 4, 6, 8, 12, 16):
                if sp > 1 and -(-tiles // sp) < waves:  # (at least a tile per wave)
                    break
                per_wave = -(-(-(-tiles // sp)) // waves)
                if backward:
                    shared = waves == 8 or n_jobs * sp > n_cu
                    unit = 10.0 + (10.0 if sp > 1 else 0.0) + (14.0 if shared else 10.0) * per_wave
                else:
                    unit = 3.0 + 6.0 * per_wave
                t = -(-n_jobs * sp // slots) * unit
                if best_t is None or t < best_t - 1e-9:
                    best, best_t = (sp, waves), t
        return best

    def sum_layout(n_jobs: int, backward: bool) -> tuple[list[int], int]:
        sp, waves = sum_config(n_jobs, backward)
        if not backward:
            return [sp] * n_jobs, waves

        def unit(s_: int, w_: int, shared: bool) -> float:
            per_wave = -(-(-(-tiles // s_)) // w_)
            return 10.0 + (10.0 if s_ > 1 else 0.0) + (14.0 if shared else 10.0) * per_wave

        slots_u = n_cu * (2 if waves == 4 else 1)
        t_uniform = -(-n_jobs * sp // slots_u) * unit(sp, waves, waves == 8 or n_jobs * sp > n_cu)
        best = ([sp] * n_jobs, waves, t_uniform)
        for w_ in (4, 8):
            slots = n_cu * (2 if w_ == 4 else 1)
            full = (n_jobs // slots) * slots
            rem = n_jobs - full
            if full == 0 or rem == 0:
                continue
            for sr in (2, 3, 4, 6, 8, 12, 16):
                if -(-tiles // sr) < w_:
                    break
                t = (full // slots) * unit(1, w_, True) + -(-rem * sr // slots) * unit(sr, w_, True)
                if t < best[2] - 1e-9:
                    best = ([1] * full + [sr] * rem, w_, t)
        return best[0], best[1]

    return sum_layout(n_jobs, backward)


def parent_mix_split(n_jobs: int, B: int, n_cu: int, backward: bool, fwd_wg: int) -> tuple[int, int]:
    def splits_for(n_jobs: int, max_split: int) -> int:
        return int(max(1, min(max_split, -(-2 * n_cu // max(1, n_jobs)))))

    ns = splits_for(n_jobs, max(1, B // 64))
    if not backward:
        ns = int(max(1, min(max(1, B // 64), -(-fwd_wg * n_cu // max(1, n_jobs)))))
    rows_per = -(-(-(-B // ns)) // 16) * 16
    ns = -(-B // rows_per)
    return ns, rows_per


def run_lengths(splits: list[int]) -> list[list[int]]:
    out: list[list[int]] = []
    for s in splits:
        if out and out[-1][0] == s:
            out[-1][1] += 1
        else:
            out.append([s, 1])
    return out


def record(sum_layout=parent_sum_layout, mix_split=parent_mix_split) -> dict:
    """The grid through a pair of layout functions (the copies above by default)."""
    sums, mixes = [], []
    for n_cu in N_CU:
        for backward in (False, True):
            for n_jobs in N_JOBS:
                for tiles in TILES:
                    splits, waves = sum_layout(n_jobs, tiles, n_cu, backward)
                    sums.append([n_jobs, tiles, n_cu, int(backward), run_lengths(list(splits)), int(waves)])
            for n_jobs in MIX_N_JOBS:
                for B in MIX_B:
                    ns, rows_per = mix_split(n_jobs, B, n_cu, backward, MIX_FWD_WG)
                    mixes.append([n_jobs, B, n_cu, int(backward), int(ns), int(rows_per)])
    return {"sum": sums, "mix": mixes, "mix_fwd_wg": MIX_FWD_WG}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    doc = record()
    remainder = [r for r in doc["sum"] if len(r[4]) > 1]
    eight = [r for r in doc["sum"] if r[5] == 8]
    if not remainder or not eight:
        raise SystemExit("the grid must hold a point where the remainder layout wins and one where eight waves win")
    print(f"{len(doc['sum'])} sum points ({len(remainder)} remainder layouts, {len(eight)} with eight waves), {len(doc['mix'])} mixing points")
    with open(args.out, "w", encoding="utf-8") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
