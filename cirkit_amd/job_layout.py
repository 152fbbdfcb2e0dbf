"""The launch cost model of the job form of the training step (cirkit_amd/train_jobs.py): how a level's jobs are cut into the
units of one launch.  Pure arithmetic on (jobs, tiles or rows, CUs, direction) -- tests/golden/job_layouts.json pins it.

A sum launch runs in ROUNDS of as many workgroups as the chip holds (backward: 2 per CU with 4 waves, 1 with 8; forward: 4 per
CU) and a round lasts as long as one unit, so 1040 jobs on 512 slots take three rounds where 2.03 would do -- finer units waste
less of the last round, at a fixed cost per unit.  Measured [MI355X, scripts/exp_jobs_fixed.py]: a backward unit costs ~10 us
beside its tiles (launch, weights staged, accumulators reduced, optimizer epilogue), ~10 us more when its partial sums of dW go
through memory, and a tile ~10 us of a wave that has its SIMD to itself, ~14 us when two waves share it; forward ~3 us + 6 us per
tile.  Eight waves halve a unit's chain of tiles (what the few-fold levels at the top of a circuit consist of)."""
from __future__ import annotations


def unit(tiles: int, splits: int, waves: int, backward: bool, shared: bool) -> float:
    """The modelled time (us) of one unit: a job's rows cut in `splits`, its tiles dealt over `waves` waves; `shared`: two waves
    on a SIMD."""
    per_wave = -(-(-(-tiles // splits)) // waves)
    if not backward:
        return 3.0 + 6.0 * per_wave
    return 10.0 + (10.0 if splits > 1 else 0.0) + (14.0 if shared else 10.0) * per_wave


def sum_layout(n_jobs: int, tiles: int, n_cu: int, backward: bool) -> tuple[list[int], int]:
    """(row splits of every job, waves per workgroup) of a sum launch: the cheapest uniform split, or -- a backward launch of
    more jobs than the chip holds -- whole jobs for the full rounds and only the REMAINDER cut fine, issued last: 1060 jobs on
    512 slots are two rounds of whole jobs + 36 jobs in 8 pieces each instead of three rounds."""
    best: tuple[list[int], int, float] | None = None
    for waves in ((4, 8) if backward else (4,)):
        slots = n_cu * ((2 if waves == 4 else 1) if backward else 4)
        for sp in (1, 2, 3, 4, 6, 8, 12, 16):
            if sp > 1 and -(-tiles // sp) < waves:  # (at least a tile per wave)
                break
            t = -(-n_jobs * sp // slots) * unit(tiles, sp, waves, backward, waves == 8 or n_jobs * sp > n_cu)
            if best is None or t < best[2] - 1e-9:
                best = ([sp] * n_jobs, waves, t)
    for waves in ((4, 8) if backward else ()):
        slots = n_cu * (2 if waves == 4 else 1)
        full = (n_jobs // slots) * slots
        rem = n_jobs - full
        if full == 0 or rem == 0:
            continue
        for sr in (2, 3, 4, 6, 8, 12, 16):
            if -(-tiles // sr) < waves:
                break
            t = (full // slots) * unit(tiles, 1, waves, True, True) + -(-rem * sr // slots) * unit(tiles, sr, waves, True, True)
            if t < best[2] - 1e-9:
                best = ([1] * full + [sr] * rem, waves, t)
    return best[0], best[1]


def mix_split(n_jobs: int, B: int, n_cu: int, backward: bool, fwd_wg_per_cu: int) -> tuple[int, int]:
    """(row splits per job, rows per split) of a mixing launch: two workgroups per CU backward; the forward has no sums over
    the rows, so `fwd_wg_per_cu` of them (eight: a workgroup is a chain of one round trip per 16 rows, and 256 threads with
    4 KB of LDS leave room for eight).  At least 64 rows per split, in whole 16-row steps."""
    per_cu = 2 if backward else fwd_wg_per_cu
    ns = int(max(1, min(max(1, B // 64), -(-per_cu * n_cu // max(1, n_jobs)))))
    rows_per = -(-(-(-B // ns)) // 16) * 16
    return -(-B // rows_per), rows_per
