"""The contract of the class head (`ck_class_head`, cirkit_amd/csrc/ck_class.hip) restated in fp64 numpy: what the GPU tests
compare the kernel against, itself pinned against torch's fp64 autograd in tests/test_class_head_restatement.py.

    j = l + pi,  e = logsumexp_c j,  q = j - e
    labelled row (0 <= y < C): gen = j_y, disc = q_y;   unlabelled (y = -1): gen = e, disc = 0;   anything else: bad
    L = -(1 / gB) sum_live (w_gen gen + w_disc disc)
    seed = dL/dl: -(1 / gB) [w_gen d(c, y) + w_disc (d(c, y) - exp q)]  |  -(1 / gB) w_gen exp q
    dead row: e not finite, a NaN in the row, a labelled row with j_y = -inf (here also: a bad label) -- zero seed, left out
    of every sum.  Entries with j = -inf in a live row get seed 0.
    stats = [sum gen, sum disc, live, labelled live, correct among labelled live, dead]
"""
from dataclasses import dataclass

import numpy as np


@dataclass
class Head:
    loss: float
    stats: np.ndarray  # (6,) fp64
    seed: np.ndarray  # (B, C) fp64
    log_post: np.ndarray  # (B, C) fp64, NaN rows where e is not finite
    log_evid: np.ndarray  # (B,)
    pred: np.ndarray  # (B,) int64, -1 where e is not finite
    dead: np.ndarray  # (B,) bool
    bad: bool
    joint: np.ndarray  # (B, C) fp64
    gen: np.ndarray  # (B,) fp64, 0 on dead rows
    disc: np.ndarray  # (B,) fp64, 0 on dead and unlabelled rows


def uniform_log_prior(C: int) -> np.ndarray:
    """-log C as the fp32 number the kernel adds."""
    return np.full(C, np.float32(-np.log(float(C))), dtype=np.float32)


def class_head(l, y=None, log_prior=None, w_gen=1.0, w_disc=1.0, global_batch=None) -> Head:
    l = np.asarray(l, dtype=np.float64)
    B, C = l.shape
    pi = (uniform_log_prior(C) if log_prior is None else np.asarray(log_prior)).astype(np.float64)
    y = np.full(B, -1, dtype=np.int64) if y is None else np.asarray(y, dtype=np.int64)
    gB = float(global_batch or B)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        j = l + pi[None, :]
        has_nan = np.isnan(j).any(axis=1)
        m = np.where(has_nan, np.nan, np.max(np.where(np.isnan(j), -np.inf, j), axis=1))
        e = m + np.log(np.exp(j - m[:, None]).sum(axis=1))
        e = np.where(np.isfinite(m), e, np.where(np.isneginf(m), -np.inf, np.nan))  # (inf - inf above)
        finite_e = np.isfinite(e)
        q = np.where(finite_e[:, None], j - e[:, None], np.nan)
    bad_rows = (y < -1) | (y >= C)
    labelled = (y >= 0) & (y < C)
    rows = np.arange(B)
    jy = np.where(labelled, j[rows, np.clip(y, 0, C - 1)], 0.0)
    dead = ~finite_e | bad_rows | (labelled & np.isneginf(jy))
    live = ~dead
    qy = np.where(labelled & live, q[rows, np.clip(y, 0, C - 1)], 0.0)
    gen = np.where(live, np.where(labelled, jy, e), 0.0)
    disc = np.where(live & labelled, qy, 0.0)
    with np.errstate(invalid="ignore"):
        p = np.where(np.isneginf(j), 0.0, np.exp(q))
    delta = np.zeros((B, C))
    delta[rows[labelled], y[labelled]] = 1.0
    seed = np.where(labelled[:, None], -(w_gen * delta + w_disc * (delta - p)), -(w_gen * p)) / gB
    seed = np.where(live[:, None] & ~np.isneginf(j), seed, 0.0)
    pred = np.where(finite_e, np.argmax(np.where(np.isnan(j), -np.inf, j), axis=1), -1).astype(np.int64)  # (first maximum)
    stats = np.array([gen.sum(), disc.sum(), live.sum(), (live & labelled).sum(), (live & labelled & (pred == y)).sum(), dead.sum()],
                     dtype=np.float64)
    loss = -(w_gen * gen.sum() + w_disc * disc.sum()) / gB
    return Head(loss, stats, seed, q, e, pred, dead, bool(bad_rows.any()), j, gen, disc)
