"""A numpy restatement of the autoregressive conditionals and the coding tables (`HipCircuit.autoregressive_conditionals`,
`autoregressive_log_probs`, `coding_tables`; cirkit_amd/csrc/ck_ar.hip), for tests only.

The contract of DESIGN.md section 11 ("Autoregressive conditionals and coding") on the USER's plan: the rows are expanded on
the host, `leave_one_out_restated` (tests/loo_restatement.py) runs on the expanded batch with a mask per row, and the
diagonal -- expanded row (b, i) at variable order[i] -- is the answer, in fp64 or, with ``dtype=np.float32``, the same
formulas in fp32: the yardstick of the GPU tolerances.  The expanded row (b, i) KEEPS the value at order[i] (the mask hides
the steps > i): the leave-one-out conditional of a variable does not depend on the variable's own value -- the derivative
with respect to its input units never reads them --, so the conditionals are those of the row with order[i] hidden too,
and `logp` can read the value.  Also here: the numpy quantiser (the rule of `ck_ar_quantise`, integer for integer) and a
brute force by enumeration on the oracle for the tiniest plans.
"""
from __future__ import annotations

import numpy as np

from loo_restatement import leave_one_out_restated


def covered(plan) -> list[int]:
    return sorted({int(v) for l in plan.layers if l.inputs is None and l.scope_idx is not None for v in l.scope_idx[:, 0]})


def discrete_vars(plan) -> np.ndarray:
    d = np.zeros(plan.num_variables, dtype=bool)
    for l in plan.layers:
        if l.type in ("categorical", "binomial"):
            d[l.scope_idx[:, 0]] = True
    return d


def expand(plan, x, order=None, positions=None, *, keep_own: bool = False):
    """(xe (B P, D), mask (B P, D), order, positions): expanded row b P + j is row b with every variable order[k],
    k >= positions[j] (k > positions[j] with `keep_own`), marked missing; sentinels already in `x` are marked too."""
    x = np.asarray(x, dtype=np.float64)
    B, D = x.shape
    order = covered(plan) if order is None else [int(v) for v in order]
    positions = list(range(len(order))) if positions is None else sorted(int(i) for i in positions)
    step = np.full(D, -1, dtype=np.int64)
    step[order] = np.arange(len(order))
    first = np.asarray(positions)[:, None] + (1 if keep_own else 0)  # (P, 1)
    hide = (step[None, :] >= first) & (step[None, :] >= 0)  # (P, D)
    mask = np.broadcast_to(hide[None], (B, len(positions), D)).reshape(-1, D).copy()
    xe = np.repeat(x, len(positions), axis=0)
    mask |= np.isnan(xe) | ((xe <= -1) & discrete_vars(plan)[None])
    return xe, mask, order, positions


def autoregressive_restated(plan, tensors, x, order=None, positions=None, *, dtype=np.float64) -> dict:
    """``p`` (B, P, C) -- (B, P, 2) mean and variance for an all-Gaussian order, None for a mixed one --, ``logp`` (B, P)
    log p(x_{order[i]} | x_{order[:i]}) (0 where the row misses order[i]), ``missing`` (B, P) where that is, ``order`` and
    ``positions``."""
    xe, mask, order, positions = expand(plan, x, order, positions, keep_own=True)
    B, P = np.asarray(x).shape[0], len(positions)
    kinds = {v: "d" if d else "g" for v, d in zip(range(plan.num_variables), discrete_vars(plan))}
    mixed = len({kinds[v] for v in order}) > 1
    query = [order[0]] if mixed else sorted(order)
    res = leave_one_out_restated(plan, tensors, xe, query, mask, dtype=dtype)
    rows = np.arange(B * P)
    var = np.tile(np.asarray([order[i] for i in positions]), B)
    logp = res["logp"][rows, var].reshape(B, P)
    p = None
    if not mixed:
        qi = np.asarray([res["query"].index(int(v)) for v in var])
        p = res["p"][rows, qi].reshape(B, P, -1)
    return {"p": p, "logp": logp, "missing": res["mask"][rows, var].reshape(B, P), "order": order, "positions": positions}


def log_prob_restated(plan, tensors, x, *, dtype=np.float64) -> np.ndarray:
    """(B,) log p(x) over the covered variables: the log evidence of the rows minus the log partition function."""
    x = np.asarray(x, dtype=np.float64)
    ev = leave_one_out_restated(plan, tensors, x, [covered(plan)[0]], None, dtype=dtype)["logev"]
    z = leave_one_out_restated(plan, tensors, x[:1], [covered(plan)[0]], np.ones(plan.num_variables, dtype=bool), dtype=dtype)["logev"]
    return ev - z[0]


def brute_force(plan, tensors, x, order=None):
    """(p (B, steps, C), logp (B, steps)) of a discrete plan by enumeration on the oracle: step i is one marginal forward per
    state of order[i] with the prefix observed and everything else integrated out."""
    import torch

    from oracle.torch_oracle import as_torch, evaluate_plan

    default = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        tt = {k: v.double() for k, v in as_torch(tensors).items()}
        x = np.asarray(x).astype(np.int64)
        B, D = x.shape
        order = covered(plan) if order is None else list(order)
        states = np.zeros(D, dtype=np.int64)
        for l in plan.layers:
            if l.type in ("categorical", "binomial"):
                states[l.scope_idx[:, 0]] = int(l.config["num_categories"]) if l.type == "categorical" else int(l.config["total_count"]) + 1
        C = int(states[order].max())
        joint = np.full((B, len(order), C), -np.inf)
        for i, v in enumerate(order):
            m = np.ones((B, D), dtype=bool)
            m[:, order[: i + 1]] = False
            for c in range(int(states[v])):
                xs = np.where(m, 0, x)
                xs[:, v] = c
                joint[:, i, c] = evaluate_plan(plan, tt, torch.from_numpy(xs), integrate_mask=torch.from_numpy(m))[:, 0, 0].numpy()
    finally:
        torch.set_default_dtype(default)
    mx = joint.max(axis=2, keepdims=True)
    e = np.exp(joint - mx)
    p = e / e.sum(axis=2, keepdims=True)
    logp = np.log(np.take_along_axis(p, x[:, order][:, :, None], axis=2)[:, :, 0])
    return p, logp


# -- the quantiser -----------------------------------------------------------------------------------------------------------
def quantise(p, nstates, precision: int) -> np.ndarray:
    """(rows, C + 1) int32 cumulative frequency tables of the fp32 conditionals `p` (rows, C), `nstates` (rows,) the state
    count of each row's variable: the rule of `ck_ar_quantise`.  count_c = 1 + floor(p_c (T - S)) for c < S -- the product
    rounded once to fp32 --, 0 past S; the slack T - sum, of either sign, goes to the first state with the largest count; a
    row with a value outside [0, 1] (NaN included), or whose largest count would fall below 1, is uniform: floor(T / S) each,
    the remainder to state 0."""
    p = np.asarray(p, dtype=np.float32)
    rows, C = p.shape
    T = 1 << int(precision)
    S = np.clip(np.asarray(nstates, dtype=np.int64).reshape(rows), 1, C)
    live = np.arange(C)[None, :] < S[:, None]
    with np.errstate(invalid="ignore"):
        ok = ((p >= 0) & (p <= 1)) | ~live
        scaled = p * (T - S).astype(np.float32)[:, None]  # fp32 x fp32, rounded once
        count = np.where(live & ok, 1 + np.where(ok & live, scaled, 0).astype(np.int64), 0)
    top = count.argmax(axis=1)  # (the first of the largest)
    slack = T - count.sum(axis=1)
    uniform = ~ok.all(axis=1) | (count[np.arange(rows), top] + slack < 1)
    count[np.arange(rows), top] += slack
    flat = np.where(live, (T // S)[:, None], 0)
    flat[:, 0] += T - (T // S) * S
    count = np.where(uniform[:, None], flat, count)
    out = np.zeros((rows, C + 1), dtype=np.int64)
    out[:, 1:] = np.cumsum(count, axis=1)
    return out.astype(np.int32)


def restated_tables(plan, tensors, order, precision: int, *, dtype=np.float64):
    """The table provider of cirkit_amd/codec.py from the restatement: ``tables(step, x_so_far) -> (B, C + 1)``."""
    states = np.zeros(plan.num_variables, dtype=np.int64)
    for l in plan.layers:
        if l.type in ("categorical", "binomial"):
            n = int(l.config["num_categories"]) if l.type == "categorical" else int(l.config["total_count"]) + 1
            states[l.scope_idx[:, 0]] = np.maximum(states[l.scope_idx[:, 0]], n)

    def tables(step: int, xs: np.ndarray) -> np.ndarray:
        p = autoregressive_restated(plan, tensors, xs, order, [step], dtype=dtype)["p"][:, 0]
        return quantise(p.astype(np.float32), np.full(p.shape[0], states[order[step]]), precision)

    return tables
