"""A numpy restatement of interval evidence (`HipCircuit.interval_log_prob`, cirkit_amd/csrc/ck_interval.hip), for tests only.

The contract of DESIGN.md section 11 ("Interval evidence") on the USER's plan, with parameters from the oracle
(`eval_param`), in fp64 -- or, with ``dtype=np.float32``, the yardstick of the GPU tolerances: the same layers in fp32.  The
inner layers, `_log_table` and `_lse` are those of the posterior restatement's upward pass; only the leaves differ.

A unit of a Categorical / Binomial layer with C states, on the bounds (lo, hi) of its variable (ceil(lo), floor(hi) of
floating-point bounds): lo < 0 and hi < 0, or a NaN in either, integrates the variable -- the layer's integral, lse_c of a
logit table and 0 otherwise, exactly what the marginal forward emits; else lo' = max(lo, 0), hi' = min(hi, C - 1): -inf if
lo' > hi', table[lo'] if lo' == hi', the integral if the range is full (C > 1), else log sum_c exp(table[c]) over the range --
in fp32 the terms exp(t_c - max) are added one by one, in order.  A Gaussian unit: log_partition (or 0) + log(Phi(b) - Phi(a)),
a = (lo - mean) / stddev, b = (hi - mean) / stddev, the mass (erfc(-b / sqrt 2) - erfc(-a / sqrt 2)) / 2 after (a, b) ->
(-b, -a) where a + b > 0; NaN in either bound: log_partition (or 0); lo >= hi: -inf.  In fp32 the Gaussian leaf is this fp64
formula on the fp32 parameters, rounded once.
"""
from __future__ import annotations

import numpy as np
from scipy.special import erfc

from cirkit_amd.plan import Plan, resolve_fold_index
from mpe_restatement import _entries
from posterior_restatement import _log_table, _lse


def gaussian_leaf(lo, hi, mean, sd, lp=None) -> np.ndarray:
    """log_partition + log mass of [lo, hi] under N(mean, sd^2), fp64; the arguments broadcast."""
    lo, hi, mean, sd = (np.asarray(a, dtype=np.float64) for a in (lo, hi, mean, sd))
    lp = np.zeros(()) if lp is None else np.asarray(lp, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = 1.0 / (sd * np.sqrt(2.0))
        a, b = (lo - mean) * inv, (hi - mean) * inv
        flip = a + b > 0
        a, b = np.where(flip, -b, a), np.where(flip, -a, b)
        mass = 0.5 * (erfc(-b) - erfc(-a))
        y = lp + np.log(mass)
    shape = y.shape
    lo, hi, lp = np.broadcast_to(lo, shape), np.broadcast_to(hi, shape), np.broadcast_to(lp, shape)
    y = np.where(lo < hi, y, -np.inf)
    return np.where(np.isnan(lo) | np.isnan(hi), lp, y)


def discrete_bounds(lo: np.ndarray, hi: np.ndarray, C: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(integrated, lo', hi') of one variable's (B,) bounds for a layer of C states."""
    nan = np.isnan(lo) | np.isnan(hi)
    l = np.ceil(np.where(nan, -1.0, np.maximum(lo, -(2.0**40)))).astype(np.int64)
    h = np.floor(np.where(nan, -1.0, np.minimum(hi, 2.0**40))).astype(np.int64)
    integ = nan | ((l < 0) & (h < 0))
    return integ, np.maximum(l, 0), np.minimum(h, C - 1)


def interval_restated(plan: Plan, tensors, lo, hi, *, dtype=np.float64) -> dict:
    """``y`` (B, O, K), the log mass of every row's box at the circuit's outputs, and ``vals``, the (F, B, K) values of every
    layer.  `lo`, `hi` (B, D), inclusive."""
    from oracle.torch_oracle import as_torch, eval_param

    dt = np.dtype(dtype).type
    tt = {k: (v.double() if not v.is_complex() else v) for k, v in as_torch(tensors).items()}
    lo = np.asarray(lo, dtype=np.float64)
    hi = np.asarray(hi, dtype=np.float64)
    B = lo.shape[0]
    folds = [l.num_folds for l in plan.layers]
    vals: list[np.ndarray] = []
    for l in plan.layers:
        p = {pn: eval_param(pg, tt) for pn, pg in l.params.items()}
        F, K = l.num_folds, l.num_output_units
        y = np.empty((F, B, K), dtype=dt)
        if l.inputs is None and l.type == "gaussian":
            mean, sd = p["mean"].numpy().astype(dt), p["stddev"].numpy().astype(dt)
            lp = p["log_partition"].numpy().astype(dt) if "log_partition" in p else np.zeros((F, K), dtype=dt)
            for f in range(F):
                v = int(l.scope_idx[f, 0])
                y[f] = gaussian_leaf(lo[:, v, None], hi[:, v, None], mean[f][None], sd[f][None], lp[f][None]).astype(dt)
        elif l.inputs is None:
            tab = _log_table(l, p, dt)  # (F, K, C)
            C = tab.shape[2]
            integ = _lse(tab, 2) if (l.type == "categorical" and "logits" in p) else np.zeros((F, K), dtype=dt)
            for f in range(F):
                v = int(l.scope_idx[f, 0])
                whole, a, b = discrete_bounds(lo[:, v], hi[:, v], C)
                for n in range(B):
                    if whole[n] or (a[n] == 0 and b[n] == C - 1 and C > 1):
                        y[f, n] = integ[f]
                    elif a[n] > b[n]:
                        y[f, n] = -np.inf
                    elif a[n] == b[n]:
                        y[f, n] = tab[f][:, a[n]]
                    else:
                        t = tab[f][:, a[n] : b[n] + 1]
                        m = t.max(axis=1, keepdims=True)
                        m = np.where(np.isfinite(m), m, 0).astype(dt)
                        with np.errstate(divide="ignore"):
                            # (cumsum adds in order, one term at a time, in the array's own precision)
                            y[f, n] = np.log(np.cumsum(np.exp(t - m), axis=1, dtype=dt)[:, -1]) + m[:, 0]
        else:
            ch = resolve_fold_index(l.inputs, folds)
            cvs = [np.stack([vals[ch[f, h, 0]][ch[f, h, 1]] for h in range(l.arity)]) for f in range(F)]  # (H, B, Ki)
            if l.type == "hadamard":
                for f in range(F):
                    y[f] = cvs[f].sum(0)
            elif l.type == "kronecker":
                for f in range(F):
                    acc = cvs[f][0]
                    for h in range(1, l.arity):
                        acc = (acc[:, :, None] + cvs[f][h][:, None, :]).reshape(B, -1)
                    y[f] = acc
            else:
                w = p["weight"].numpy().astype(dt)
                w = np.where(w > 0, w, 0).astype(dt)  # (F, Ko, M)
                with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                    lw = np.log(w)
                    for f in range(F):
                        y[f] = _lse(_entries(l, cvs[f])[:, None, :] + lw[f][None], 2)
        vals.append(y)
    out = resolve_fold_index(plan.output, folds).reshape(-1, 2)
    return {"y": np.stack([vals[p][f] for p, f in out], axis=1), "vals": vals}
