"""A numpy restatement of the most probable explanation (`HipCircuit.mpe`, cirkit_amd/csrc/ck_mpe.hip), for tests only.

The contract of DESIGN.md section 11 ("Most probable explanation") in fp64 on the USER's plan, with parameters from the
oracle (`eval_param`).  Upward, max-product: a sum / mixing / CP-T / Tucker unit takes max_i (log w_i + v_i) over the entries
with w_i > 0 (v_i: the entry's child value, CP-T summed over the inputs, Tucker v0[a] + v1[b]); Hadamard and Kronecker units
add their children's values; an input unit gives log p(x_v) where x_v is observed and max_c log p(c) where it is maximised
(a Gaussian: its log density at the mean).  Downward, every unit on the row's tree takes its argmax entry, the smallest
index on ties (numpy's argmax); a maximised variable takes its unit's argmax category or the Gaussian mean.  A row whose root
value is not finite takes nothing.  `near` marks the rows on whose tree some argmax wins by less than `tol`.
"""
from __future__ import annotations

import numpy as np
import torch

from cirkit_amd.plan import Plan, resolve_fold_index


def _is_mixing(l) -> bool:
    g = l.params["weight"]
    return l.type == "sum" and len(g.output.ids) == 1 and g.nodes[g.output.ids[0]].op == "mixing_weight"


def _log_table(l, params) -> np.ndarray:
    """(F, K, C) log-probabilities of a Categorical / Binomial layer, fp64."""
    if l.type == "categorical":
        if "probs" in params:
            with np.errstate(divide="ignore"):
                return np.log(params["probs"].numpy())
        return params["logits"].numpy()
    T = int(l.config["total_count"])
    p = params["probs"].numpy() if "probs" in params else 1.0 / (1.0 + np.exp(-params["logits"].numpy()))
    c = np.arange(T + 1)
    from math import lgamma

    lc = np.array([lgamma(T + 1) - lgamma(i + 1) - lgamma(T - i + 1) for i in c])
    with np.errstate(divide="ignore", invalid="ignore"):
        lp = lc + c * np.log(p[..., None]) + (T - c) * np.log1p(-p[..., None])
    return np.where(np.isnan(lp), -np.inf, lp)


def _gauss(x, mean, sd, lp):
    v = -((x - mean) ** 2) / (2.0 * sd**2) - np.log(sd) - 0.5 * np.log(2.0 * np.pi)
    return v if lp is None else v + lp


def _entries(l, cv):
    """(n, M) entry values of a sum-type fold from its children's values cv (H, n, Ki)."""
    if l.type == "cpt":
        return cv.sum(0)
    if l.type == "tucker":
        return (cv[0][:, :, None] + cv[1][:, None, :]).reshape(cv.shape[1], -1)
    return cv.transpose(1, 0, 2).reshape(cv.shape[1], -1)


def _gap(t: np.ndarray) -> np.ndarray:
    """(n,) how much the largest entry of each row of t beats the second (inf for a single entry)."""
    if t.shape[1] < 2:
        return np.full(t.shape[0], np.inf)
    s = -np.partition(-t, 1, axis=1)
    with np.errstate(invalid="ignore"):
        return s[:, 0] - s[:, 1]


def mpe_restated(plan: Plan, tensors, x, mask, *, tol: float = 1e-4):
    """(out (B, D) float64, choices [(F, B) int per sum / mixing / CP-T / Tucker layer], log value (B,), near (B,) bool).

    `x` (B, D) the evidence, `mask` a bool (B, D) / (1, D) / (D,) array of the variables to maximise; entries of `x` holding
    the sentinel (NaN; a value <= -1 of a variable read by a discrete layer) are maximised too.  Maximised entries of rows
    without mass hold the sentinel: NaN for a circuit with a Gaussian layer, -1 otherwise."""
    from oracle.torch_oracle import as_torch, eval_param

    tt = {k: (v.double() if not v.is_complex() else v) for k, v in as_torch(tensors).items()}
    D = plan.num_variables
    x = np.asarray(x, dtype=np.float64)
    B = x.shape[0]
    gauss = any(l.type == "gaussian" for l in plan.layers)
    discrete = np.zeros(D, dtype=bool)
    for l in plan.layers:
        if l.type in ("categorical", "binomial"):
            discrete[l.scope_idx[:, 0]] = True
    mask = np.broadcast_to(np.asarray(mask, dtype=bool).reshape(-1, D), (B, D))
    mask = mask | np.isnan(x) | ((x <= -1) & discrete)
    folds = [l.num_folds for l in plan.layers]
    params = [{pn: eval_param(pg, tt) for pn, pg in l.params.items()} for l in plan.layers]
    tabs: dict[int, np.ndarray] = {}
    lws: dict[int, np.ndarray] = {}
    chs: dict[int, np.ndarray] = {}
    vals: list[np.ndarray] = []
    for j, l in enumerate(plan.layers):  # upward, max-product
        p = params[j]
        F, K = l.num_folds, l.num_output_units
        y = np.empty((F, B, K))
        if l.inputs is None:
            if l.type != "gaussian":
                tabs[j] = _log_table(l, p)  # (F, K, C)
            for f in range(F):
                v = int(l.scope_idx[f, 0])
                m = mask[:, v]
                if l.type == "gaussian":
                    mean, sd = p["mean"].numpy()[f], p["stddev"].numpy()[f]
                    lp = p["log_partition"].numpy()[f] if "log_partition" in p else None
                    y[f] = _gauss(np.where(m, 0.0, x[:, v])[:, None], mean, sd, lp)
                    y[f, m] = _gauss(mean, mean, sd, lp)
                else:
                    tab = tabs[j]
                    c = np.where(m, 0, x[:, v]).astype(np.int64)
                    y[f] = tab[f][:, c].T
                    y[f, m] = tab[f].max(axis=1)
            vals.append(y)
            continue
        ch = chs[j] = resolve_fold_index(l.inputs, folds)
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
            w = p["weight"].numpy()
            with np.errstate(divide="ignore"):
                lw = lws[j] = np.where(w > 0, np.log(np.where(w > 0, w, 1.0)), -np.inf)  # (F, Ko, M)
            for f in range(F):
                y[f] = (_entries(l, cvs[f])[:, None, :] + lw[f][None]).max(axis=2)
        vals.append(y)
    root = resolve_fold_index(plan.output, folds).reshape(-1, 2)[0]
    logv = vals[root[0]][root[1], :, 0].copy()
    sel = [np.full((F, B), -1, dtype=np.int64) for F in folds]
    sel[root[0]][root[1], np.isfinite(logv)] = 0
    out = np.where(mask, np.nan if gauss else -1.0, x)
    near = np.zeros(B, dtype=bool)
    choices: dict[int, np.ndarray] = {}
    for j in range(len(plan.layers) - 1, -1, -1):  # downward, argmax
        l, p = plan.layers[j], params[j]
        if l.type in ("sum", "cpt", "tucker"):
            choices[j] = np.full((l.num_folds, B), -1, dtype=np.int64)
        for f in range(l.num_folds):
            on = np.nonzero(sel[j][f] >= 0)[0]
            if l.inputs is None:
                on = on[mask[on, int(l.scope_idx[f, 0])]]  # (observed variables keep their value)
            if on.size == 0:
                continue
            k = sel[j][f][on]
            if l.inputs is None:
                v = int(l.scope_idx[f, 0])
                if l.type == "gaussian":
                    out[on, v] = p["mean"].numpy()[f][k]
                else:
                    t = tabs[j][f][k]  # (n_on, C)
                    out[on, v] = np.argmax(t, axis=1)
                    near[on] |= _gap(t) < tol
                continue
            ch = chs[j]
            if l.type == "hadamard":
                for h in range(l.arity):
                    sel[ch[f, h, 0]][ch[f, h, 1], on] = k
                continue
            if l.type == "kronecker":
                r = k.copy()
                for h in range(l.arity - 1, -1, -1):
                    sel[ch[f, h, 0]][ch[f, h, 1], on] = r % l.num_input_units
                    r //= l.num_input_units
                continue
            Ki = l.num_input_units
            cv = np.stack([vals[ch[f, h, 0]][ch[f, h, 1]][on] for h in range(l.arity)])
            t = lws[j][f][k] + _entries(l, cv)  # (n_on, M)
            i = np.argmax(t, axis=1)
            near[on] |= _gap(t) < tol
            choices[j][f, on] = i // Ki if _is_mixing(l) else i
            if l.type == "sum":
                h, kk = np.divmod(i, Ki)
                for hh in range(l.arity):
                    m = h == hh
                    sel[ch[f, hh, 0]][ch[f, hh, 1], on[m]] = kk[m]
            elif l.type == "cpt":
                for h in range(l.arity):
                    sel[ch[f, h, 0]][ch[f, h, 1], on] = i
            else:
                a, b = np.divmod(i, Ki)
                sel[ch[f, 0, 0]][ch[f, 0, 1], on] = a
                sel[ch[f, 1, 0]][ch[f, 1, 1], on] = b
    covered = np.zeros(D, dtype=bool)
    for l in plan.layers:
        if l.inputs is None:
            covered[l.scope_idx[:, 0]] = True
    fill = mask & ~covered[None, :] & np.isfinite(logv)[:, None]  # (variables outside every input layer's scope: 0)
    out[fill] = 0.0
    return out, [choices[j] for j in sorted(choices)], logv, near
