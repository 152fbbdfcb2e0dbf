"""A numpy restatement of soft (likelihood) evidence (`HipCircuit.soft_evidence_log_prob`,
`HipCircuit.soft_posterior_marginals`, cirkit_amd/csrc/ck_soft.hip), for tests only.

The contract of DESIGN.md section 11 ("Soft evidence") on the USER's plan, with parameters from the oracle (`eval_param`), in
fp64 -- or, with ``dtype=np.float32``, the yardstick of the GPU tolerances: the same layers in fp32.  The inner layers,
`_log_table`, `_lse` and `_entries` are those of the interval and posterior restatements; only the leaves differ.

Upward.  A unit k of a Categorical / Binomial fold over the s-th soft variable emits log sum_{c < C} exp(log_lik[n, s, c] +
table[k, c]), C the layer's states -- in fp32 the terms exp(. - max) are added one by one, in order; every term -inf: -inf; a
NaN or +inf in a read entry: the row is NaN.  Every other input unit is the marginal forward's: observed at x[n, v], or the
layer's integral where x holds the sentinel (NaN; a value <= -1 of a variable a discrete layer reads) or is None.

Downward, the flow pass of the posterior restatement, f(root) = 1.  The posterior of soft variable s:
p[n, s, c] = sum over its input folds and their units k of f_k exp(table[k, c] + log_lik[n, s, c] - v_k), v_k the unit's own
upward value -- d log Z / d log_lik[n, s, c].  0 at c >= C.  Rows without a finite root value are NaN.
"""
from __future__ import annotations

import numpy as np

from cirkit_amd.plan import Plan, resolve_fold_index
from mpe_restatement import _entries
from posterior_restatement import _log_table, _lse


def soft_restated(plan: Plan, tensors, log_lik, x, soft_vars, dtype=np.float64) -> dict:
    """``y`` (B, O, K), ``vals`` (one (F, B, K) array per layer), ``p`` (B, S, Cl) and ``logev`` (B,).  `log_lik` (B, S, Cl);
    `x` (B, D) or None; `soft_vars` the soft variable ids."""
    from oracle.torch_oracle import as_torch, eval_param

    dt = np.dtype(dtype).type
    tt = {k: (v.double() if not v.is_complex() else v) for k, v in as_torch(tensors).items()}
    D = plan.num_variables
    ll = np.asarray(log_lik, dtype=np.float64).astype(np.float32).astype(dt)  # (staged as fp32 on the device)
    B, S, Cl = ll.shape
    soft = sorted(int(v) for v in soft_vars)
    assert len(soft) == S
    spos = {v: i for i, v in enumerate(soft)}
    x = np.full((B, D), np.nan) if x is None else np.asarray(x, dtype=np.float64)[:, :D]
    discrete = np.zeros(D, dtype=bool)
    for l in plan.layers:
        if l.type in ("categorical", "binomial"):
            discrete[l.scope_idx[:, 0]] = True
    mask = np.isnan(x) | ((x <= -1) & discrete)
    folds = [l.num_folds for l in plan.layers]
    params = [{pn: eval_param(pg, tt) for pn, pg in l.params.items()} for l in plan.layers]
    tabs: dict[int, np.ndarray] = {}
    ws: dict[int, np.ndarray] = {}
    chs: dict[int, np.ndarray] = {}
    vals: list[np.ndarray] = []
    rowbad = np.zeros(B, dtype=bool)
    for j, l in enumerate(plan.layers):  # upward
        p = params[j]
        F, K = l.num_folds, l.num_output_units
        y = np.empty((F, B, K), dtype=dt)
        if l.inputs is None:
            if l.type == "gaussian":
                mean, sd = p["mean"].numpy().astype(dt), p["stddev"].numpy().astype(dt)
                lp = p["log_partition"].numpy().astype(dt) if "log_partition" in p else np.zeros((F, K), dtype=dt)
            else:
                tab = tabs[j] = _log_table(l, p, dt)  # (F, K, C)
                C = tab.shape[2]
                integ = _lse(tab, 2) if (l.type == "categorical" and "logits" in p) else np.zeros((F, K), dtype=dt)
            for f in range(F):
                v = int(l.scope_idx[f, 0])
                m = mask[:, v]
                if l.type == "gaussian":
                    assert v not in spos, "a Gaussian variable cannot carry soft evidence"
                    xv = np.where(m, 0.0, x[:, v]).astype(dt)[:, None]
                    y[f] = -((xv - mean[f]) ** 2) / (dt(2) * sd[f] ** 2) - np.log(sd[f]) - dt(0.5 * np.log(2.0 * np.pi)) + lp[f]
                    y[f, m] = lp[f]
                elif v in spos:
                    lv = ll[:, spos[v], :C]  # (B, C)
                    nan = (np.isnan(lv) | (lv == np.inf)).any(axis=1)
                    rowbad |= nan
                    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                        t = np.where(nan[:, None, None], dt(0), lv[:, None, :] + tab[f][None])  # (B, K, C)
                        mx = t.max(axis=2, keepdims=True)
                        mx = np.where(np.isfinite(mx), mx, 0).astype(dt)
                        # (cumsum adds in order, one term at a time, in the array's own precision)
                        y[f] = np.log(np.cumsum(np.exp(t - mx), axis=2, dtype=dt)[:, :, -1]) + mx[:, :, 0]
                    y[f, nan] = np.nan
                else:
                    c = np.where(m, 0, x[:, v]).astype(np.int64)
                    y[f] = tab[f][:, c].T
                    y[f, m] = integ[f]
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
            w = p["weight"].numpy().astype(dt)
            w = ws[j] = np.where(w > 0, w, 0).astype(dt)  # (F, Ko, M)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                lw = np.log(w)
                for f in range(F):
                    y[f] = _lse(_entries(l, cvs[f])[:, None, :] + lw[f][None], 2)
        vals.append(y)
    out = resolve_fold_index(plan.output, folds).reshape(-1, 2)
    yout = np.stack([vals[p][f] for p, f in out], axis=1)
    yout[rowbad] = np.nan
    root = out[0]
    logev = vals[root[0]][root[1], :, 0].copy()
    logev[rowbad] = np.nan
    flows = [np.zeros((F, B, l.num_output_units), dtype=dt) for F, l in zip(folds, plan.layers)]
    flows[root[0]][root[1], :, 0] = 1
    post = np.zeros((B, S, Cl), dtype=dt)
    for j in range(len(plan.layers) - 1, -1, -1):  # downward, flows
        l = plan.layers[j]
        Ki = l.num_input_units
        for f in range(l.num_folds):
            fk = flows[j][f]
            if l.inputs is None:
                v = int(l.scope_idx[f, 0])
                if v not in spos:
                    continue
                tab = tabs[j][f]  # (K, C)
                C = tab.shape[1]
                lv, vk = ll[:, spos[v], :C], vals[j][f]  # (B, C), (B, K)
                with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                    keep = (fk > 0) & np.isfinite(vk)
                    e = (tab[None] + lv[:, None, :]) - np.where(keep, vk, 0)[:, :, None]  # (B, K, C)
                    term = np.where(keep[:, :, None], fk[:, :, None] * np.exp(np.minimum(e, 0)), 0).astype(dt)
                post[:, spos[v], :C] += np.where(np.isnan(term), 0, term).sum(axis=1)
                continue
            ch = chs[j]
            kids = [flows[ch[f, h, 0]][ch[f, h, 1]] for h in range(l.arity)]
            if l.type == "hadamard":
                for k in kids:
                    k += fk
                continue
            if l.type == "kronecker":
                cube = fk.reshape((B,) + (Ki,) * l.arity)
                for h, k in enumerate(kids):
                    k += cube.sum(axis=tuple(a + 1 for a in range(l.arity) if a != h))
                continue
            v = vals[j][f]
            cv = np.stack([vals[ch[f, h, 0]][ch[f, h, 1]] for h in range(l.arity)])
            e = _entries(l, cv)  # (B, M)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                keep = (fk > 0) & np.isfinite(v)
                lg = np.where(keep, np.log(np.where(keep, fk, 1)) - np.where(keep, v, 0), -np.inf).astype(dt)
                m = lg.max(axis=1, keepdims=True)
                a = np.where(keep, np.exp(lg - np.where(np.isfinite(m), m, 0)), 0).astype(dt)
                T = a @ ws[j][f]  # (B, M)
                ok = (T > 0) & np.isfinite(e)
                fl = np.where(ok, np.exp(m + np.where(ok, e, 0) + np.log(np.where(ok, T, 1))), 0).astype(dt)
            if l.type == "sum":
                for h, k in enumerate(kids):
                    k += fl[:, h * Ki : (h + 1) * Ki]
            elif l.type == "cpt":
                for k in kids:
                    k += fl
            else:
                sq = fl.reshape(B, Ki, Ki)
                kids[0] += sq.sum(2)
                kids[1] += sq.sum(1)
    post[~np.isfinite(logev)] = np.nan
    return {"y": yout, "vals": vals, "p": post, "logev": logev}
