"""A numpy restatement of the expected statistics (`HipCircuit.expected_statistics`, cirkit_amd/csrc/ck_stats.hip), for
tests only.

The contract of DESIGN.md section 11 ("Expected statistics") on the USER's plan, with parameters from the oracle
(`eval_param`), in fp64 -- or, with ``dtype=np.float32``, the same formulas in fp32: the yardstick of the GPU tolerances.
Upward: the marginal forward in log space, as tests/posterior_restatement.py.  Downward, linear space, f(root) = 1: a
sum-type unit k with f_k > 0 and a finite v_k gives entry i the term f_k w[k, i] exp(e_i - v_k) (nothing for w <= 0), which
is both the flow the entry's inputs receive and, summed over the LIVE rows (finite root value), ``edge``; ``unit`` is the
sum of f_k, ``leaf`` the flows of the input units by observed state (spread over the unit's normalised table row where the
variable is missing), for Gaussian units (sum f, sum f m1, sum f m2).
"""
from __future__ import annotations

import numpy as np

from cirkit_amd.plan import Plan, resolve_fold_index
from mpe_restatement import _entries
from posterior_restatement import _log_table, _lse


def statistics_restated(plan: Plan, tensors, x, missing=(), *, dtype=np.float64) -> dict:
    """``edge`` {layer: (F, Ko, M)}, ``leaf`` {layer: (F, K, C) | (F, K, 3)}, ``unit`` [(F, Ko)], ``logev`` (B,), ``rows``,
    and the per-row ``flows`` / ``vals`` ((F, B, K) per layer) and evaluated weights ``w`` behind them.

    `x` (B, D) the evidence, `missing` the variable ids integrated out in every row; entries of `x` holding the sentinel
    (NaN; a value <= -1 of a variable read by a discrete layer) are integrated out for their row."""
    from oracle.torch_oracle import as_torch, eval_param

    dt = np.dtype(dtype).type
    tt = {k: (v.double() if not v.is_complex() else v) for k, v in as_torch(tensors).items()}
    D = plan.num_variables
    x = np.asarray(x, dtype=np.float64)
    B = x.shape[0]
    discrete = np.zeros(D, dtype=bool)
    for l in plan.layers:
        if l.type in ("categorical", "binomial"):
            discrete[l.scope_idx[:, 0]] = True
    mask = np.zeros((B, D), dtype=bool)
    mask[:, sorted(int(v) for v in missing)] = True
    mask |= np.isnan(x) | ((x <= -1) & discrete)
    folds = [l.num_folds for l in plan.layers]
    params = [{pn: eval_param(pg, tt) for pn, pg in l.params.items()} for l in plan.layers]
    tabs, ws, chs, vals = {}, {}, {}, []
    for j, l in enumerate(plan.layers):  # upward, marginal forward
        p = params[j]
        F, K = l.num_folds, l.num_output_units
        y = np.empty((F, B, K), dtype=dt)
        if l.inputs is None:
            if l.type == "gaussian":
                mean, sd = p["mean"].numpy().astype(dt), p["stddev"].numpy().astype(dt)
                lp = p["log_partition"].numpy().astype(dt) if "log_partition" in p else np.zeros((F, K), dtype=dt)
            else:
                tab = tabs[j] = _log_table(l, p, dt)
                integ = _lse(tab, 2) if (l.type == "categorical" and "logits" in p) else np.zeros((F, K), dtype=dt)
            for f in range(F):
                v = int(l.scope_idx[f, 0])
                m = mask[:, v]
                if l.type == "gaussian":
                    xv = np.where(m, 0.0, x[:, v]).astype(dt)[:, None]
                    y[f] = -((xv - mean[f]) ** 2) / (dt(2) * sd[f] ** 2) - np.log(sd[f]) - dt(0.5 * np.log(2.0 * np.pi)) + lp[f]
                    y[f, m] = lp[f]
                else:
                    c = np.where(m, 0, x[:, v]).astype(np.int64)
                    y[f] = tab[f][:, c].T
                    y[f, m] = integ[f]
            vals.append(y)
            continue
        ch = chs[j] = resolve_fold_index(l.inputs, folds)
        cvs = [np.stack([vals[ch[f, h, 0]][ch[f, h, 1]] for h in range(l.arity)]) for f in range(F)]
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
            w = ws[j] = np.where(w > 0, w, 0).astype(dt)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                lw = np.log(w)
                for f in range(F):
                    y[f] = _lse(_entries(l, cvs[f])[:, None, :] + lw[f][None], 2)
        vals.append(y)
    root = resolve_fold_index(plan.output, folds).reshape(-1, 2)[0]
    logev = vals[root[0]][root[1], :, 0].copy()
    live = np.isfinite(logev)
    flows = [np.zeros((F, B, l.num_output_units), dtype=dt) for F, l in zip(folds, plan.layers)]
    flows[root[0]][root[1], :, 0] = 1
    edge, leaf, unit = {}, {}, [None] * len(plan.layers)
    for j in range(len(plan.layers) - 1, -1, -1):  # downward, flows and their sums over the live rows
        l, p = plan.layers[j], params[j]
        Ki, F, K = l.num_input_units, l.num_folds, l.num_output_units
        unit[j] = flows[j][:, live, :].sum(axis=1, dtype=dt)
        if l.inputs is None:
            if l.type == "gaussian":
                out = np.zeros((F, K, 3), dtype=dt)
                mean, sd = p["mean"].numpy().astype(dt), p["stddev"].numpy().astype(dt)
            else:
                out = np.zeros((F, K, tabs[j].shape[2]), dtype=dt)
            for f in range(F):
                v = int(l.scope_idx[f, 0])
                fk = flows[j][f]
                obs, mis = live & ~mask[:, v], live & mask[:, v]
                if l.type == "gaussian":
                    xv = x[obs, v].astype(dt)
                    fm = fk[mis].sum(axis=0, dtype=dt)
                    out[f, :, 0] = fk[obs].sum(axis=0, dtype=dt) + fm
                    out[f, :, 1] = (fk[obs] * xv[:, None]).sum(axis=0, dtype=dt) + fm * mean[f]
                    out[f, :, 2] = (fk[obs] * (xv * xv)[:, None]).sum(axis=0, dtype=dt) + fm * (sd[f] * sd[f] + mean[f] * mean[f])
                    continue
                t = tabs[j][f]
                mx = t.max(axis=1, keepdims=True)
                with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                    t = np.exp(t - np.where(np.isfinite(mx), mx, 0).astype(dt))
                    tot = t.sum(axis=1, keepdims=True)
                    nt = np.where(tot > 0, t / tot, 0).astype(dt)
                onehot = np.zeros((int(obs.sum()), nt.shape[1]), dtype=dt)
                onehot[np.arange(onehot.shape[0]), x[obs, v].astype(np.int64)] = 1
                out[f] = fk[obs].T @ onehot + fk[mis].sum(axis=0, dtype=dt)[:, None] * nt
            leaf[j] = out
            continue
        ch = chs[j]
        for f in range(F):
            fk = flows[j][f]
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
            e = _entries(l, np.stack([vals[ch[f, h, 0]][ch[f, h, 1]] for h in range(l.arity)]))  # (B, M)
            w = ws[j][f]
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                keep = (fk > 0) & np.isfinite(v)
                use = keep[:, :, None] & (w > 0)[None] & (e > -np.inf)[:, None, :]
                d = np.where(use, e[:, None, :] - np.where(keep, v, 0)[:, :, None], 0).astype(dt)
                term = np.where(use, np.where(keep, fk, 0)[:, :, None] * w[None] * np.exp(d), 0).astype(dt)  # (B, Ko, M)
            if j not in edge:
                edge[j] = np.zeros((F, K, w.shape[1]), dtype=dt)
            edge[j][f] = term[live].sum(axis=0, dtype=dt)
            fl = term.sum(axis=1, dtype=dt)
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
    return {"edge": edge, "leaf": leaf, "unit": unit, "logev": logev, "rows": int(live.sum()), "flows": flows, "vals": vals,
            "w": ws, "mask": mask}


def normalised_restated(plan: Plan, res: dict, pseudocount: float = 0.0) -> dict:
    """The closed-form M-step targets of `ExpectedStatistics.normalised`, for sum-type and Categorical layers."""
    out = {}
    for j, n in list(res["edge"].items()) + [(j, n) for j, n in res["leaf"].items() if plan.layers[j].type == "categorical"]:
        sup = res["w"][j] > 0 if j in res["edge"] else np.ones_like(n, dtype=bool)
        n = n + pseudocount * sup
        den = n.sum(axis=-1, keepdims=True)
        out[j] = np.where(den > 0, n / np.where(den > 0, den, 1), 0)
    return out
