"""A numpy restatement of the posterior marginals (`HipCircuit.posterior_marginals`, cirkit_amd/csrc/ck_flow.hip), for
tests only.

The contract of DESIGN.md section 11 ("Posterior marginals") on the USER's plan, with parameters from the oracle
(`eval_param`), in fp64 -- or, with ``dtype=np.float32``, the same formulas in fp32: the yardstick of the GPU tolerances.
Upward: the marginal forward in log space (an integrated input unit gives its layer's integral).  Downward, linear space,
f(root) = 1: per sum-type fold lg_k = log f_k - v_k over the units with f_k > 0 and finite v_k, m = max_k lg_k,
T_i = sum_k w[k, i] exp(lg_k - m), entry i receives exp(m + e_i + log T_i) (0 where T_i = 0); sum / mixing entries go to
input i // Ki unit i % Ki, CP-T entries to every input, Tucker (a, b) summed over b to input 0 and over a to input 1;
Hadamard hands f_k to every input's unit k, Kronecker the digit sums.  A Categorical / Binomial unit over a query variable
adds f_k t_k[c] / sum_c' t_k[c'], a Gaussian one f_k, f_k mean_k, f_k (stddev_k^2 + mean_k^2).  Nothing is renormalised.
"""
from __future__ import annotations

from math import lgamma

import numpy as np

from cirkit_amd.plan import Plan, resolve_fold_index
from mpe_restatement import _entries


def _log_table(l, params, dt) -> np.ndarray:
    """(F, K, C) log-probabilities of a Categorical / Binomial layer, evaluated in `dt` from the `dt` parameters."""
    if l.type == "categorical":
        if "probs" in params:
            with np.errstate(divide="ignore"):
                return np.log(params["probs"].numpy().astype(dt))
        return params["logits"].numpy().astype(dt)
    T = int(l.config["total_count"])
    # the reference's expression (torch.distributions.Binomial.log_prob, input.py:530-541; the device's table evaluates the
    # same one in fp32, ck_param.hip), every term and every step in `dt`:
    #   c l - lgamma(c + 1) - lgamma(T - c + 1) - (T max(l, 0) + T log1p(exp(-|l|)) - lgamma(T + 1)),  l the logit
    with np.errstate(divide="ignore", invalid="ignore"):
        if "probs" in params:
            p = params["probs"].numpy().astype(dt)
            lg = (np.log(p) - np.log1p(-p)).astype(dt)[..., None]
        else:
            lg = params["logits"].numpy().astype(dt)[..., None]
        c = np.arange(T + 1).astype(dt)
        lgam = lambda a: np.array([lgamma(float(v)) for v in a]).astype(dt)  # noqa: E731
        norm = dt(T) * np.maximum(lg, dt(0)) + dt(T) * np.log1p(np.exp(-np.abs(lg))) - dt(lgamma(T + 1))
        lp = c * lg - lgam(c + 1) - lgam(dt(T) - c + 1) - norm
    return np.where(np.isnan(lp), -np.inf, lp).astype(dt)


def _lse(t: np.ndarray, axis: int) -> np.ndarray:
    m = t.max(axis=axis, keepdims=True)
    m0 = np.where(np.isfinite(m), m, 0).astype(t.dtype)
    with np.errstate(divide="ignore"):
        return (np.log(np.exp(t - m0).sum(axis=axis, keepdims=True)) + m0).squeeze(axis)


def posterior_restated(plan: Plan, tensors, x, query, *, dtype=np.float64) -> dict:
    """``p`` (B, Q, C) -- (B, Q, 2) mean and variance for Gaussian query variables --, ``logev`` (B,), ``flows`` (one
    (F, B, K) array per layer) and ``leaf_flow`` (B, Q), the flow reaching the input units of each query variable.

    `x` (B, D) the evidence, `query` the query variable ids; entries of `x` holding the sentinel (NaN; a value <= -1 of a
    variable read by a discrete layer) are integrated out.  Rows without a finite root value are NaN."""
    from oracle.torch_oracle import as_torch, eval_param

    dt = np.dtype(dtype).type
    tt = {k: (v.double() if not v.is_complex() else v) for k, v in as_torch(tensors).items()}
    D = plan.num_variables
    x = np.asarray(x, dtype=np.float64)
    B = x.shape[0]
    query = sorted(int(v) for v in query)
    qpos = {v: i for i, v in enumerate(query)}
    discrete = np.zeros(D, dtype=bool)
    for l in plan.layers:
        if l.type in ("categorical", "binomial"):
            discrete[l.scope_idx[:, 0]] = True
    mask = np.zeros((B, D), dtype=bool)
    mask[:, query] = True
    mask |= np.isnan(x) | ((x <= -1) & discrete)
    folds = [l.num_folds for l in plan.layers]
    params = [{pn: eval_param(pg, tt) for pn, pg in l.params.items()} for l in plan.layers]
    tabs: dict[int, np.ndarray] = {}
    ws: dict[int, np.ndarray] = {}
    chs: dict[int, np.ndarray] = {}
    vals: list[np.ndarray] = []
    for j, l in enumerate(plan.layers):  # upward, marginal forward
        p = params[j]
        F, K = l.num_folds, l.num_output_units
        y = np.empty((F, B, K), dtype=dt)
        if l.inputs is None:
            if l.type == "gaussian":
                mean, sd = p["mean"].numpy().astype(dt), p["stddev"].numpy().astype(dt)
                lp = p["log_partition"].numpy().astype(dt) if "log_partition" in p else np.zeros((F, K), dtype=dt)
            else:
                tab = tabs[j] = _log_table(l, p, dt)  # (F, K, C)
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
    root = resolve_fold_index(plan.output, folds).reshape(-1, 2)[0]
    logev = vals[root[0]][root[1], :, 0].copy()
    flows = [np.zeros((F, B, l.num_output_units), dtype=dt) for F, l in zip(folds, plan.layers)]
    flows[root[0]][root[1], :, 0] = 1
    gauss_q = [plan.layers[j].type == "gaussian" for j, l in enumerate(plan.layers) if l.inputs is None
               for v in l.scope_idx[:, 0] if int(v) in qpos]
    is_gauss = bool(gauss_q) and all(gauss_q)
    C = 2
    if not is_gauss:
        C = max(tabs[j].shape[2] for j, l in enumerate(plan.layers) if l.inputs is None and l.type != "gaussian"
                and any(int(v) in qpos for v in l.scope_idx[:, 0]))
    out = np.zeros((B, len(query), C), dtype=dt)
    s1 = np.zeros((B, len(query)), dtype=dt)
    s2 = np.zeros((B, len(query)), dtype=dt)
    leaf_flow = np.zeros((B, len(query)), dtype=dt)
    for j in range(len(plan.layers) - 1, -1, -1):  # downward, flows
        l, p = plan.layers[j], params[j]
        Ki = l.num_input_units
        for f in range(l.num_folds):
            fk = flows[j][f]
            if l.inputs is None:
                v = int(l.scope_idx[f, 0])
                if v not in qpos:
                    continue
                q = qpos[v]
                leaf_flow[:, q] += fk.sum(1)
                if l.type == "gaussian":
                    mean, sd = p["mean"].numpy().astype(dt)[f], p["stddev"].numpy().astype(dt)[f]
                    s1[:, q] += fk @ mean
                    s2[:, q] += fk @ (sd * sd + mean * mean)
                else:
                    t = tabs[j][f]
                    mx = t.max(axis=1, keepdims=True)
                    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                        t = np.exp(t - np.where(np.isfinite(mx), mx, 0).astype(dt))
                        tot = t.sum(axis=1, keepdims=True)
                        nt = np.where(tot > 0, t / tot, 0).astype(dt)
                    out[:, q, : nt.shape[1]] += fk @ nt
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
                fl = np.where(T > 0, np.exp(m + np.where(T > 0, e, 0) + np.log(np.where(T > 0, T, 1))), 0).astype(dt)
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
    if is_gauss:
        out = np.stack([s1, s2 - s1 * s1], axis=2)
    dead = ~np.isfinite(logev)
    out[dead] = np.nan
    return {"p": out, "logev": logev, "flows": flows, "leaf_flow": leaf_flow}
