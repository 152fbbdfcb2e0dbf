"""A numpy restatement of marginal MAP (`HipCircuit.marginal_map`, cirkit_amd/csrc/ck_mmap.hip), for tests only.

The contract of DESIGN.md section 11 ("Marginal MAP") in fp64 on the USER's plan, with parameters from the oracle
(`eval_param`).  One query set Q per call.  A variable of Q is maximised in every row; any other variable is evidence where
`x` holds a value and summed out where it holds the sentinel (NaN; a value <= -1 of a variable read by a discrete layer).
Upward: a fold of a sum / mixing / CP-T / Tucker layer whose scope is disjoint from Q takes log sum_i w_i exp(v_i) over the
entries with w_i > 0, a fold whose scope meets Q takes max_i (log w_i + v_i); Hadamard and Kronecker units add their
children; an input unit gives log p(x_v) where observed, max_c log p(c) where maximised (a Gaussian: its log density at the
mean) and its log integral where summed out: 0 for `probs` and for a Binomial, the logsumexp of `logits`, a Gaussian's
`log_partition` or 0 -- what the oracle's marginal forward gives an integrated unit.  Downward from output fold 0, unit 0:
a max fold on the row's tree takes its argmax entry (smallest index on ties, numpy's argmax), a sum fold ends the walk, an
input unit writes its argmax category (or the Gaussian mean) only for a variable of Q.  `log_prob` is the same upward pass,
all folds summing, on the returned rows.
"""
from __future__ import annotations

import numpy as np

from cirkit_amd.plan import Plan, resolve_fold_index
from mpe_restatement import _entries, _gap, _gauss, _is_mixing, _log_table


def _lse(t: np.ndarray) -> np.ndarray:
    """logsumexp over the last axis; -inf where every term is -inf."""
    m = t.max(axis=-1)
    safe = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return safe + np.log(np.exp(t - safe[..., None]).sum(axis=-1)) + np.where(np.isfinite(m), 0.0, m)


def _integral(l, p, f) -> np.ndarray:
    """(K,) log integral of the units of fold f of an input layer."""
    K = l.num_output_units
    if l.type == "gaussian":
        return p["log_partition"].numpy()[f] if "log_partition" in p else np.zeros(K)
    if l.type == "categorical" and "logits" in p:
        return _lse(p["logits"].numpy()[f])
    return np.zeros(K)


def _upward(plan, params, tabs, chs, lws, x, maximised, missing, maxf):
    """Per layer the (F, B, K) values; `maximised`, `missing` (B, D) the roles of the entries, `maxf[j]` (F,) the max folds."""
    B = x.shape[0]
    vals: list[np.ndarray] = []
    for j, l in enumerate(plan.layers):
        p = params[j]
        F, K = l.num_folds, l.num_output_units
        y = np.empty((F, B, K))
        if l.inputs is None:
            for f in range(F):
                v = int(l.scope_idx[f, 0])
                mx, ms = maximised[:, v], missing[:, v]
                hid = mx | ms
                if l.type == "gaussian":
                    mean, sd = p["mean"].numpy()[f], p["stddev"].numpy()[f]
                    lp = p["log_partition"].numpy()[f] if "log_partition" in p else None
                    y[f] = _gauss(np.where(hid, 0.0, x[:, v])[:, None], mean, sd, lp)
                    y[f, mx] = _gauss(mean, mean, sd, lp)
                else:
                    tab = tabs[j]
                    y[f] = tab[f][:, np.where(hid, 0, x[:, v]).astype(np.int64)].T
                    y[f, mx] = tab[f].max(axis=1)
                y[f, ms] = _integral(l, p, f)
            vals.append(y)
            continue
        ch = chs[j]
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
            for f in range(F):
                t = _entries(l, cvs[f])[:, None, :] + lws[j][f][None]  # (B, Ko, M): log w_i + v_i, -inf where w_i <= 0
                y[f] = t.max(axis=2) if maxf[j][f] else _lse(t)
        vals.append(y)
    return vals


def mmap_restated(plan: Plan, tensors, x, query_mask, tol: float = 1e-4, *, leaf_tol: float | None = None):
    """(out (B, D) float64, choices [(F, B) int per sum / mixing / CP-T / Tucker layer], log_value (B,), log_prob (B,), near
    (B,) bool).  `query_mask` (D,) bool.  Query entries of rows without finite mass, and summed-out entries, hold the
    sentinel: NaN for a circuit with a Gaussian layer, -1 otherwise.  `near`: the rows on whose tree some max fold has its
    best two entries within `tol`, or some input unit over a query variable its best two categories within `leaf_tol`
    (default `tol`) without being equal.  The two differ because an entry of a max fold carries the rounding of a whole
    sub-circuit, a table entry only its own."""
    from oracle.torch_oracle import as_torch, eval_param

    tt = {k: (v.double() if not v.is_complex() else v) for k, v in as_torch(tensors).items()}
    D = plan.num_variables
    x = np.asarray(x, dtype=np.float64)
    B = x.shape[0]
    q = np.asarray(query_mask, dtype=bool).reshape(D)
    leaf_tol = tol if leaf_tol is None else leaf_tol
    gauss = any(l.type == "gaussian" for l in plan.layers)
    sentinel = np.nan if gauss else -1.0
    discrete = np.zeros(D, dtype=bool)
    for l in plan.layers:
        if l.type in ("categorical", "binomial"):
            discrete[l.scope_idx[:, 0]] = True
    maximised = np.broadcast_to(q, (B, D))
    missing = (np.isnan(x) | ((x <= -1) & discrete)) & ~maximised
    folds = [l.num_folds for l in plan.layers]
    params = [{pn: eval_param(pg, tt) for pn, pg in l.params.items()} for l in plan.layers]
    tabs, lws, chs, maxf = {}, {}, {}, []
    for j, l in enumerate(plan.layers):
        if l.inputs is None:
            if l.type != "gaussian":
                tabs[j] = _log_table(l, params[j])
            maxf.append(q[l.scope_idx[:, 0]])
            continue
        ch = chs[j] = resolve_fold_index(l.inputs, folds)
        maxf.append(np.array([any(maxf[ch[f, h, 0]][ch[f, h, 1]] for h in range(l.arity)) for f in range(l.num_folds)]))
        if l.type in ("sum", "cpt", "tucker"):
            w = params[j]["weight"].numpy()
            with np.errstate(divide="ignore"):
                lws[j] = np.where(w > 0, np.log(np.where(w > 0, w, 1.0)), -np.inf)
    vals = _upward(plan, params, tabs, chs, lws, x, maximised, missing, maxf)
    root = resolve_fold_index(plan.output, folds).reshape(-1, 2)[0]
    logv = vals[root[0]][root[1], :, 0].copy()
    sel = [np.full((F, B), -1, dtype=np.int64) for F in folds]
    sel[root[0]][root[1], np.isfinite(logv)] = 0
    out = np.where(maximised | missing, sentinel, x)
    near = np.zeros(B, dtype=bool)
    choices: dict[int, np.ndarray] = {}
    for j in range(len(plan.layers) - 1, -1, -1):  # downward: argmax at the max folds, nothing below a sum fold
        l, p = plan.layers[j], params[j]
        if l.type in ("sum", "cpt", "tucker"):
            choices[j] = np.full((l.num_folds, B), -1, dtype=np.int64)
        for f in range(l.num_folds):
            on = np.nonzero(sel[j][f] >= 0)[0]
            if on.size == 0 or not maxf[j][f]:
                continue
            k = sel[j][f][on]
            if l.inputs is None:
                v = int(l.scope_idx[f, 0])  # (a max fold of an input layer: its variable is in Q)
                if l.type == "gaussian":
                    out[on, v] = p["mean"].numpy()[f][k]
                else:
                    t = tabs[j][f][k]
                    out[on, v] = np.argmax(t, axis=1)
                    g = _gap(t)  # (equal table entries are equal numbers on the device too: the smallest index, no near tie)
                    near[on] |= (g < leaf_tol) & (g > 0)
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
            t = lws[j][f][k] + _entries(l, cv)
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
    out[maximised & ~covered[None, :] & np.isfinite(logv)[:, None]] = 0.0  # (query variables no input layer reads: 0)
    # log c(q*, x_E): every fold summing, on the returned rows (the query entries of a row without mass stay hidden: -inf)
    none = np.zeros((B, D), dtype=bool)
    hidden = np.isnan(out) | ((out <= -1) & discrete)
    sums = [np.zeros(F, dtype=bool) for F in folds]
    lp_vals = _upward(plan, params, tabs, chs, lws, out, none, hidden, sums)
    logp = np.where(np.isfinite(logv), lp_vals[root[0]][root[1], :, 0], logv)
    return out, [choices[j] for j in sorted(choices)], logv, logp, near
