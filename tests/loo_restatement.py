"""A numpy restatement of the leave-one-out conditionals (`HipCircuit.leave_one_out`, `HipCircuit.conditional_log_probs`,
cirkit_amd/csrc/ck_loo.hip), for tests only.

The contract of DESIGN.md section 11 ("Leave-one-out conditionals") on the USER's plan, with parameters from the oracle
(`eval_param`), in fp64 -- or, with ``dtype=np.float32``, the same formulas in fp32: the yardstick of the GPU tolerances.
Upward: the marginal forward in log space, as tests/posterior_restatement.py.  Downward, LOG space: D(u) = log dc(x_O)/du,
0 at the root unit, -inf elsewhere until written.  Per sum-type fold m = max_k D_k over the finite D_k,
T_i = sum_k w[k, i] exp(D_k - m), base_i = m + log T_i (-inf where T_i = 0); sum / mixing entry i goes to input i // Ki unit
i % Ki as it is, CP-T entry i to every input h with the values of the inputs h' != h at unit i added in input order, Tucker
(a, b) as lse_b(base + v_1[b]) to input 0 and lse_a(base + v_0[a]) to input 1; Hadamard hands D_k plus the siblings' values
at unit k, Kronecker the log-sum-exp over the outputs that share the digit.  A fold combines its messages with logaddexp,
layers last to first, folds and input positions ascending.  Leaves, over the input units k of a variable in all its folds,
with d_k = D_k - max_k D_k and log Z_k = log sum_c t_k[c]: p[c] = a_c / sum_c a_c, a_c = sum_k exp(d_k + log Z_k - shift)
nt_k[c] (nt the table row over its own sum); Gaussian moments under pi = softmax_k(D_k); log p(x_v | rest) = lse_k(d_k + v_k)
- lse_k(d_k + log Z_k).
"""
from __future__ import annotations

import numpy as np

from cirkit_amd.plan import Plan, resolve_fold_index
from mpe_restatement import _entries
from posterior_restatement import _log_table, _lse


def forward_restated(plan: Plan, tensors, x, mask, dt):
    """The marginal forward of tests/posterior_restatement.py: (per-layer (F, B, K) log values, evaluated parameters, log
    tables of the discrete input layers, clamped sum weights, resolved child folds)."""
    from oracle.torch_oracle import as_torch, eval_param

    tt = {k: (v.double() if not v.is_complex() else v) for k, v in as_torch(tensors).items()}
    B = x.shape[0]
    folds = [l.num_folds for l in plan.layers]
    params = [{pn: eval_param(pg, tt) for pn, pg in l.params.items()} for l in plan.layers]
    tabs, ws, chs, vals = {}, {}, {}, []
    for j, l in enumerate(plan.layers):
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
    return vals, params, tabs, ws, chs


def _max_finite(a: np.ndarray, axis: int):
    """(max over the finite entries, kept as a dimension; 0 where there is none, and whether there is one)."""
    fin = np.isfinite(a)
    m = np.where(fin, a, -np.inf).max(axis=axis, keepdims=True)
    has = np.isfinite(m)
    return np.where(has, m, 0).astype(a.dtype), has, fin


def derivatives_restated(plan: Plan, vals, ws, chs, dt) -> list[np.ndarray]:
    """Per layer the (F, B, K) log derivatives D of the root unit's value with respect to every unit's value."""
    folds = [l.num_folds for l in plan.layers]
    B = vals[0].shape[1]
    ninf = dt(-np.inf)
    Ds = [np.full((F, B, l.num_output_units), ninf, dtype=dt) for F, l in zip(folds, plan.layers)]
    root = resolve_fold_index(plan.output, folds).reshape(-1, 2)[0]
    Ds[root[0]][root[1], :, 0] = 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for j in range(len(plan.layers) - 1, -1, -1):
            l = plan.layers[j]
            if l.inputs is None:
                continue
            Ki, H, ch = l.num_input_units, l.arity, chs[j]
            for f in range(l.num_folds):
                Dk = Ds[j][f]
                cv = [vals[ch[f, h, 0]][ch[f, h, 1]] for h in range(H)]

                def send(h, msg):
                    kid = Ds[ch[f, h, 0]]
                    kid[ch[f, h, 1]] = np.logaddexp(kid[ch[f, h, 1]], msg.astype(dt))

                if l.type == "hadamard":
                    for h in range(H):
                        acc = Dk
                        for h2 in range(H):
                            if h2 != h:
                                acc = acc + cv[h2]
                        send(h, acc)
                    continue
                if l.type == "kronecker":
                    cube = Dk.reshape((B,) + (Ki,) * H)
                    for h in range(H):
                        t = cube
                        for h2 in range(H - 1, -1, -1):
                            if h2 != h:
                                t = t + cv[h2].reshape((B,) + tuple(Ki if a == h2 else 1 for a in range(H)))
                        send(h, _lse(np.moveaxis(t, h + 1, 1).reshape(B, Ki, -1), 2))
                    continue
                m, _, fin = _max_finite(Dk, 1)
                a = np.where(fin, np.exp(np.where(fin, Dk, 0) - m), 0).astype(dt)
                T = (a @ ws[j][f]).astype(dt)  # (B, M)
                base = np.where(T > 0, m + np.log(np.where(T > 0, T, 1)), ninf).astype(dt)
                if l.type == "sum":
                    for h in range(H):
                        send(h, base[:, h * Ki : (h + 1) * Ki])
                elif l.type == "cpt":
                    for h in range(H):
                        acc = base
                        for h2 in range(H):
                            if h2 != h:
                                acc = acc + cv[h2]
                        send(h, acc)
                else:  # tucker, arity 2
                    sq = base.reshape(B, Ki, Ki)
                    send(0, _lse(sq + cv[1][:, None, :], 2))
                    send(1, _lse(sq + cv[0][:, :, None], 1))
    return Ds


def leave_one_out_restated(plan: Plan, tensors, x, query=None, missing=None, *, dtype=np.float64) -> dict:
    """``p`` (B, Q, C) -- (B, Q, 2) mean and variance for Gaussian query variables --, ``logp`` (B, D), ``logev`` (B,),
    ``cons`` (B, D) = lse_k(D_k + v_k) (NaN for an uncovered variable), ``zero_share`` (B, D) the share of the leave-one-out
    mass carried by input units whose value is -inf, ``D`` and ``vals`` (one (F, B, K) array per layer), ``mask`` (B, D)
    what was integrated out, and ``units`` per covered variable (D, v, log Z, normalised table rows) over its input units.

    `x` (B, D) the evidence, `query` the query variable ids (None: every covered variable, those of the first kind met if
    the circuit mixes kinds), `missing` ids or a bool mask (D,) / (B, D); entries of `x` holding the sentinel (NaN; a value
    <= -1 of a variable read by a discrete layer) are integrated out too."""
    dt = np.dtype(dtype).type
    D = plan.num_variables
    x = np.asarray(x, dtype=np.float64)
    B = x.shape[0]
    discrete = np.zeros(D, dtype=bool)
    for l in plan.layers:
        if l.type in ("categorical", "binomial"):
            discrete[l.scope_idx[:, 0]] = True
    mask = np.zeros((B, D), dtype=bool)
    if missing is not None:
        missing = np.asarray(missing)
        if missing.dtype == bool:
            mask |= np.broadcast_to(missing.reshape(-1, D), (B, D))
        else:
            mask[:, missing.astype(np.int64)] = True
    mask |= np.isnan(x) | ((x <= -1) & discrete)
    vals, params, tabs, ws, chs = forward_restated(plan, tensors, x, mask, dt)
    folds = [l.num_folds for l in plan.layers]
    root = resolve_fold_index(plan.output, folds).reshape(-1, 2)[0]
    logev = vals[root[0]][root[1], :, 0].copy()
    Ds = derivatives_restated(plan, vals, ws, chs, dt)
    ninf = dt(-np.inf)
    var_folds: dict[int, list] = {}
    for j, l in enumerate(plan.layers):
        if l.inputs is None:
            for f, v in enumerate(l.scope_idx[:, 0]):
                var_folds.setdefault(int(v), []).append((j, f))
    is_gauss = {v: plan.layers[fl[0][0]].type == "gaussian" for v, fl in var_folds.items()}
    if query is None:
        first = is_gauss[min(var_folds)]
        query = [v for v in sorted(var_folds) if is_gauss[v] == first]
    query = sorted(int(v) for v in query)
    gauss_q = bool(query) and all(is_gauss[v] for v in query)
    C = 2 if gauss_q else max(tabs[j].shape[2] for v in query for j, _ in var_folds[v])
    p = np.zeros((B, len(query), C), dtype=dt)
    logp = np.zeros((B, D), dtype=dt)
    cons = np.full((B, D), np.nan, dtype=dt)
    share = np.zeros((B, D), dtype=dt)
    units = {}
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for v, fl in var_folds.items():
            Dc = np.concatenate([Ds[j][f] for j, f in fl], axis=1)  # (B, Ktot)
            vc = np.concatenate([vals[j][f] for j, f in fl], axis=1)
            if is_gauss[v]:
                lz = np.zeros(Dc.shape[1], dtype=dt)
                nt = None
                mean = np.concatenate([params[j]["mean"].numpy().astype(dt)[f] for j, f in fl])
                sd = np.concatenate([params[j]["stddev"].numpy().astype(dt)[f] for j, f in fl])
            else:
                Cv = max(tabs[j].shape[2] for j, _ in fl)
                lzs, nts = [], []
                for j, f in fl:
                    t = tabs[j][f]  # (K, C) log table
                    mx = t.max(axis=1, keepdims=True)
                    mx0 = np.where(np.isfinite(mx), mx, 0).astype(dt)
                    e = np.exp(t - mx0)
                    tot = e.sum(axis=1, keepdims=True)
                    lzs.append(np.where(tot > 0, np.log(np.where(tot > 0, tot, 1)) + mx0, ninf)[:, 0].astype(dt))
                    n = np.zeros((t.shape[0], Cv), dtype=dt)
                    n[:, : t.shape[1]] = np.where(tot > 0, e / np.where(tot > 0, tot, 1), 0)
                    nts.append(n)
                lz, nt = np.concatenate(lzs), np.concatenate(nts)
            units[v] = (Dc, vc, lz, nt)
            mD, has, fin = _max_finite(Dc, 1)
            d = np.where(fin, np.where(fin, Dc, 0) - mD, ninf).astype(dt)
            cons[:, v] = _lse((Dc + vc).astype(dt), 1)
            num, den = _lse((d + vc).astype(dt), 1), _lse((d + lz[None]).astype(dt), 1)
            lp = np.where(np.isfinite(den), num - np.where(np.isfinite(den), den, 0), np.nan)
            logp[:, v] = np.where(mask[:, v], 0, lp)
            t = (d + lz[None]).astype(dt)
            m2, _, fin2 = _max_finite(t, 1)
            pi = np.where(fin2, np.exp(np.where(fin2, t, 0) - m2), 0).astype(dt)
            tot = pi.sum(1)
            share[:, v] = np.where(tot > 0, (pi * (vc == -np.inf)).sum(1) / np.where(tot > 0, tot, 1), 0)
            if v not in query:
                continue
            q = query.index(v)
            if is_gauss[v]:
                w = np.where(fin, np.exp(d), 0).astype(dt)
                s0 = w.sum(1)
                m1 = (w @ mean) / s0
                p[:, q, 0] = m1
                p[:, q, 1] = (w @ (sd * sd + mean * mean)) / s0 - m1 * m1
            else:
                a = (pi @ nt).astype(dt)  # (B, Cv)
                tot = a.sum(1, keepdims=True)
                p[:, q, : a.shape[1]] = np.where(tot > 0, a / np.where(tot > 0, tot, 1), np.nan)
    return {"p": p, "logp": logp, "logev": logev, "cons": cons, "zero_share": share, "D": Ds, "vals": vals, "mask": mask,
            "units": units, "query": query}
