"""A numpy restatement of decoding under soft evidence (`HipCircuit.soft_mpe`, `HipCircuit.sample_soft`,
cirkit_amd/csrc/ck_soft_decode.hip), for tests only.

The contracts of DESIGN.md section 11 ("Decoding under soft evidence") on the USER's plan, with parameters from the oracle
(`eval_param`), in fp64 -- or, with ``dtype=np.float32``, the yardstick of the GPU value tolerance: the same upward pass in
fp32.  Built from the soft-evidence, MPE and conditional-sampling restatements: their tables, entries, Philox counters and
`near` flags.

`soft_mpe_restated`.  Upward, max-product as `mpe_restated`, with one more kind of input: a unit k of a Categorical /
Binomial fold over the s-th soft variable is worth max_{c < C} (table[k, c] + log_lik[n, s, c]).  Downward, every unit on
the row's tree takes its argmax entry and a soft leaf its argmax state, the smallest index on ties; every other maximised
variable as `mpe_restated`.  `near`: a maximum on the row's tree wins by less than `tol`.

`sample_soft_restated`.  Upward, `soft_restated`'s values.  Downward, `sample_conditional_restated`'s draws over them; a soft
leaf on the tree draws c with mass exp(table[k, c] + log_lik[n, s, c]) from the uniform of word 0 of the node's Philox call
(n, global fold, 0, 0); every other unobserved variable from its own table row or Gaussian.  `near`: a uniform within `tol`
of an interior CDF boundary.

A NaN or +inf in a read entry of log_lik: the row's value is NaN and it takes nothing; a root value of -inf: nothing either.
Variables outside every input layer's scope read 0 in the rows that have a tree.
"""
from __future__ import annotations

import numpy as np

from cirkit_amd.plan import Plan, resolve_fold_index
from conditional_restatement import _is_mixing
from mpe_restatement import _entries, _gap, _gauss
from mpe_restatement import _log_table as _log_table64
from posterior_restatement import _log_table
from sampling_restatement import _probs_table, philox4x32_10, uniform
from soft_restatement import soft_restated


def _setup(plan: Plan, tensors, log_lik, x, soft_vars, dt):
    from oracle.torch_oracle import as_torch, eval_param

    tt = {k: (v.double() if not v.is_complex() else v) for k, v in as_torch(tensors).items()}
    D = plan.num_variables
    ll = np.asarray(log_lik, dtype=np.float64).astype(np.float32).astype(dt)  # (staged as fp32 on the device)
    B = ll.shape[0]
    soft = sorted(int(v) for v in soft_vars)
    assert len(soft) == ll.shape[1]
    spos = {v: i for i, v in enumerate(soft)}
    x = np.full((B, D), np.nan) if x is None else np.asarray(x, dtype=np.float64)[:, :D].copy()
    discrete = np.zeros(D, dtype=bool)
    covered = np.zeros(D, dtype=bool)
    for l in plan.layers:
        if l.inputs is None:
            covered[l.scope_idx[:, 0]] = True
            if l.type in ("categorical", "binomial"):
                discrete[l.scope_idx[:, 0]] = True
    mask = np.isnan(x) | ((x <= -1) & discrete)
    mask[:, soft] = True  # (entries of x at soft variables are ignored)
    folds = [l.num_folds for l in plan.layers]
    params = [{pn: eval_param(pg, tt) for pn, pg in l.params.items()} for l in plan.layers]
    tabs = {}
    for j, l in enumerate(plan.layers):
        if l.inputs is None and l.type != "gaussian":
            tabs[j] = _log_table64(l, params[j]) if dt is np.float64 else _log_table(l, params[j], dt)
    gauss = any(l.type == "gaussian" for l in plan.layers)
    return {"ll": ll, "x": x, "mask": mask, "spos": spos, "folds": folds, "params": params, "tabs": tabs, "gauss": gauss,
            "covered": covered, "B": B, "D": D, "off": np.concatenate([[0], np.cumsum(folds)]).astype(np.int64),
            "root": resolve_fold_index(plan.output, folds).reshape(-1, 2)[0]}


def _upward_max(plan: Plan, c: dict, dt):
    """(vals: one (F, B, K) array per layer, lws, chs, rowbad) of the max-product pass in `dt`."""
    ll, x, mask, spos, B = c["ll"], c["x"], c["mask"], c["spos"], c["B"]
    vals, lws, chs = [], {}, {}
    rowbad = np.zeros(B, dtype=bool)
    for j, l in enumerate(plan.layers):
        p = c["params"][j]
        F, K = l.num_folds, l.num_output_units
        y = np.empty((F, B, K), dtype=dt)
        if l.inputs is None:
            for f in range(F):
                v = int(l.scope_idx[f, 0])
                m = mask[:, v]
                if l.type == "gaussian":
                    mean, sd = p["mean"].numpy()[f].astype(dt), p["stddev"].numpy()[f].astype(dt)
                    lp = p["log_partition"].numpy()[f].astype(dt) if "log_partition" in p else None
                    y[f] = _gauss(np.where(m, 0.0, x[:, v]).astype(dt)[:, None], mean, sd, lp)
                    y[f, m] = _gauss(mean, mean, sd, lp)
                    continue
                tab = c["tabs"][j][f]  # (K, C)
                if v in spos:
                    lv = ll[:, spos[v], : tab.shape[1]]  # (B, C)
                    nan = (np.isnan(lv) | (lv == np.inf)).any(axis=1)
                    rowbad |= nan
                    with np.errstate(invalid="ignore"):
                        t = np.where(nan[:, None, None], dt(0), tab[None] + lv[:, None, :])  # (B, K, C)
                    y[f] = np.where(np.isnan(t), -np.inf, t).max(axis=2)
                else:
                    cat = np.where(m, 0, x[:, v]).astype(np.int64)
                    y[f] = tab[:, cat].T
                    y[f, m] = tab.max(axis=1)
            vals.append(y)
            continue
        ch = chs[j] = resolve_fold_index(l.inputs, c["folds"])
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
            with np.errstate(divide="ignore"):
                lw = lws[j] = np.where(w > 0, np.log(np.where(w > 0, w, 1.0)), -np.inf).astype(dt)  # (F, Ko, M)
            for f in range(F):
                y[f] = (_entries(l, cvs[f])[:, None, :] + lw[f][None]).max(axis=2)
        vals.append(y)
    return vals, lws, chs, rowbad


def _walk(plan: Plan, c: dict, vals, value, mode: str, tol: float, lws=None, seed: int = 0, row_ids=None):
    """The top-down walk of both queries over the upward values `vals`, rows with a finite `value` only.  mode "max": argmax
    entries over the log weights `lws`; mode "draw": draws over the linear weights.  Returns (out, choices, near)."""
    ll, x, mask, spos, B, D = c["ll"].astype(np.float64), c["x"], c["mask"], c["spos"], c["B"], c["D"]
    folds, off = c["folds"], c["off"]
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    n = np.arange(B, dtype=np.uint64) if row_ids is None else np.asarray(row_ids, dtype=np.uint64)
    vals = [v.astype(np.float64) for v in vals]
    sel = [np.full((F, B), -1, dtype=np.int64) for F in folds]
    root = c["root"]
    sel[root[0]][root[1], np.isfinite(value)] = 0
    out = np.where(mask, np.nan if c["gauss"] else -1.0, x)
    near = np.zeros(B, dtype=bool)
    choices: dict[int, np.ndarray] = {}

    def draw(rows: np.ndarray, u: np.ndarray, on: np.ndarray) -> np.ndarray:
        cdf = np.cumsum(rows, axis=1)
        T = cdf[:, -1:]
        t = u[:, None] * T
        i = np.argmax(t < cdf, axis=1)
        r = np.arange(len(i))
        lo = np.where(i > 0, cdf[r, np.maximum(i - 1, 0)] / T[:, 0], -1.0)
        hi = np.where(cdf[r, i] < T[:, 0], cdf[r, i] / T[:, 0], 2.0)
        near[on] |= (np.abs(u - lo) < tol) | (np.abs(u - hi) < tol)
        return i

    for j in range(len(plan.layers) - 1, -1, -1):
        l, p = plan.layers[j], c["params"][j]
        ch = None if l.inputs is None else resolve_fold_index(l.inputs, folds)
        if l.type in ("sum", "cpt", "tucker"):
            choices[j] = np.full((l.num_folds, B), -1, dtype=np.int64)
        for f in range(l.num_folds):
            k = sel[j][f]
            on = np.nonzero(k >= 0)[0]
            if l.inputs is None:
                on = on[mask[on, int(l.scope_idx[f, 0])]]  # (observed variables keep their value)
            if on.size == 0:
                continue
            k = k[on]
            g = int(off[j] + f)
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
            ph = philox4x32_10(n[on], g, 0, 0, k0, k1) if mode == "draw" else None
            if l.inputs is None:
                v = int(l.scope_idx[f, 0])
                if l.type == "gaussian":
                    mean, sd = p["mean"].numpy()[f], p["stddev"].numpy()[f]
                    if mode == "max":
                        out[on, v] = mean[k]
                    else:
                        u1 = ((ph[0].astype(np.uint64) >> np.uint64(8)) + 1).astype(np.float64) * 2.0**-24
                        z = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * uniform(ph[1]))
                        out[on, v] = mean[k] + sd[k] * z
                    continue
                t = c["tabs"][j][f][k].astype(np.float64)  # (n_on, C)
                if v in spos:
                    with np.errstate(invalid="ignore"):
                        t = t + ll[on, spos[v], : t.shape[1]]
                    t = np.where(np.isnan(t), -np.inf, t)
                if mode == "max":
                    out[on, v] = np.argmax(t, axis=1)
                    near[on] |= _gap(t) < tol
                elif v in spos:
                    with np.errstate(invalid="ignore", over="ignore"):
                        rows = np.exp(t - t.max(axis=1, keepdims=True))
                    out[on, v] = draw(rows, uniform(ph[0]), on)
                else:
                    out[on, v] = draw(_probs_table(l, p)[f][k], uniform(ph[0]), on)
                continue
            Ki = l.num_input_units
            cv = np.stack([vals[ch[f, h, 0]][ch[f, h, 1]][on] for h in range(l.arity)])  # (H, n_on, Ki)
            ent = _entries(l, cv)  # (n_on, M)
            if mode == "max":
                t = lws[j][f][k].astype(np.float64) + ent
                i = np.argmax(t, axis=1)
                near[on] |= _gap(t) < tol
            else:
                wr = p["weight"].numpy()[f][k]  # (n_on, M)
                pos = (wr > 0) & ~np.isnan(ent)
                emax = np.where(pos, ent, -np.inf).max(axis=1)
                ok = np.isfinite(emax)
                with np.errstate(invalid="ignore", over="ignore"):
                    rows = np.where(pos, wr * np.exp(ent - emax[:, None]), 0.0)
                on, k, rows, u = on[ok], k[ok], rows[ok], uniform(ph[0])[ok]
                if on.size == 0:
                    continue
                i = draw(rows, u, on)
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
    fill = mask & ~c["covered"][None, :] & np.isfinite(value)[:, None]  # (variables outside every input layer's scope: 0)
    out[fill] = 0.0
    return out, [choices[j] for j in sorted(choices)], near


def soft_mpe_restated(plan: Plan, tensors, log_lik, x, soft_vars, *, tol: float = 1e-4, dtype=np.float64):
    """(out (B, D) float64, choices [(F, B) int per sum-type layer], log value (B,) in `dtype`, near (B,) bool).  `log_lik`
    (B, S, C); `x` (B, D) or None; `soft_vars` the soft variable ids.  Entries that are not filled hold the sentinel: NaN
    for a circuit with a Gaussian layer, -1 otherwise."""
    dt = np.dtype(dtype).type
    c = _setup(plan, tensors, log_lik, x, soft_vars, dt)
    vals, lws, _, rowbad = _upward_max(plan, c, dt)
    logv = vals[c["root"][0]][c["root"][1], :, 0].copy()
    logv[rowbad] = np.nan
    out, choices, near = _walk(plan, c, vals, logv, "max", tol, lws=lws)
    return out, choices, logv, near


def sample_soft_restated(plan: Plan, tensors, log_lik, x, soft_vars, seed: int, *, tol: float = 1e-5, row_ids=None,
                         dtype=np.float64):
    """(out (B, D) float64, choices, near (B,) bool, log evidence (B,) in `dtype`).  `row_ids`: the rows' indices in the
    batch the device drew (the Philox counter), by default 0 .. B - 1."""
    dt = np.dtype(dtype).type
    c = _setup(plan, tensors, log_lik, x, soft_vars, dt)
    xs = np.where(c["mask"], np.nan, c["x"])
    up = soft_restated(plan, tensors, log_lik, xs, sorted(c["spos"]), dtype=dtype)
    logev = up["logev"]
    out, choices, near = _walk(plan, c, up["vals"], logev, "draw", tol, seed=seed, row_ids=row_ids)
    return out, choices, near, logev


def completion_value(plan: Plan, tensors, log_lik, out, soft_vars) -> np.ndarray:
    """(B,) the max-product value of the full assignment `out` plus the log weights of its soft states:
    what `soft_mpe`'s value must equal when its completion is evaluated again."""
    from mpe_restatement import mpe_restated

    soft = sorted(int(v) for v in soft_vars)
    ll = np.asarray(log_lik, dtype=np.float64).astype(np.float32).astype(np.float64)
    _, _, lv, _ = mpe_restated(plan, tensors, out, np.zeros(plan.num_variables, dtype=bool))
    B = out.shape[0]
    for s, v in enumerate(soft):
        lv = lv + ll[np.arange(B), s, out[:, v].astype(np.int64)]
    return lv
