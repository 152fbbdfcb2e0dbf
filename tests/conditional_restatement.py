"""A numpy restatement of conditional sampling (`HipCircuit.sample_conditional`, cirkit_amd/csrc/ck_sample_cond.hip), for
tests only.

The contract of DESIGN.md section 11 ("Conditional sampling") in fp64 on the USER's plan: the per-row value of every unit
under the row's evidence from the oracle's forward with the row's integration mask; a row whose root value is not finite
draws nothing; a sum-type unit draws entry i with mass w_i exp(v_i) (v_i: the entry's child value at the row, CP-T summed
over the inputs, Tucker v0[a] + v1[b]; entries with w_i <= 0 have no mass); an input unit draws only an unobserved
variable, from its own table row.  Philox4x32-10 counters (n, global fold id, 0, 0) and the uniform of
tests/sampling_restatement.py; `near` as `sample_restated` flags it.
"""
from __future__ import annotations

import numpy as np
import torch

from cirkit_amd.plan import Plan, resolve_fold_index
from sampling_restatement import _probs_table, philox4x32_10, uniform


def _is_mixing(l) -> bool:
    g = l.params["weight"]
    return l.type == "sum" and len(g.output.ids) == 1 and g.nodes[g.output.ids[0]].op == "mixing_weight"


def sample_conditional_restated(plan: Plan, tensors, x, mask, seed: int, *, tol: float = 1e-5, row_ids=None):
    """(out (B, D) float64, choices [(F, B) int per sum / mixing / CP-T / Tucker layer], near (B,) bool, log evidence (B,)).

    `x` (B, D) the evidence, `mask` a bool (B, D) / (1, D) / (D,) array of the variables to draw; entries of `x` holding the
    sentinel (NaN; a value <= -1 of a variable read by a discrete layer) are drawn too.  Sampled entries that are not drawn
    (rows without mass) hold the sentinel: NaN for a circuit with a Gaussian layer, -1 otherwise.  `row_ids`: the rows' indices
    n in the batch the device drew (the Philox counter), by default 0 .. B - 1."""
    from oracle.torch_oracle import as_torch, eval_param, evaluate_plan

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
    xin = np.where(mask, 0.0, x)
    xin = torch.from_numpy(xin) if gauss else torch.from_numpy(xin.astype(np.int64))
    _, outs = evaluate_plan(plan, tt, xin, return_all=True, integrate_mask=torch.from_numpy(mask.copy()))
    vals = [o.numpy() for o in outs]  # (F, B, K) per-row log values under the evidence
    folds = [l.num_folds for l in plan.layers]
    off = np.concatenate([[0], np.cumsum(folds)]).astype(np.int64)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    n = np.arange(B, dtype=np.uint64) if row_ids is None else np.asarray(row_ids, dtype=np.uint64)
    sel = [np.full((F, B), -1, dtype=np.int64) for F in folds]
    root = resolve_fold_index(plan.output, folds).reshape(-1, 2)[0]
    logev = vals[root[0]][root[1], :, 0].copy()
    sel[root[0]][root[1], np.isfinite(logev)] = 0
    out = np.where(mask, np.nan if gauss else -1.0, x)
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
        l = plan.layers[j]
        params = {pn: eval_param(pg, tt) for pn, pg in l.params.items()}
        ch = None if l.inputs is None else resolve_fold_index(l.inputs, folds)
        if l.type in ("sum", "cpt", "tucker"):
            choices[j] = np.full((l.num_folds, B), -1, dtype=np.int64)
            w = params["weight"].numpy()
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
            p = philox4x32_10(n[on], g, 0, 0, k0, k1)
            if l.type == "gaussian":
                u1 = ((p[0].astype(np.uint64) >> np.uint64(8)) + 1).astype(np.float64) * 2.0**-24
                u2 = uniform(p[1])
                z = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
                mean, sd = params["mean"].numpy()[f], params["stddev"].numpy()[f]
                out[on, int(l.scope_idx[f, 0])] = mean[k] + sd[k] * z
                continue
            u = uniform(p[0])
            if l.type in ("categorical", "binomial"):
                out[on, int(l.scope_idx[f, 0])] = draw(_probs_table(l, params)[f][k], u, on)
                continue
            Ki = l.num_input_units
            cv = np.stack([vals[ch[f, h, 0]][ch[f, h, 1]][on] for h in range(l.arity)])  # (H, n_on, Ki)
            if l.type == "cpt":
                ent = cv.sum(0)
            elif l.type == "tucker":
                ent = (cv[0][:, :, None] + cv[1][:, None, :]).reshape(on.size, -1)
            else:
                ent = cv.transpose(1, 0, 2).reshape(on.size, -1)
            wr = w[f][k]  # (n_on, M)
            pos = (wr > 0) & ~np.isnan(ent)
            emax = np.where(pos, ent, -np.inf).max(axis=1)
            ok = np.isfinite(emax)
            with np.errstate(invalid="ignore", over="ignore"):
                rows = np.where(pos, wr * np.exp(ent - emax[:, None]), 0.0)
            on, k, rows, u = on[ok], k[ok], rows[ok], u[ok]
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
    return out, [choices[j] for j in sorted(choices)], near, logev
