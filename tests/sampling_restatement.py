"""A numpy restatement of the GPU sampler (cirkit_amd/sampling.py, cirkit_amd/csrc/ck_sample.hip), for tests only.

Same contract as DESIGN.md section 11, computed in fp64 on the USER's (unpadded) plan: the partition function of every unit
from the oracle's integrated forward, Philox4x32-10 with key (seed_lo, seed_hi) and counter (n, global fold id, 0, 0), the
uniform u = (x0 >> 8) 2^-24, the categorical draw = the smallest i with u T < CDF_i, Box-Muller on (x0, x1).  Padding a plan
inserts zero-mass entries without reordering the real ones, so the draws of the padded GPU plan are the same indices.
"""
from __future__ import annotations

import numpy as np
import torch

from cirkit_amd.plan import Plan, resolve_fold_index

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0: int, k1: int):
    """Vectorised Philox4x32-10 (Random123): counters as arrays (broadcast), key as two ints; four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & _MASK for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0 = _M0 * c[0]
        p1 = _M1 * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & _MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & _MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0 = (k0 + _W0) & 0xFFFFFFFF
        k1 = (k1 + _W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def uniform(x) -> np.ndarray:
    return (np.asarray(x, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) * 2.0**-24


def _probs_table(l, params) -> np.ndarray:
    """(F, K, C) unnormalised probabilities of a Categorical / Binomial layer, fp64."""
    if l.type == "categorical":
        if "probs" in params:
            return params["probs"].numpy()
        return np.exp(params["logits"].numpy())
    T = int(l.config["total_count"])
    p = params["probs"].numpy() if "probs" in params else 1.0 / (1.0 + np.exp(-params["logits"].numpy()))
    c = np.arange(T + 1)
    from math import lgamma

    lc = np.array([lgamma(T + 1) - lgamma(i + 1) - lgamma(T - i + 1) for i in c])
    with np.errstate(divide="ignore"):
        lp = lc + c * np.log(p[..., None]) + (T - c) * np.log1p(-p[..., None])
    return np.exp(lp)


def sample_restated(plan: Plan, tensors, num_samples: int, seed: int, *, tol: float = 1e-5):
    """(x (N, D) float64, choices [(F, N) int per sum / mixing / CP-T / Tucker layer], near (N,) bool): `near` marks the
    samples of which some draw had its uniform within `tol` of an interior end of the interval it fell in (the device's fp32
    tables may choose the neighbouring entry there)."""
    from oracle.torch_oracle import as_torch, eval_param, evaluate_plan

    tt = {k: (v.double() if not v.is_complex() else v) for k, v in as_torch(tensors).items()}
    D, N = plan.num_variables, int(num_samples)
    gauss = any(l.type == "gaussian" for l in plan.layers)
    xm = torch.zeros((1, D), dtype=torch.float64 if gauss else torch.int64)
    _, outs = evaluate_plan(plan, tt, xm, return_all=True, integrate_mask=torch.ones((1, D), dtype=torch.bool))
    lz = [o[:, 0, :].numpy() for o in outs]  # (F, K) log partition functions
    folds = [l.num_folds for l in plan.layers]
    off = np.concatenate([[0], np.cumsum(folds)]).astype(np.int64)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    n = np.arange(N, dtype=np.uint64)
    sel = [np.full((F, N), -1, dtype=np.int64) for F in folds]
    root = resolve_fold_index(plan.output, folds).reshape(-1, 2)[0]
    sel[root[0]][root[1]] = 0
    x = np.zeros((N, D), dtype=np.float64)
    near = np.zeros(N, dtype=bool)
    choices: dict[int, np.ndarray] = {}

    def draw(rows: np.ndarray, u: np.ndarray, on: np.ndarray) -> np.ndarray:
        cdf = np.cumsum(rows, axis=1)
        T = cdf[:, -1:]
        t = u[:, None] * T
        i = np.argmax(t < cdf, axis=1)
        r = np.arange(len(i))
        lo = np.where(i > 0, cdf[r, np.maximum(i - 1, 0)] / T[:, 0], -1.0)  # the interior ends of the chosen interval
        hi = np.where(cdf[r, i] < T[:, 0], cdf[r, i] / T[:, 0], 2.0)
        near[on] |= (np.abs(u - lo) < tol) | (np.abs(u - hi) < tol)
        return i

    for j in range(len(plan.layers) - 1, -1, -1):
        l = plan.layers[j]
        params = {pn: eval_param(pg, tt) for pn, pg in l.params.items()}
        ch = None if l.inputs is None else resolve_fold_index(l.inputs, folds)
        if l.type in ("sum", "cpt", "tucker"):
            choices[j] = np.full((l.num_folds, N), -1, dtype=np.int64)
            w = params["weight"].numpy()
        for f in range(l.num_folds):
            k = sel[j][f]
            on = np.nonzero(k >= 0)[0]
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
                x[on, int(l.scope_idx[f, 0])] = mean[k] + sd[k] * z
                continue
            u = uniform(p[0])
            if l.type in ("categorical", "binomial"):
                x[on, int(l.scope_idx[f, 0])] = draw(_probs_table(l, params)[f][k], u, on)
                continue
            Ki = l.num_input_units
            zc = np.stack([lz[ch[f, h, 0]][ch[f, h, 1]] for h in range(l.arity)])  # (H, Ki)
            if l.type == "cpt":
                ent = zc.sum(0)
            elif l.type == "tucker":
                ent = (zc[0][:, None] + zc[1][None, :]).reshape(-1)
            else:
                ent = zc.reshape(-1)
            rows = w[f][k]  # (n_on, M)
            with np.errstate(invalid="ignore", over="ignore"):
                rows = np.where(rows > 0, rows * np.exp(ent - ent[np.isfinite(ent)].max()), 0.0)
            i = draw(rows, u, on)
            mixing = l.type == "sum" and (lambda g_: len(g_.output.ids) == 1 and g_.nodes[g_.output.ids[0]].op == "mixing_weight")(
                l.params["weight"])
            choices[j][f, on] = i // Ki if mixing else i
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
    return x, [choices[j] for j in sorted(choices)], near
