"""A numpy restatement of the M-step of `HipEMTrainer` (cirkit_amd/em.py, cirkit_amd/csrc/ck_em.hip), for tests only.

The contract of DESIGN.md section 11 ("EM training") on the USER's plan: from the statistics of
`statistics_restated` (tests/statistics_restatement.py) to new RAW tensors, every parameter graph inverted in closed form, in
fp64 -- or, with ``dtype=np.float32``, the same formulas in fp32: the yardstick of the GPU tolerances.  The graph kinds are
read off the ops of each graph here, independently of `cirkit_amd.em.em_jobs`.
"""
from __future__ import annotations

import numpy as np

from cirkit_amd.plan import Plan

CLAMP = 2.0 ** -24


def _raw(g, tensors, dt) -> tuple[str, np.ndarray]:
    name = g.nodes[0].config["tensor"]
    v = tensors[name]
    return name, np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v).astype(dt)


def _logit(s, dt):
    s = np.clip(s, dt(CLAMP), dt(1.0 - CLAMP)).astype(dt)
    return (np.log(s) - np.log1p(-s)).astype(dt)


def _sigmoid(x, dt):
    return (dt(1) / (dt(1) + np.exp(-x))).astype(dt)


def _rows(raw, N, sup, is_log: bool, step, a, dt) -> np.ndarray:
    """theta = (1 - step) theta_old + step (N + a [sup]) / sum over the last axis, as log theta or theta; rows without mass
    keep `raw`.  `sup` None: the support is read off the row itself."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if is_log:
            mx = raw.max(axis=-1, keepdims=True)
            u = np.exp(raw - np.where(np.isfinite(mx), mx, 0).astype(dt)).astype(dt)
        else:
            u = np.maximum(raw, 0).astype(dt)
        tot = u.sum(axis=-1, keepdims=True, dtype=dt)
        old = np.where(tot > 0, u / np.where(tot > 0, tot, 1), 0).astype(dt)
        if sup is None:
            sup = u > 0
        n = (N.astype(dt) + dt(a) * sup.astype(dt)).astype(dt)
        den = n.sum(axis=-1, keepdims=True, dtype=dt)
        theta = (dt(1 - step) * old + dt(step) * (n / np.where(den > 0, den, 1))).astype(dt)
        new = np.log(theta).astype(dt) if is_log else theta
    return np.where(den > 0, new, raw).astype(dt)


def em_restated(plan: Plan, tensors, stats: dict, step_size: float = 1.0, pseudocount: float = 0.0, *, dtype=np.float64) -> dict:
    """New raw tensors {name: array in the user plan's shape} from the statistics `stats` (``edge``, ``leaf`` and the
    evaluated weights ``w`` of `statistics_restated`)."""
    dt = np.dtype(dtype).type
    out = {}
    for j, l in enumerate(plan.layers):
        ops = {pn: list(g.ops) for pn, g in l.params.items()}
        if l.type in ("sum", "cpt", "tucker"):
            g = l.params["weight"]
            name, raw = _raw(g, tensors, dt)
            N, sup = np.asarray(stats["edge"][j]), np.asarray(stats["w"][j]) > 0
            if ops["weight"][-1] == "mixing_weight":
                assert ops["weight"] in (["tensor", "mixing_weight"], ["tensor", "softmax", "mixing_weight"])
                F, K, H = raw.shape
                k = np.arange(K)
                pick = lambda t: np.stack([t[:, k, h * K + k] for h in range(H)], axis=-1)  # noqa: E731  (F, K, H) diagonals
                out[name] = _rows(raw, pick(N), pick(sup), "softmax" in ops["weight"], step_size, pseudocount, dt)
            else:
                assert ops["weight"] in (["tensor"], ["tensor", "softmax"]), ops
                out[name] = _rows(raw, N, sup, ops["weight"] == ["tensor", "softmax"], step_size, pseudocount, dt)
        elif l.type == "categorical":
            (pn, g), = l.params.items()
            assert ops[pn] in (["tensor"], ["tensor", "softmax"]), ops
            name, raw = _raw(g, tensors, dt)
            is_log = pn == "logits" or ops[pn] == ["tensor", "softmax"]
            out[name] = _rows(raw, np.asarray(stats["leaf"][j]), None, is_log, step_size, pseudocount, dt)
        elif l.type == "binomial":
            assert ops == {"probs": ["tensor", "sigmoid"]}, ops
            name, raw = _raw(l.params["probs"], tensors, dt)
            N = np.asarray(stats["leaf"][j]).astype(dt)
            T = N.shape[-1] - 1
            tot = N.sum(axis=-1, dtype=dt)
            num = (N * np.arange(T + 1, dtype=dt)).sum(axis=-1, dtype=dt)
            with np.errstate(divide="ignore", invalid="ignore"):
                hat = (num / (dt(T) * np.where(tot > 0, tot, 1))).astype(dt)
                p = (dt(1 - step_size) * _sigmoid(raw, dt) + dt(step_size) * hat).astype(dt)
                out[name] = np.where(tot > 0, _logit(p, dt), raw).astype(dt)
        elif l.type == "gaussian":
            assert ops == {"mean": ["tensor"], "stddev": ["tensor", "scaled_sigmoid"]}, ops
            c = l.params["stddev"].nodes[1].config
            lo, hi = dt(c.get("vmin", 0.0)), dt(c.get("vmax", 1.0))
            nm, mean = _raw(l.params["mean"], tensors, dt)
            ns, rs = _raw(l.params["stddev"], tensors, dt)
            S = np.asarray(stats["leaf"][j]).astype(dt)
            s0, s1, s2 = S[..., 0], S[..., 1], S[..., 2]
            ok = s0 > 0
            den = np.where(ok, s0, 1).astype(dt)
            mu_hat = (s1 / den).astype(dt)
            var_hat = np.maximum(s2 / den - mu_hat * mu_hat, 0).astype(dt)
            sd_old = (lo + (hi - lo) * _sigmoid(rs, dt)).astype(dt)
            var = (dt(1 - step_size) * sd_old * sd_old + dt(step_size) * var_hat).astype(dt)
            out[nm] = np.where(ok, dt(1 - step_size) * mean + dt(step_size) * mu_hat, mean).astype(dt)
            out[ns] = np.where(ok, _logit((np.sqrt(var) - lo) / (hi - lo), dt), rs).astype(dt)
        else:
            assert not l.params, (j, l.type)
    return out


def normalised_parameters(plan: Plan, tensors) -> dict:
    """{(layer, parameter): the oracle's fp64 evaluation of the graph} -- what the raw tensors MEAN.  Mixing weights as
    their (F, K, H) diagonals, Categorical logits as the distribution they normalise to."""
    import torch

    from oracle.torch_oracle import as_torch, eval_param

    tt = {k: v.double() for k, v in as_torch({k: np.asarray(v) for k, v in tensors.items()}).items()}
    out = {}
    for j, l in enumerate(plan.layers):
        for pn, g in l.params.items():
            v = eval_param(g, tt)
            if g.ops[-1] == "mixing_weight":
                K = v.shape[1]
                k = np.arange(K)
                v = torch.stack([v[:, k, h * K + k] for h in range(v.shape[2] // K)], dim=-1)
            if pn == "logits":
                v = torch.softmax(v, dim=-1)
            out[(j, pn)] = v.numpy()
    return out
