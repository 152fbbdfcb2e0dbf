"""Soft and interval evidence of a squared circuit (cirkit_amd/squared_soft.py, csrc/ck_sqsoft.hip) restated in torch on the
host, and their yardstick.

`enumerated_soft` is the yardstick: c evaluated in fp64 by the repository's oracle on every completion of the soft and the
integrated variables, ``logsumexp(2 Re log c + sum_v log lambda)`` over them.

`restated_soft` is the ALGORITHM: the input fold of a soft variable becomes the logarithm of its weighted Gram matrix
``G_b[k, l] = sum_s lambda_b(s) e_k(s) conj(e_l(s))`` -- the weights shifted by their clamped maximum per row, a table of
logarithms by the clamped maximum of every unit's column -- and every fold whose scope meets the soft set is evaluated at K^2
units by the stages of `squared_marginal_restatement.restated_log_marginal`.  It runs in the dtype it is given.

The cases the CPU tests (the fp32 run stays below half the GPU bound) and the GPU tests share are built here, once per process.
"""
import functools
import itertools

import numpy as np
import torch

import squared_marginal_restatement as R
from cirkit_amd.functional import squared_partition_plan
from cirkit_amd.plan import resolve_fold_index

OBSERVED, INTEGRATED, MIXED = R.OBSERVED, R.INTEGRATED, R.MIXED


def mask_of(ids, D):
    m = np.zeros(D, dtype=bool)
    m[list(ids)] = True
    return m


def enumerated_soft(plan, tensors, x, log_lik, soft, mask, states):
    """(B,) fp64, unnormalised: logsumexp over every completion of the soft variables `soft` (bool mask; the S axis of
    `log_lik` (B, |S|, C) in ascending variable order) and the integrated variables `mask` of 2 Re log c + sum_v log lambda."""
    soft, mask = np.asarray(soft, dtype=bool), np.asarray(mask, dtype=bool)
    assert not (soft & mask).any()
    sv, free = np.nonzero(soft)[0], np.nonzero(soft | mask)[0]
    assert states ** len(free) <= R.MAX_WORLDS, "too many completions to enumerate"
    x = torch.as_tensor(x).to(torch.int64)
    ll = torch.as_tensor(log_lik).to(torch.float64)
    comp = R.all_worlds(len(free), states)  # (W, |S| + |M|)
    rows = x[:, None, :].repeat(1, comp.shape[0], 1)
    rows[:, :, torch.from_numpy(free)] = comp[None]
    lc = R.log_c2_of(plan, tensors, rows.reshape(-1, x.shape[1])).reshape(x.shape[0], -1)
    for j, v in enumerate(sv):
        lc = lc + ll[:, j, :][:, rows[0, :, v]]
    return torch.logsumexp(lc, dim=1)


def soft_classes(plan, soft, mask):
    """`classes_from_scopes` of the integrated set, then every fold whose scope meets the soft set MIXED."""
    S = frozenset(int(v) for v in np.nonzero(np.asarray(soft))[0])
    cls = R.classes_from_scopes(plan, mask)
    return [np.asarray([MIXED if s & S else c for s, c in zip(layer, cl)], dtype=np.int8) for layer, cl in zip(R.fold_scopes(plan), cls)]


def log_gram(log_e, ll, table_log):
    """log of the weighted Gram matrix: log_e (C, K) the logarithms of a fold's table in the circuit's semiring, ll (B, C) real
    log weights -> (B, K^2), unit k K + l with k the unconjugated factor."""
    real = ll.dtype
    big = torch.finfo(real).max
    m = ll.amax(dim=1, keepdim=True).clamp(min=-big, max=big)
    w = torch.exp(ll - m)
    if table_log:  # (a real table of logarithms: shifted unit by unit)
        mt = log_e.amax(dim=0).clamp(min=-big, max=big)
        a = torch.exp(log_e - mt)
        shift = m + (mt[:, None] + mt[None, :]).reshape(1, -1)
    else:
        a = torch.exp(log_e)
        shift = m
    g = torch.einsum("bs,sk,sl->bkl", w.to(a.dtype), a, a.conj()).flatten(1)
    return torch.log(g) + shift


def restated_soft(plan, tensors, x, log_lik, soft, mask, states, dtype=torch.float64):
    """(B,) unnormalised log evidence and log Z in `dtype`'s real type."""
    from oracle.torch_oracle import eval_param, evaluate_plan

    soft, mask = np.asarray(soft, dtype=bool), np.asarray(mask, dtype=bool)
    tt = R._cast(tensors, dtype)
    x = torch.as_tensor(x).clone()
    x[:, torch.from_numpy(soft | mask)] = 0
    ll = torch.as_tensor(log_lik).to(dtype)
    _, c_out = evaluate_plan(plan, tt, x, return_all=True)
    every = torch.arange(states)[:, None].expand(states, plan.num_variables).contiguous()
    _, e_out = evaluate_plan(plan, tt, every, return_all=True)  # row s: every input fold at state s
    z_plan, z_of = squared_partition_plan(plan, return_layer_map=True)
    z_root, z_out = evaluate_plan(z_plan, tt, None, return_all=True)
    cls = soft_classes(plan, soft, mask)
    folds = [l.num_folds for l in plan.layers]
    conj = plan.semiring == "complex-lse-sum"
    pos = np.cumsum(soft) - 1
    full = {}

    def child(p, f):
        if cls[p][f] == MIXED:
            return full[(p, f)]
        if cls[p][f] == INTEGRATED:
            return z_out[z_of[p]][f]
        y = c_out[p][f]
        return (y[:, :, None] + (y.conj() if conj else y)[:, None, :]).flatten(1)

    for i, l in enumerate(plan.layers):
        mixed = [f for f in range(l.num_folds) if cls[i][f] == MIXED]
        if l.inputs is None:
            for f in mixed:
                v = int(l.scope_idx[f][0])
                full[(i, f)] = log_gram(e_out[i][f], ll[:, pos[v], :states], l.type == "categorical")
            continue
        ch = resolve_fold_index(l.inputs, folds)
        w = eval_param(l.params["weight"], tt) if "weight" in l.params else None
        for f in mixed:
            v = sum(child(int(p), int(g)) for p, g in ch[f])
            if l.type != "hadamard":
                K = l.num_input_units
                v = R._stage(v.reshape(-1, K, K), w[f])
                v = R._stage(v, w[f]).flatten(1)
            full[(i, f)] = v
    op, of = (int(v) for v in resolve_fold_index(plan.output, folds).reshape(-1, 2)[0])
    val = full[(op, of)][:, 0]
    lz = z_root.reshape(-1)[0]
    return (val.real if val.is_complex() else val), (lz.real if lz.is_complex() else lz)


def interval_log_lik(lo, hi, ids, states):
    """(B, |ids|, states) fp64: 0 inside [lo, hi] at the variables `ids`, -inf outside (bounds already inside 0 .. states - 1)."""
    s = torch.arange(states)[None, None, :]
    lo, hi = (torch.as_tensor(t)[:, list(ids)][:, :, None] for t in (lo, hi))
    return torch.where((s >= lo) & (s <= hi), 0.0, float("-inf")).to(torch.float64)


def log_lik_of(B, S, C, seed):
    """Random log weights within e^+-8 of each other per variable: uniform on [-4, 4]."""
    return torch.from_numpy(np.random.default_rng(seed).uniform(-4.0, 4.0, size=(B, S, C)))


def yardstick(plan, tensors, x, ll, soft, mask, states):
    """The enumeration where the completions can be listed, else the fp64 restatement (pinned to the enumeration by the CPU
    tests on every case that can be listed)."""
    if states ** int((soft | mask).sum()) <= R.MAX_WORLDS:
        return enumerated_soft(plan, tensors, x, ll, soft, mask, states)
    return restated_soft(plan, tensors, x, ll, soft, mask, states)[0]


# ---- the cases the CPU and the GPU tests share: (name, soft ids, integrated ids) ---------------------------------------------
TINY_VARS = (0, 2, 5)
TINY_OTHER = 3


def tiny_splits():
    subsets = [c for n in (1, 2, 3) for c in itertools.combinations(TINY_VARS, n)]
    return [(s, m) for s in subsets for m in ((), (TINY_OTHER,))]


@functools.lru_cache(maxsize=None)
def tiny_expected(sum_product):
    """plan, tensors, x (5, 6), per split (soft ids, integrated ids, log_lik (5, |S|, 3), enumeration)."""
    plan, tensors, states = R.tiny_case(sum_product)
    x = R.rows_of(6, states, 5)
    out = []
    for j, (s, m) in enumerate(tiny_splits()):
        ll = log_lik_of(5, len(s), states, 100 + j)
        out.append((s, m, ll, enumerated_soft(plan, tensors, x, ll, mask_of(s, 6), mask_of(m, 6), states)))
    return plan, tensors, x, out


# one pixel beside an integrated and beside an observed one (the first product layer pairs pixels 4 and 5), a 2 x 2 block, all 16
EMB32_SPLITS = (((5,), (4,)), ((5,), ()), ((0, 1, 4, 5), (15,)), (tuple(range(16)), ()))


@functools.lru_cache(maxsize=None)
def emb32_expected():
    plan, tensors, states = R.emb32_case()
    x = R.rows_of(16, states, 33)
    out = []
    for j, (s, m) in enumerate(EMB32_SPLITS):
        ll = log_lik_of(33, len(s), states, 200 + j)
        out.append((s, m, ll, yardstick(plan, tensors, x, ll, mask_of(s, 16), mask_of(m, 16), states)))
    return plan, tensors, x, out, R.oracle_log_z(plan, tensors)


CAT_SPLITS = (((5,), ()), ((5, 10), ()), ((0, 3, 5, 10, 12), (7,)))


@functools.lru_cache(maxsize=None)
def cat_expected():
    plan, tensors, states = R.cat_case()
    x = torch.from_numpy(np.random.default_rng(2).integers(0, states, size=(3, 16)))
    out = []
    for j, (s, m) in enumerate(CAT_SPLITS):
        ll = log_lik_of(3, len(s), states, 300 + j)
        out.append((s, m, ll, yardstick(plan, tensors, x, ll, mask_of(s, 16), mask_of(m, 16), states)))
    return plan, tensors, x, out
