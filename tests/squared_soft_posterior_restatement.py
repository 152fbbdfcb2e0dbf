"""Posteriors and sampling under soft evidence of a squared circuit (cirkit_amd/squared_soft_posterior.py,
csrc/ck_sqsoftdown.hip, `ck_squared_path_soft_bwd`) restated in torch / numpy on the host, in the dtype they are given.

`restated_soft_query_log_marginals` is the ALGORITHM: the soft bottom-up pass of `squared_soft_restatement` (the input fold of a
soft variable is the logarithm of its weighted Gram matrix, every fold whose scope meets the soft set is evaluated at K^2 units),
the down pass of `squared_down_restatement` over those values (a down child receives dP plus the values of the OTHER children:
the G that reaches the input fold of v never holds lambda_v), and the weighted leaf ``log lambda_v(s) + S.leaf_log_m``.

Its yardstick is the enumeration (`expected_soft_query_log_marginals`): ``log m(v, s)`` is `RS.enumerated_soft` with row v of
``log_lik`` replaced by ``-inf`` except ``log_lik[v, s]`` at ``s``.

`restated_soft_sampler` draws the soft variables one after the other with the Philox stream of `squared_sampling_restatement`:
at the step of v the variables drawn before are observed, v and the ones still to draw are the soft set.

Comparison: `P.check` ("Posterior marginals of squared circuits"): a state that holds at least e^-4 of its
row's largest expected mass is held to 1e-4 max(1, |want|) on the logarithm, the others to 4e-5 in linear space after the shift by
the row's expected maximum; at most a quarter of a case's finite states may take the linear route.
"""
import functools
import os

import numpy as np
import torch

import squared_down_restatement as P
import squared_marginal_restatement as R
import squared_sampling_restatement as S
import squared_soft_restatement as RS
from cirkit_amd.squared_sampling import path_plan, tree_order
from sampling_restatement import philox4x32_10, uniform

NEG_INF = float("-inf")


class SoftProduct(S.Product):
    """`S.Product` under soft evidence: every fold whose scope meets the soft set is evaluated, the input folds as weighted Grams."""

    def __init__(self, plan, tensors, x, log_lik, soft, mask, states, dtype=torch.float64):
        from oracle.torch_oracle import evaluate_plan

        soft, mask = np.asarray(soft, dtype=bool), np.asarray(mask, dtype=bool)
        super().__init__(plan, tensors, x, soft | mask, dtype)  # (x is cleaned at both sets)
        self.mask = mask
        self.cls = RS.soft_classes(plan, soft, mask)
        self.ll = torch.as_tensor(log_lik).to(dtype)
        self.pos = np.cumsum(soft) - 1
        self.states = states
        every = torch.arange(states)[:, None].expand(states, plan.num_variables).contiguous()
        _, self.e_out = evaluate_plan(plan, self.tt, every, return_all=True)  # row s: every input fold at state s

    def value(self, p, f):
        l = self.plan.layers[p]
        if l.inputs is None and self.cls[p][f] == R.MIXED:
            if (p, f) not in self.full:
                v = int(l.scope_idx[f][0])
                self.full[(p, f)] = RS.log_gram(self.e_out[p][f], self.ll[:, self.pos[v], :self.states], l.type == "categorical")
            return self.full[(p, f)]
        return super().value(p, f)


def restated_soft_query_log_marginals(plan, tensors, x, log_lik, soft, mask, states, dtype=torch.float64, return_evidence=False):
    """(B, |S|, C) unnormalised ``log m_b(v, s)`` in `dtype`'s real type, the S axis in ascending variable order."""
    soft = np.asarray(soft, dtype=bool)
    ids = np.nonzero(soft)[0].tolist()
    prod = SoftProduct(plan, tensors, x, log_lik, soft, mask, states, dtype)
    G = P.down_gradients(prod, ids)
    B = torch.as_tensor(x).shape[0]
    real = prod.ll.dtype
    out = torch.stack([S.leaf_log_m(G[path_plan(plan, v).leaf], S.leaf_values(plan, tensors, v, states, dtype)).expand(B, -1)
                       + prod.ll[:, j, :states].to(real) for j, v in enumerate(ids)], dim=1)
    if not return_evidence:
        return out
    ev = prod.value(*P.output_fold(plan))[:, 0]
    return out, (ev.real if ev.is_complex() else ev).expand(B)


def expected_soft_query_log_marginals(plan, tensors, x, log_lik, soft, mask, states):
    """(B, |S|, C) fp64: the yardstick.  Entry (v, s): the evidence with lambda_v replaced by the indicator of s times lambda_v(s)."""
    soft = np.asarray(soft, dtype=bool)
    ll = torch.as_tensor(log_lik).to(torch.float64)
    n = int(soft.sum())
    cols = []
    for j in range(n):
        per_state = []
        for s in range(states):
            one = ll.clone()
            one[:, j, :] = NEG_INF
            one[:, j, s] = ll[:, j, s]
            per_state.append(RS.yardstick(plan, tensors, x, one, soft, np.asarray(mask, dtype=bool), states))
        cols.append(torch.stack(per_state, dim=1))
    return torch.stack(cols, dim=1)


def quadratic_log_m(G, a, ll, tlog=False):
    """The weighted leaf alone in fp64: G (B, K, K) real or complex log values, a (C, K) the table (logarithms when `tlog`),
    ll (B, C) -> (B, C)."""
    a = torch.exp(a.double()) if tlog else a.double()
    return S.leaf_log_m(G, a.to(G.dtype)) + ll.double()


def restated_soft_sampler(plan, tensors, x, log_lik, soft, mask, states, seed, order=None, dtype=torch.float64, row0=0):
    """The sampler on the host.  x (B, D) int64 (entries at the soft and the integrated variables are ignored), `log_lik`
    (B, |S|, C), the S axis in ascending variable order.  Returns the completed rows (integrated columns as given, -1 in every soft column of a row without
    mass) and per row the smallest distance of a draw's u to a boundary of its bin (`S.restated_sampler`)."""
    soft, mask = np.asarray(soft, dtype=bool), np.asarray(mask, dtype=bool)
    ids = np.nonzero(soft)[0].tolist()
    order = [v for v in tree_order(plan) if soft[v]] if order is None else list(order)
    given = torch.as_tensor(x)
    x = given.clone()
    ll = torch.as_tensor(log_lik).double()
    B = x.shape[0]
    x[:, torch.from_numpy(soft | mask)] = 0
    left = soft.copy()
    margin = np.full(B, np.inf)
    dead = np.zeros(B, dtype=bool)
    n = np.arange(B, dtype=np.uint64) + np.uint64(row0)
    for v in order:
        pp = path_plan(plan, v)
        u = uniform(philox4x32_10(n, S.global_fold_id(plan, *pp.leaf), 0, 0, seed & 0xFFFFFFFF, seed >> 32)[0])
        rest = [w for w in ids if left[w]]  # v and the variables still to draw: the soft set of this step
        sub = ll[:, [ids.index(w) for w in rest], :]
        lm = restated_soft_query_log_marginals(plan, tensors, x, sub, left, mask, states, dtype)[:, rest.index(v), :].double().numpy()
        state, cdf = S.draw(lm, u)
        dead |= state < 0
        lo = np.where(state > 0, np.take_along_axis(cdf, np.maximum(state - 1, 0)[:, None], 1)[:, 0], -np.inf)
        hi = np.where(state < states - 1, np.take_along_axis(cdf, np.maximum(state, 0)[:, None], 1)[:, 0], np.inf)
        margin = np.minimum(margin, np.minimum(u - lo, hi - u))
        x[:, v] = torch.from_numpy(np.where(dead, 0, state))
        left[v] = False
    out = x.clone()
    out[:, torch.from_numpy(mask)] = given[:, torch.from_numpy(mask)]  # (integrated columns come back as given)
    out[torch.from_numpy(dead)[:, None] & torch.from_numpy(soft)[None, :]] = -1
    return out, margin


def enumerated_joint(plan, tensors, x_row, log_lik_row, soft, mask, states):
    """(states^|S|,) fp64: p(x_S | lambda, x_O) of ONE row over the worlds of its soft variables, first soft variable slowest."""
    soft, mask = np.asarray(soft, dtype=bool), np.asarray(mask, dtype=bool)
    ids = np.nonzero(soft)[0]
    worlds = R.all_worlds(len(ids), states)
    rows = torch.as_tensor(x_row).reshape(1, -1).repeat(worlds.shape[0], 1)
    rows[:, torch.from_numpy(ids)] = worlds
    lw = R.yardstick(plan, tensors, rows, mask, states)
    ll = torch.as_tensor(log_lik_row).double()
    for j in range(len(ids)):
        lw = lw + ll[j, worlds[:, j]]
    return torch.exp(lw - torch.logsumexp(lw, dim=0)).numpy()


# ---- the cases the CPU and the GPU tests share ------------------------------------------------------------------------------
WEIGHT_SCALE = 0.25  # `RS.log_lik_of` draws log weights on [-4, 4]; on top of the model's own spread that puts more than a quarter of the
#                      states of a case below e^-4 of their row's largest (the linear route of `P.check`): the weights here lie on [-1, 1]


def with_holes(ll, seed, share=0.15):
    """`ll` scaled by `WEIGHT_SCALE`, with exact -inf in a share of its entries, never a whole variable of a row."""
    rng = np.random.default_rng(seed)
    ll = ll * WEIGHT_SCALE
    hole = torch.from_numpy(rng.random(tuple(ll.shape)) < share)
    hole[:, :, 0] &= ~hole.all(dim=2)
    ll[hole] = NEG_INF
    return ll


TINY_SEED = 520  # the weights of split j: seed TINY_SEED + j, their holes TINY_SEED + 100 + j


def tiny_splits():
    """Every subset of `RS.TINY_VARS` with and without `RS.TINY_OTHER` integrated, and S = all six variables."""
    return RS.tiny_splits() + [(tuple(range(6)), ())]


@functools.lru_cache(maxsize=None)
def tiny_expected(sum_product):
    """plan, tensors, x (5, 6), per split (soft ids, integrated ids, log_lik (5, |S|, 3), enumerated (5, |S|, 3))."""
    plan, tensors, states = R.tiny_case(sum_product)
    x = P.tiny_rows()
    out = []
    for j, (s, m) in enumerate(tiny_splits()):
        ll = with_holes(RS.log_lik_of(5, len(s), states, TINY_SEED + j), TINY_SEED + 100 + j)
        out.append((s, m, ll, expected_soft_query_log_marginals(plan, tensors, x, ll, RS.mask_of(s, 6), RS.mask_of(m, 6), states)))
    return plan, tensors, x, out


# one pixel, a 2 x 2 block of the quad tree, all 16, and scattered pixels with two integrated
EMB32_SPLITS = (((5,), ()), ((0, 1, 4, 5), ()), (tuple(range(16)), ()), ((1, 6, 11, 12), (3, 9)))
CAT_SPLIT = ((0, 6, 15), (1,))
GOLDEN = "sq_soft_posterior_expected.npz"
DRAW_ROWS, DRAW_SEED = 2048, 20250201
CHI_ROWS, CHI_SEED, CHI_VARS = 1 << 16, 20250202, (2, 3, 6, 7)


def emb32_rows():
    return P.emb32_rows()


def emb32_log_lik(i):
    s, _ = EMB32_SPLITS[i]
    return with_holes(RS.log_lik_of(33, len(s), 3, 700 + i), 800 + i)


def emb32_expected(i):
    plan, tensors, states = R.emb32_case()
    s, m = EMB32_SPLITS[i]
    return expected_soft_query_log_marginals(plan, tensors, emb32_rows(), emb32_log_lik(i), RS.mask_of(s, 16), RS.mask_of(m, 16), states).numpy()


def cat_rows():
    return P.cat_rows()


def cat_log_lik():
    return with_holes(RS.log_lik_of(3, len(CAT_SPLIT[0]), 256, 900), 901)


def cat_expected():
    """Three soft 256-state pixels and one integrated: past enumeration, the fp64 restatement (pinned to the enumeration by the
    CPU tests on every case that can be listed)."""
    plan, tensors, states = R.cat_case()
    s, m = CAT_SPLIT
    return restated_soft_query_log_marginals(plan, tensors, cat_rows(), cat_log_lik(), RS.mask_of(s, 16), RS.mask_of(m, 16), states).numpy()


def draw_case():
    """x (2048, 16), soft (16,) bool, integrated (16,) bool, log_lik (2048, 8, 3), seed on `R.emb32_case`: a random half of the
    pixels soft, one of the others integrated, the rest observed; the default order."""
    rng = np.random.default_rng(29)
    soft = np.zeros(16, dtype=bool)
    soft[rng.choice(16, size=8, replace=False)] = True
    mask = np.zeros(16, dtype=bool)
    mask[int(np.nonzero(~soft)[0][3])] = True
    ll = with_holes(RS.log_lik_of(DRAW_ROWS, 8, 3, 950), 951, share=0.1)
    return R.rows_of(16, 3, DRAW_ROWS, seed=31), soft, mask, ll, DRAW_SEED


def draw_expected():
    plan, tensors, states = R.emb32_case()
    x, soft, mask, ll, seed = draw_case()
    out, margin = restated_soft_sampler(plan, tensors, x, ll, soft, mask, states, seed)
    return out.numpy().astype(np.int8), margin


def chi_case():
    """One row of evidence repeated: x (16,), soft = `CHI_VARS`, log_lik (4, 3) with one exact -inf, and the enumerated joint (81,)."""
    plan, tensors, states = R.emb32_case()
    x = R.rows_of(16, 3, 1, seed=37)[0]
    ll = RS.log_lik_of(1, 4, 3, 960)[0]
    ll[1, 2] = NEG_INF
    soft = RS.mask_of(CHI_VARS, 16)
    return x, soft, ll, enumerated_joint(plan, tensors, x, ll, soft, np.zeros(16, dtype=bool), states)


# ---- hand-built launches of the leaf kernel alone -------------------------------------------------------------------------------
LEAF_UNITS = (3, 5, 32)
LEAF_ROWS = ((1, 1), (5, 3), (19, 20))  # (B, rows per block)


def leaf_states(C):
    """The state counts of the three variables of one launch of the leaf kernel alone."""
    return [C, 5 if C == 3 else 3, 40]


def leaf_case(cplx, tlog, K, C, B):
    """A hand-built launch of `ck_squared_soft_down_leaf`: G (2, B, K, K) log values (the third variable has offset -1), one
    table per variable, weights with -inf, and ``log m`` (B, 3, Cl + 1) in fp64.  Values close to each other -- tables of
    1 +- 0.3, G of +- 0.5, under c32 one off-diagonal element of G in ten negative and small -- so that the states of a row stay within e^-4 of its largest, where the
    bound on the logarithm can be asked of them (`S.hand_path_case`)."""
    Cs, seed = leaf_states(C), 1000 + 7 * C + K + B
    g = torch.Generator().manual_seed(seed)
    nq, Cl = len(Cs), max(Cs) + 1

    def signs(*sh):  # one entry in ten negative, as `S.hand_path_case`: the sums stay far from cancelling
        return torch.where(torch.rand(*sh, generator=g) < 0.1, -1.0, 1.0).double()

    re = 0.5 * torch.randn(nq - 1, B, K, K, generator=g, dtype=torch.float64)
    if B > 1:
        re[:, B - 1] = NEG_INF  # the last row: an all -inf G, so every state is -inf (not NaN)
    if cplx:  # (a negative element lies off the diagonal and is a small one: the quadratic forms stay clear of 0, where fp32 cannot tell the sign)
        neg = (signs(nq - 1, B, K, K) < 0) & ~torch.eye(K, dtype=torch.bool)
        G = torch.complex(re - 3.0 * neg.double(), neg.double() * np.pi)
    else:
        G = re
    tables = []
    for Cj in Cs:
        t = 0.3 * torch.randn(Cj + 1, K, generator=g, dtype=torch.float64)
        tables.append(t if tlog else (1.0 + t).abs())
    ll = with_holes(RS.log_lik_of(B, nq, Cl, seed), seed + 1)
    ll[0, 0, :2] = NEG_INF
    want = torch.full((B, nq, Cl + 1), NEG_INF, dtype=torch.float64)
    top = torch.full((1, K, K), NEG_INF, dtype=torch.float64)
    top[0, 0, 0] = 0
    for j, Cj in enumerate(Cs):
        Gj = G[j] if j < nq - 1 else (torch.complex(top, torch.zeros_like(top)) if cplx else top)
        want[:, j, :Cj] = quadratic_log_m(Gj, tables[j][:Cj], ll[:, j, :Cj], tlog).expand(B, -1)
    return G, tables, ll, want


def golden():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)) as z:
        return {k: z[k] for k in z.files}


def record():
    rec = {f"emb32_want_{i}": emb32_expected(i) for i in range(len(EMB32_SPLITS))}
    rec["cat_want"] = cat_expected()
    rec["draw_out"], rec["draw_margin"] = draw_expected()
    rec["chi_joint"] = chi_case()[3]
    return rec
