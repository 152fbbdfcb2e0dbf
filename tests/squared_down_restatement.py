"""Posterior marginals of a squared circuit for a whole set of query variables (cirkit_amd/squared_posterior.py,
csrc/ck_sqdown.hip) restated in torch / numpy on the host, in the dtype they are given.

`restated_query_log_marginals` is the ALGORITHM, layer by layer: with ``M = Q + I`` integrated out, the derivative G of the root
of the product circuit is kept for every fold whose scope meets Q (the down folds, here from explicit scope sets).  From the
output fold (log 1 at unit 0) downwards a fold's G goes through the two transposed TensorDot stages where its layer has them
(dP = W^T G W) and every child that is a down fold receives dP plus, in log space, the values of the OTHER children under M
(`S.Product`: observed -- the lift of c's outputs; integrated -- the partition-function circuit; mixed -- evaluated at K^2
units), never the total minus its own value.  The leaves are `S.leaf_log_m` on the G of each query variable's input fold.

Its yardstick is `S.enumerated_state_log_marginals(plan, tensors, x, v, (Q + I) - v, states)` for every ``v`` in Q.

Comparison rule (`check`): signed cancellation makes a state accurate relative to its row's LARGEST state, not to itself
("Accuracy"), so a state that holds at least ``e^-4`` of its row's largest (`S.MIN_LOG_SHARE`) is compared
on the logarithm with `R.bound`, the others in linear space after the shift by the row's expected maximum,
``|exp(got - max) - exp(want - max)| <= S.EPS``; which state goes where is decided from the fp64 expectation alone, and at most
a quarter of a case's states may take the linear route.
"""
import numpy as np
import torch

import squared_marginal_restatement as R
import squared_sampling_restatement as S
from cirkit_amd.plan import resolve_fold_index
from cirkit_amd.squared_sampling import path_plan


def mask_of(D, *sets):
    m = np.zeros(D, dtype=bool)
    for s in sets:
        m[list(s)] = True
    return m


def down_folds(plan, qvars):
    """The (layer, fold) whose scope meets the query variables."""
    Q = frozenset(int(v) for v in qvars)
    return {(p, f) for p, row in enumerate(R.fold_scopes(plan)) for f, s in enumerate(row) if s & Q}


def output_fold(plan):
    p, f = resolve_fold_index(plan.output, [l.num_folds for l in plan.layers]).reshape(-1, 2)[0]
    return int(p), int(f)


def layer_down(g, wt, others, K, down_slots):
    """One fold of the pass: g (B or 1, Ko, Ko) log values, wt the (Ki, Ko) transposed weights of the two stages (a pair, or
    None: a Hadamard layer), `others` the (B or 1, K^2) values of ALL children in slot order -> {slot: G of that child}."""
    if wt is not None:
        g = R._stage(R._stage(g, wt[0]), wt[1])
    out = {}
    for h in down_slots:
        gc = g
        for h2, v in enumerate(others):
            if h2 != h:
                gc = S._add(gc, v.reshape(-1, K, K))
        out[h] = gc
    return out


def down_gradients(prod, qvars):
    """{(layer, fold): (B or 1, K, K) log G} of every down fold, from the output fold downwards."""
    plan = prod.plan
    down = down_folds(plan, qvars)
    top = output_fold(plan)
    K0 = plan.layers[top[0]].num_output_units
    g0 = torch.full((1, K0, K0), float("-inf"), dtype=prod.c_out[0][0].dtype)
    g0[0, 0, 0] = 0
    G = {top: g0}
    for i in range(len(plan.layers) - 1, -1, -1):
        l = plan.layers[i]
        if l.inputs is None:
            continue
        for f in sorted(f for p, f in down if p == i):
            ch = [(int(p), int(q)) for p, q in prod.children[i][f]]
            wt = None
            if l.type != "hadamard":
                w = prod.weight(i, f).transpose(0, 1)
                wt = (w, w)
            slots = [h for h, c in enumerate(ch) if c in down]
            vals = [prod.value(p, q) if len(slots) > 1 or h not in slots else None for h, (p, q) in enumerate(ch)]
            vals = [torch.zeros((1, l.num_input_units ** 2), dtype=g0.dtype) if v is None else v for v in vals]  # (never read)
            for h, gc in layer_down(G[(i, f)], wt, vals, l.num_input_units, slots).items():
                G[ch[h]] = gc
    return G


def restated_query_log_marginals(plan, tensors, x, qvars, ivars, states, dtype=torch.float64, return_evidence=False):
    """(B, |Q|, C) unnormalised ``log m_b(v, s)`` in `dtype`'s real type, the Q axis in ascending variable order."""
    qvars = sorted(int(v) for v in qvars)
    mask = mask_of(plan.num_variables, qvars, ivars)
    prod = S.Product(plan, tensors, x, mask, dtype)
    G = down_gradients(prod, qvars)
    B = torch.as_tensor(x).shape[0]
    out = torch.stack([S.leaf_log_m(G[path_plan(plan, v).leaf], S.leaf_values(plan, tensors, v, states, dtype)).expand(B, -1)
                       for v in qvars], dim=1)
    if not return_evidence:
        return out
    ev = prod.value(*output_fold(plan))[:, 0]
    return out, (ev.real if ev.is_complex() else ev).expand(B)


def expected_query_log_marginals(plan, tensors, x, qvars, ivars, states):
    """(B, |Q|, C) fp64: the yardstick, one `S.enumerated_state_log_marginals` per query variable."""
    qvars = sorted(int(v) for v in qvars)
    cols = []
    for v in qvars:
        m = mask_of(plan.num_variables, qvars, ivars)
        m[v] = False
        cols.append(S.enumerated_state_log_marginals(plan, tensors, x, v, m, states))
    return torch.stack(cols, dim=1)


def check(got, want, what="", factor=1.0, route=None, min_log_share=S.MIN_LOG_SHARE):
    """The comparison rule of the module docstring on (..., C) tables; prints and returns (worst error of the log route as a
    fraction of `factor` x `R.bound`, worst linear error, states on the linear route, states).  `route`: the fp64 expectation
    that decides which states are compared how, where `want` is itself a result under test (an identity between two results).
    `min_log_share` = -inf holds EVERY state to the bound on its logarithm (the Categorical fixture: a circuit without signed
    cancellation, where 27 % of the states lie below e^-4 of their row's largest -- more than the linear route may take -- and
    none needs it)."""
    got = torch.as_tensor(got).detach().cpu().double().numpy()
    want = np.asarray(torch.as_tensor(want).detach().cpu().double().numpy())
    assert got.shape == want.shape, (got.shape, want.shape)
    fin = np.isfinite(want)
    assert bool((got[~fin] == want[~fin]).all()), f"{what}: where the expected value is not finite"
    with np.errstate(all="ignore"):
        mx = np.where(fin, want, -np.inf).max(axis=-1, keepdims=True)
        mx = np.where(np.isfinite(mx), mx, 0.0)
        ref = want if route is None else np.asarray(route, dtype=np.float64)
        rmx = np.where(np.isfinite(ref), ref, -np.inf).max(axis=-1, keepdims=True)
        by_log = fin & (ref - np.where(np.isfinite(rmx), rmx, 0.0) >= min_log_share)
        by_lin = fin & ~by_log
        log_err = np.abs(got - want) / (factor * R.bound(want))
        lin_err = np.abs(np.exp(got - mx) - np.exp(want - mx))
    worst_log = float(log_err[by_log].max()) if by_log.any() else 0.0
    worst_lin = float(lin_err[by_lin].max()) if by_lin.any() else 0.0
    print(f"{what}: worst error {worst_log:.3f} of the bound; {int(by_lin.sum())} of {int(fin.sum())} states below e^{S.MIN_LOG_SHARE:g} "
          f"of their row's largest, worst linear error {worst_lin:.1e}")
    assert 4 * int(by_lin.sum()) <= int(fin.sum()), f"{what}: more than a quarter of the states take the linear route"
    assert not np.isnan(got[fin]).any(), f"{what}: NaN"
    assert worst_log <= 1.0, f"{what}: {worst_log} of the bound on the logarithm"
    assert worst_lin <= factor * S.EPS, f"{what}: linear error {worst_lin}"
    return worst_log, worst_lin, int(by_lin.sum()), int(fin.sum())


# ---- the cases the CPU and the GPU tests share ------------------------------------------------------------------------------
TINY_QUERIES = [(list(range(6)), []), ([0, 1, 4], [2]), ([3], [])]
EMB32_QUERIES = [(list(range(16)), []), (list(range(8, 16)), []), ([1, 6, 11, 12], [3, 9])]
CAT_QUERY = ([0, 6, 15], [1, 4])
GOLDEN = "sq_posterior_expected.npz"


def tiny_rows():
    return R.rows_of(6, 3, 5, seed=S.TINY_ROWS_SEED)


def emb32_rows():
    return R.rows_of(16, 3, 33, 1)


def cat_rows():
    return torch.from_numpy(np.random.default_rng(S.CAT_ROWS_SEED).integers(0, 256, size=(3, 16)))


def emb32_expected(i):
    plan, tensors, states = R.emb32_case()
    return expected_query_log_marginals(plan, tensors, emb32_rows(), *EMB32_QUERIES[i], states).numpy()


def cat_expected():
    """Four 256-state pixels are integrated for every query variable: past enumeration, the fp64 restatement of the one-variable
    query (`R.yardstick` inside `S.enumerated_state_log_marginals`), which the CPU tests pin to the enumeration."""
    plan, tensors, states = R.cat_case()
    return expected_query_log_marginals(plan, tensors, cat_rows(), *CAT_QUERY, states).numpy()


def golden():
    import os

    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)) as z:
        return {k: z[k] for k in z.files}


# ---- hand-built layers for the kernels alone ----------------------------------------------------------------------------------
KIND_FULL, KIND_CONST, KIND_RANK1 = S.KIND_FULL, S.KIND_CONST, S.KIND_RANK1
LAYER_STATES = 7
LAYER_FOLDS = 2  # folds per launch; fold j reads weight fold j + 1 of 4
LAYER_SHAPES = {  # name -> (stages, Ki, Ko, the folds are output folds, [(the child is a down fold, kind of its value)])
    "stage32": (1, 32, 32, False, [(True, KIND_FULL)]),
    "root32": (1, 32, 1, True, [(True, KIND_CONST)]),
    "hadamard2": (0, 32, 32, False, [(True, KIND_FULL), (True, KIND_RANK1)]),
    "hadamard3": (0, 3, 3, False, [(False, KIND_CONST), (True, KIND_FULL), (False, KIND_RANK1)]),
    "generic33": (1, 3, 3, False, [(True, KIND_RANK1), (False, KIND_FULL)]),
    "generic52": (1, 5, 2, True, [(True, KIND_CONST)]),
}


def _hand_layer(cplx, shape, B, seed):
    st, Ki, Ko, top, slots = LAYER_SHAPES[shape]
    g = torch.Generator().manual_seed(seed)

    def signs(*sh):  # one entry in ten negative, as `S.hand_path_case`
        return torch.where(torch.rand(*sh, generator=g) < 0.1, -1.0, 1.0).double()

    def values(*sh):
        re = torch.randn(*sh, generator=g, dtype=torch.float64)
        if not cplx:
            return re
        flip = (signs(*sh) < 0).double() * np.pi
        return torch.complex(re, flip + 0.1 * torch.randn(*sh, generator=g, dtype=torch.float64))

    def neg_inf(n):
        return torch.complex(torch.full((n,), -np.inf, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)) if cplx else \
            torch.full((n,), -np.inf, dtype=torch.float64)

    w = None
    if st:
        w = torch.randn(2, 4, Ko, Ki, generator=g, dtype=torch.float64).abs() + 0.05  # (stage, weight fold, Ko, Ki)
        if cplx:
            w = w * signs(2, 4, Ko, Ki)
        w[:, :, :, Ki - 1] = 0.0  # a weight column of 0: a -inf row and column of dP
    folds = []
    for j in range(LAYER_FOLDS):
        gin = None
        if not top:
            gin = values(B, Ko * Ko)
            if B > 1:
                gin[B - 1] = neg_inf(Ko * Ko)  # the last row: an all -inf G, so every child's G and every state -inf (not NaN)
        kids = []
        for dn, kd in slots:
            raw = values(1 if kd == KIND_CONST else B, Ki if kd == KIND_RANK1 else Ki * Ki)
            kids.append((dn, kd, raw, S._lift(raw) if kd == KIND_RANK1 else raw))
        folds.append((gin, kids))
    tlog = 1 if B == 3 else 0
    table = torch.randn(LAYER_FOLDS * len(slots), LAYER_STATES + 1, Ki, generator=g, dtype=torch.float64)  # one per (fold, slot)
    if not tlog:
        table = (table.abs() + 0.05) * (signs(*table.shape) if cplx else 1.0)
    return dict(stages=st, Ki=Ki, Ko=Ko, top=top, w=w, folds=folds, table=table, tlog=tlog)


def _hand_layer_run(case, cplx, dtype):
    """Per fold {slot: G of the down child} and per (fold, down slot) its ``log m`` (B, C), in `dtype`."""
    cdt = (torch.complex128 if dtype == torch.float64 else torch.complex64) if cplx else dtype
    Ki, Ko = case["Ki"], case["Ko"]
    nslots = len(case["folds"][0][1])
    Gs, lms = [], {}
    for j, (gin, kids) in enumerate(case["folds"]):
        if gin is None:
            g = torch.full((1, Ko, Ko), -np.inf, dtype=cdt)
            g[0, 0, 0] = 0
        else:
            g = gin.to(cdt).reshape(-1, Ko, Ko)
        wt = None
        if case["stages"]:
            wt = (case["w"][0, j + 1].transpose(0, 1).to(dtype), case["w"][1, j + 1].transpose(0, 1).to(dtype))
        out = layer_down(g, wt, [v.to(cdt) for _, _, _, v in kids], Ki, [h for h, k in enumerate(kids) if k[0]])
        Gs.append(out)
        for h, gc in out.items():
            t = case["table"][j * nslots + h, :LAYER_STATES]
            a = (torch.exp(t) if case["tlog"] else t).to(dtype)
            lms[(j, h)] = S.leaf_log_m(gc, a.to(cdt))
    return Gs, lms


def hand_layer_case(cplx, shape, B):
    """A hand-built layer for `ck_squared_down_bwd` and `ck_squared_down_leaf` alone: the case, the G of every down child and
    its ``log m`` in fp64 and the ``log m`` in fp32.  Data as `S.hand_path_case` chooses them: the first seed from 31 + B on at
    which every state of every live row holds at least e^-4 of its row's largest."""
    for seed in range(31 + B, 31 + B + 50):
        case = _hand_layer(cplx, shape, B, seed)
        Gs, lms = _hand_layer_run(case, cplx, torch.float64)
        ok = True
        for lm in lms.values():
            lm = lm.expand(B, -1)
            live = torch.isfinite(lm).any(dim=1)
            dead = 1 if B > 1 and not case["top"] else 0
            ok = ok and int((~live).sum()) == dead and bool(torch.isfinite(lm[live]).all()) and \
                float(S.log_share(lm[live].numpy()).min()) >= S.MIN_LOG_SHARE
        if ok:
            return case, Gs, lms, _hand_layer_run(case, cplx, torch.float32)[1], seed
    raise AssertionError("no seed gives states above the share")


if __name__ == "__main__":
    import os

    rec = {f"emb32_want_{i}": emb32_expected(i) for i in range(len(EMB32_QUERIES))}
    rec["cat_want"] = cat_expected()
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN), **rec)
