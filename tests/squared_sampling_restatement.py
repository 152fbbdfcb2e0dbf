"""Sampling and all-state conditionals of a squared circuit (cirkit_amd/squared_sampling.py, csrc/ck_sqpath.hip) restated in
torch / numpy on the host, in the dtype they are given.

`restated_state_log_marginals` is the ALGORITHM: the derivative G of the root of the product circuit with respect to the K^2
squared units of the input fold of one variable v, walked from the root down the ancestors of v -- at a sum / CP-T fold the two
TensorDot stages with the weight matrix transposed (dP = W^T G W), plus the values of the fold's other children (observed: the
lift of c's outputs; integrated: the partition-function circuit; mixed: evaluated at K^2 units as
squared_marginal_restatement does) -- and the leaf form ``m_b(s) = Re sum_kl exp(G[k, l]) a_k(s) conj(a_l(s))``, shifted by the
maximum real part of G and clamped at 0 before the logarithm.  Its yardstick is `R.enumerated_log_marginal` on the row with
``x_v = s``.

`restated_sampler` draws one variable after the other from those marginals with the numpy Philox of sampling_restatement.py:
counter (row, global fold id of the variable's input fold, 0, 0), key the two halves of the seed, ``u = (x0 >> 8) 2^-24``, the
draw the smallest ``s`` with ``u T < CDF_s`` over the weights ``exp(log m - max)``.

Near-boundary draws.  The GPU sampler works in fp32, so a draw whose ``u`` falls next to a boundary of its bin can land in the
neighbouring state.  The worst deviation of the fp32-restated normalised CDF from the fp64 one over every step of the cases of
tests/test_squared_sampling.py (measured by tests/test_squared_sampling_restatement.py, which asserts it) is
``EPS = 4e-5`` (measured: 2.8e-5 in the default order, 3.1e-5 in raster order, 2.2e-5 with half the pixels observed); a draw is
NEAR when ``u`` lies within ``4 EPS`` of a boundary of the bin the fp64 run chose (4 x: the kernel reduces in another shape), a
row is near when any of its draws is.  With the seeds of the tests the fp64 run flags at most 2 % of the rows (tests/test_squared_sampling_restatement.py prints the shares).
"""
import numpy as np
import torch

import squared_marginal_restatement as R
from cirkit_amd.functional import squared_partition_plan
from cirkit_amd.plan import resolve_fold_index
from cirkit_amd.squared_sampling import path_plan, tree_order
from sampling_restatement import philox4x32_10, uniform

EPS = 4e-5  # bound on |CDF_fp32 - CDF_fp64| (asserted on the host); NEAR = within 4 EPS of a bin boundary


_CONSTANTS = {}  # (id(plan), id(tensors), dtype) -> (plan, tensors -- kept alive --, cast tensors, z_of, outputs of the Z circuit)


class Product:
    """The values of the folds of the product circuit for one batch and one integrated set, by class (the machinery of
    `R.restated_log_marginal`, with the value of ANY fold on request)."""

    def __init__(self, plan, tensors, x, mask, dtype=torch.float64):
        from oracle.torch_oracle import eval_param, evaluate_plan

        self.plan, self.mask = plan, np.asarray(mask, dtype=bool)
        key = (id(plan), id(tensors), dtype)
        if key not in _CONSTANTS:  # (what does not depend on the rows: evaluated once per case and dtype)
            tt = R._cast(tensors, dtype)
            z_plan, z_of = squared_partition_plan(plan, return_layer_map=True)
            _CONSTANTS[key] = (plan, tensors, tt, z_of, evaluate_plan(z_plan, tt, None, return_all=True)[1])
        _, _, self.tt, self.z_of, self.z_out = _CONSTANTS[key]
        x = torch.as_tensor(x).clone()
        x[:, torch.from_numpy(self.mask)] = 0
        _, self.c_out = evaluate_plan(plan, self.tt, x, return_all=True)
        self.cls = R.classes_from_scopes(plan, self.mask)
        self.folds = [l.num_folds for l in plan.layers]
        self.children = [None if l.inputs is None else resolve_fold_index(l.inputs, self.folds) for l in plan.layers]
        self.conj = plan.semiring == "complex-lse-sum"
        self.full = {}
        self._eval_param = eval_param

    def weight(self, layer, fold):
        return self._eval_param(self.plan.layers[layer].params["weight"], self.tt)[fold]

    def value(self, p, f):
        """(B or 1, K^2) log values of fold f of layer p of the product circuit."""
        if self.cls[p][f] == R.INTEGRATED:
            return self.z_out[self.z_of[p]][f]
        if self.cls[p][f] == R.OBSERVED:
            y = self.c_out[p][f]
            return (y[:, :, None] + (y.conj() if self.conj else y)[:, None, :]).flatten(1)
        if (p, f) not in self.full:
            l = self.plan.layers[p]
            v = sum(self.value(int(q), int(g)) for q, g in self.children[p][f])
            if l.type != "hadamard":
                K = l.num_input_units
                w = self.weight(p, f)
                v = R._stage(R._stage(v.reshape(-1, K, K), w), w).flatten(1)
            self.full[(p, f)] = v
        return self.full[(p, f)]


def leaf_values(plan, tensors, v, states, dtype):
    """(C, K): the linear value of every unit of the input fold of variable v at every state."""
    from oracle.torch_oracle import evaluate_plan

    pp = path_plan(plan, v)
    rows = torch.zeros((states, plan.num_variables), dtype=torch.int64)
    rows[:, v] = torch.arange(states)
    _, outs = evaluate_plan(plan, R._cast(tensors, dtype), rows, return_all=True)
    return torch.exp(outs[pp.leaf[0]][pp.leaf[1]])


def path_gradient(prod, pp):
    """(B, K, K) log values: the derivative of the root (unit 0 of the output fold) with respect to the K^2 squared units of
    the input fold at the end of the path `pp`."""
    plan = prod.plan
    top = plan.layers[pp.levels[0].layer] if pp.levels else plan.layers[pp.leaf[0]]
    K0 = top.num_output_units
    some = prod.c_out[0][0]
    cdt = some.dtype
    G = torch.full((1, K0, K0), float("-inf"), dtype=cdt)
    G[0, 0, 0] = 0
    for lv in pp.levels:
        l = plan.layers[lv.layer]
        if l.type != "hadamard":
            wt = prod.weight(lv.layer, lv.fold).transpose(0, 1)  # (Ki, Ko): the stages of the way up, transposed
            G = R._stage(R._stage(G, wt), wt)
        K = l.num_input_units
        for p, g in lv.siblings:
            G = G + prod.value(p, g).reshape(-1, K, K)
    return G


def leaf_log_m(G, a):
    """(B, C): log max(0, Re sum_kl exp(G[k, l] - gmax) a_k(s) conj(a_l(s))) + gmax."""
    re = G.real if G.is_complex() else G
    fi = torch.finfo(re.dtype)
    gmax = torch.clamp(re.amax(dim=(1, 2), keepdim=True), min=fi.min, max=fi.max)
    if G.is_complex():  # (by parts: torch's complex exp of -inf + i y is NaN on some code paths, and it is 0)
        mag = torch.exp(G.real - gmax)
        E = torch.complex(mag * torch.cos(G.imag), mag * torch.sin(G.imag))
    else:
        E = torch.exp(G - gmax)
    val = torch.einsum("bkl,sk,sl->bs", E, a.to(E.dtype), a.conj().to(E.dtype))
    val = val.real if val.is_complex() else val
    val = torch.where(val < 0, torch.zeros((), dtype=val.dtype), val)
    return torch.log(val) + gmax[:, :, 0]


def restated_state_log_marginals(plan, tensors, x, v, mask, states, dtype=torch.float64):
    """(B, C) unnormalised ``log m_b(s)`` in `dtype`'s real type; `mask`: the integrated variables, without v."""
    mask = np.asarray(mask, dtype=bool).copy()
    assert not mask[v]
    mask[v] = True
    prod = Product(plan, tensors, x, mask, dtype)
    G = path_gradient(prod, path_plan(plan, v))
    lm = leaf_log_m(G, leaf_values(plan, tensors, v, states, dtype))
    return lm.expand(torch.as_tensor(x).shape[0], -1)


def enumerated_state_log_marginals(plan, tensors, x, v, mask, states):
    """(B, C) fp64: the yardstick, `R.enumerated_log_marginal` on the rows with x_v = s."""
    cols = []
    for s in range(states):
        xs = torch.as_tensor(x).clone()
        xs[:, v] = s
        cols.append(R.yardstick(plan, tensors, xs, mask, states))
    return torch.stack(cols, dim=1)


def global_fold_id(plan, layer, fold):
    return int(sum(l.num_folds for l in plan.layers[:layer])) + int(fold)


def draw(lm, u):
    """The draw from ``log m`` (B, C) numpy at the uniforms u (B,), in lm's dtype: state (-1: no mass or a NaN) and the
    normalised CDF (B, C)."""
    with np.errstate(all="ignore"):
        mx = np.clip(np.nanmax(np.where(np.isnan(lm), -np.inf, lm), axis=1, keepdims=True), np.finfo(lm.dtype).min, np.finfo(lm.dtype).max)
        w = np.exp(lm - mx)
        cum = np.cumsum(w, axis=1, dtype=lm.dtype)
        tot = cum[:, -1]
        target = u.astype(lm.dtype) * tot
        hit = cum > target[:, None]
        state = np.where(hit.any(axis=1), hit.argmax(axis=1), (w.shape[1] - 1) - (w[:, ::-1] > 0).argmax(axis=1))
        ok = (tot > 0) & np.isfinite(tot)
        return np.where(ok, state, -1), cum / tot[:, None]


def restated_sampler(plan, tensors, x, drawn, states, seed, order=None, dtype=torch.float64, compare=None, row0=0):
    """The autoregressive sampler on the host.  x (B, D) int64, `drawn` (D,) bool: the variables to draw (entries of x there
    are ignored), in `order` (default: `tree_order` restricted to them).  Returns the completed rows, per row the smallest
    distance of a draw's u to a boundary of its bin (normalised CDF, decision boundaries only), and -- with `compare` a
    second dtype -- the worst deviation of that dtype's normalised CDF from this one's on the same evidence."""
    drawn = np.asarray(drawn, dtype=bool)
    order = [v for v in tree_order(plan) if drawn[v]] if order is None else list(order)
    x = torch.as_tensor(x).clone()
    B = x.shape[0]
    x[:, torch.from_numpy(drawn)] = 0
    left = drawn.copy()
    margin = np.full(B, np.inf)
    dead = np.zeros(B, dtype=bool)
    worst = 0.0
    n = np.arange(B, dtype=np.uint64) + np.uint64(row0)
    for v in order:
        left[v] = False
        pp = path_plan(plan, v)
        u = uniform(philox4x32_10(n, global_fold_id(plan, *pp.leaf), 0, 0, seed & 0xFFFFFFFF, seed >> 32)[0])
        lm = restated_state_log_marginals(plan, tensors, x, v, left, states, dtype).numpy()
        state, cdf = draw(lm, u)
        dead |= state < 0
        lo = np.where(state > 0, np.take_along_axis(cdf, np.maximum(state - 1, 0)[:, None], 1)[:, 0], -np.inf)
        hi = np.where(state < states - 1, np.take_along_axis(cdf, np.maximum(state, 0)[:, None], 1)[:, 0], np.inf)
        margin = np.minimum(margin, np.minimum(u - lo, hi - u))
        if compare is not None:
            lm2 = restated_state_log_marginals(plan, tensors, x, v, left, states, compare).numpy()
            worst = max(worst, float(np.abs(draw(lm2, u)[1].astype(np.float64) - cdf).max()))
        x[:, v] = torch.from_numpy(np.where(dead, 0, state))
    out = x.clone()
    out[torch.from_numpy(dead)[:, None] & torch.from_numpy(drawn)[None, :]] = -1
    return out, margin, worst


def near_rows(margin):
    return margin < 4 * EPS


def world_codes(rows, states):
    rows = np.asarray(rows, dtype=np.int64)
    return rows @ (states ** np.arange(rows.shape[1])[::-1])


# ---- the cases the CPU and the GPU tests share ------------------------------------------------------------------------------
TINY_ROWS_SEED = 3  # (`R.rows_of(6, 3, 5, seed=...)`: with seeds 1, 2 and 4 some state of some row is a cancelled sum near e^-20,
#                      where fp32 leaves 0.3 .. 1.8 of the bound; with 3 the worst over ALL (v, mask) is 0.11 of it)


def tiny_queries():
    """Every variable of the 6 with 8 of the 32 masks of the other five."""
    out = []
    for v in range(6):
        others = [w for w in range(6) if w != v]
        for j in range(v % 4, 32, 4):
            m = np.zeros(6, dtype=bool)
            m[[w for k, w in enumerate(others) if (j >> k) & 1]] = True
            out.append((v, m))
    return out


def emb32_queries():
    """v = 0, 5, 15 with the masks of `R.masks_4x4` that leave v out."""
    return [(v, m) for v in (0, 5, 15) for m in R.masks_4x4() if not m[v]]


def cat_queries():
    """Three variables of the Categorical fixture (256 states); nothing, one pixel and five pixels integrated -- two 256-state
    pixels times 256 states of v are too many worlds to enumerate in a test, five take the fp64 restatement (`R.yardstick`)."""
    out = []
    for v, one, five in ((0, [1], [1, 4, 5, 10, 15]), (6, [7], [2, 3, 7, 9, 12]), (15, [0], [0, 11, 12, 13, 14])):
        for ids in ([], one, five):
            m = np.zeros(16, dtype=bool)
            m[ids] = True
            out.append((v, m))
    return out


CAT_ROWS_SEED = 2  # (the rows of tests/test_squared_marginals.py::test_real_circuit_under_lse_sum)
DRAW_ROWS = 2048
RASTER = list(range(16))


def draw_cases():
    """name -> (x (B, 16), drawn (16,) bool, order or None, seed) on `R.emb32_case`: every pixel drawn in the default order,
    in raster order (which makes mixed siblings), and a random half of the pixels observed."""
    rng = np.random.default_rng(17)
    half = np.zeros(16, dtype=bool)
    half[rng.choice(16, size=8, replace=False)] = True
    every = np.ones(16, dtype=bool)
    zeros = torch.zeros((DRAW_ROWS, 16), dtype=torch.int64)
    return {"default": (zeros, every, None, 20250101), "raster": (zeros, every, RASTER, 20250102),
            "conditional": (R.rows_of(16, 3, DRAW_ROWS, seed=23), half, None, 20250103)}


# ---- recorded expectations (tests/golden/sq_sampling_expected.npz) ---------------------------------------------------------------
# What takes the host minutes -- the enumerations of the 32-unit and the Categorical cases, the fp64 restated sampler on 2048
# rows -- is recorded once by `PYTHONPATH=. python tests/squared_sampling_restatement.py`; tests/test_squared_sampling_restatement.py
# recomputes it and compares, the GPU tests read it.
GOLDEN = "sq_sampling_expected.npz"
EMB32_POOL = (200, 1)  # `R.rows_of(16, 3, *EMB32_POOL)`: the rows the 33 of the 32-unit case are chosen from
MIN_LOG_SHARE = -4.0


def log_share(want):
    """(B,) the smallest log share of a state in its row's largest state, over (B, C) expected values."""
    want = np.asarray(want)
    return (want - want.max(axis=1, keepdims=True)).min(axis=1)


def golden():
    import os

    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)) as z:
        return {k: z[k] for k in z.files}


def emb32_rows_and_expected():
    """The 33 rows of the 32-unit case and their enumerated ``log m`` per query of `emb32_queries`.

    ``m_b(s)`` is a quadratic form of K^2 signed terms whose weights exp(G) carry the rounding of G's log-space stages, about
    1e-6 relative each, so fp32 leaves an error of about 1e-5 of the row's LARGEST state in every state.  A state that holds
    e^-g of the largest therefore has a relative error of about e^g 1e-5, while the bound on its logarithm is 1e-4 |log m|
    (about 2.5e-3 here) and the fp32 restatement has to stay below a quarter of that: g <= 4.  So the rows are the first 33 of
    the pool in which every state of every query holds at least e^-4 of its row's largest (measured on the pool: no state
    above e^-4 exceeds a quarter of the bound in fp32, a third of those below e^-6 do; DESIGN.md says what this means for
    a caller).  The sampler's tests take rows as they come."""
    plan, tensors, states = R.emb32_case()
    pool = R.rows_of(16, states, *EMB32_POOL)
    want = [enumerated_state_log_marginals(plan, tensors, pool, v, m, states).numpy() for v, m in emb32_queries()]
    ok = np.min([log_share(w) for w in want], axis=0) >= MIN_LOG_SHARE
    keep = np.nonzero(ok)[0][:33]
    assert len(keep) == 33
    return pool[keep].numpy(), np.stack([w[keep] for w in want])


def cat_expected():
    plan, tensors, states = R.cat_case()
    x = torch.from_numpy(np.random.default_rng(CAT_ROWS_SEED).integers(0, states, size=(3, 16)))
    return np.stack([enumerated_state_log_marginals(plan, tensors, x, v, m, states).numpy() for v, m in cat_queries()])


def draw_expected(name, compare=None):
    plan, tensors, states = R.emb32_case()
    x, drawn, order, seed = draw_cases()[name]
    out, margin, worst = restated_sampler(plan, tensors, x, drawn, states, seed, order=order, compare=compare)
    return out.numpy().astype(np.int8), margin, worst


if __name__ == "__main__":
    import os

    rec = {}
    rec["emb32_x"], rec["emb32_want"] = emb32_rows_and_expected()
    rec["cat_want"] = cat_expected()
    for name in draw_cases():
        rec[f"draw_{name}_out"], rec[f"draw_{name}_margin"], _ = draw_expected(name)
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN), **rec)


# ---- hand-built paths for the kernel alone ------------------------------------------------------------------------------------
PATH_SHAPES = {  # name -> ([(stages, Ki, Ko, siblings)] root first, K of the leaf)
    "all32": ([(1, 32, 32, 1), (1, 32, 32, 1)], 32),
    "root": ([(1, 32, 1, 1), (1, 32, 32, 2)], 32),
    "generic33": ([(1, 3, 3, 1), (1, 3, 3, 1)], 3),
    "generic52": ([(1, 5, 2, 1)], 5),
    "hadamard": ([(1, 32, 1, 0), (0, 32, 32, 2)], 32),
    "hadamard3": ([(1, 3, 1, 1), (0, 3, 3, 2)], 3),
}
PATH_STATES = 7
KIND_FULL, KIND_CONST, KIND_RANK1 = 0, 1, 2  # (CK_SQ_*)


def _add(a, b):
    """a + b in log space by parts (torch's complex sum of two -inf leaves a NaN imaginary part)."""
    return torch.complex(a.real + b.real, a.imag + b.imag) if a.is_complex() else a + b


def _lift(y):
    if y.is_complex():
        return torch.complex(y.real[:, :, None] + y.real[:, None, :], y.imag[:, :, None] - y.imag[:, None, :]).flatten(1)
    return (y[:, :, None] + y[:, None, :]).flatten(1)


def _hand_path(cplx, shape, B, seed):
    levels, K = PATH_SHAPES[shape]
    C = PATH_STATES
    g = torch.Generator().manual_seed(seed)

    def signs(*sh):  # one entry in ten negative: the complex kernels see both phases, the sums stay far from cancelling
        return torch.where(torch.rand(*sh, generator=g) < 0.1, -1.0, 1.0).double()

    def values(*sh):
        re = torch.randn(*sh, generator=g, dtype=torch.float64)
        if not cplx:
            return re
        flip = (signs(*sh) < 0).double() * np.pi
        return torch.complex(re, flip + 0.1 * torch.randn(*sh, generator=g, dtype=torch.float64))

    out, turn = [], 0
    for li, (st, Ki, Ko, n) in enumerate(levels):
        w = None
        if st:
            w = torch.randn(2, 3, Ko, Ki, generator=g, dtype=torch.float64).abs() + 0.05  # (stage, fold, Ko, Ki); fold 1 is read
            if cplx:
                w = w * signs(2, 3, Ko, Ki)
            if li == len(levels) - 1 or not levels[li + 1][0]:
                w[:, :, :, Ki - 1] = 0.0  # a weight column of 0: a -inf row and column of dP
        sibs = []
        for _ in range(n):
            kd = (KIND_FULL, KIND_CONST, KIND_RANK1)[turn % 3]
            turn += 1
            if kd == KIND_FULL:
                raw = values(B, Ki * Ki)
                v = raw
            elif kd == KIND_CONST:
                raw = values(1, Ki * Ki)
                v = raw
            else:
                raw = values(B, Ki)
                if B > 1:  # the last row: an all -inf child, so a gradient and every state of -inf (not NaN)
                    raw[B - 1] = torch.complex(torch.full((Ki,), -np.inf, dtype=torch.float64), torch.zeros(Ki, dtype=torch.float64)) if cplx else -np.inf
                v = _lift(raw)
            sibs.append((kd, raw, v))
        out.append((st, Ki, Ko, w, sibs))
    tlog = 1 if B == 3 else 0  # (a table of logarithms, as a Categorical layer keeps it; else linear values)
    table = torch.randn(2, C + 1, K, generator=g, dtype=torch.float64)  # (fold, state, unit); fold 1 is read
    if not tlog:
        table = (table.abs() + 0.05) * (signs(2, C + 1, K) if cplx else 1.0)
    return out, table, tlog


def _hand_path_log_m(case, cplx, dtype):
    lv, table, tlog = case
    cdt = (torch.complex128 if dtype == torch.float64 else torch.complex64) if cplx else dtype
    K0 = lv[0][2]
    G = torch.full((1, K0, K0), -np.inf, dtype=cdt)
    G[0, 0, 0] = 0
    for st, Ki, Ko, w, sibs in lv:
        if st:
            G = R._stage(R._stage(G, w[0, 1].transpose(0, 1).to(dtype)), w[1, 1].transpose(0, 1).to(dtype))
        for _, _, v in sibs:
            G = _add(G, v.to(cdt).reshape(-1, Ki, Ki))
    a = (torch.exp(table[1, :PATH_STATES]) if tlog else table[1, :PATH_STATES]).to(dtype)
    return leaf_log_m(G, a.to(cdt))


def hand_path_case(cplx, shape, B):
    """A hand-built path for `ck_squared_path_bwd` alone: ([(stages, Ki, Ko, weights, [(kind, stored values, K^2 values)])],
    table, table_log), its ``log m`` (B, C) in fp64 and in fp32.  The siblings take the three kinds in turn.  Data with
    mostly aligned phases (one weight, value and table entry in ten is negative) and the first seed from 11 + B on at which
    every state of every row but the all -inf one holds at least e^-4 of its row's largest: the states the bound on the logarithm can be
    asked of (`emb32_rows_and_expected`)."""
    for seed in range(11 + B, 11 + B + 50):
        case = _hand_path(cplx, shape, B, seed)
        want = _hand_path_log_m(case, cplx, torch.float64)
        if want.shape[0] != B:
            want = want.expand(B, -1)
        live = torch.isfinite(want).any(dim=1)
        dead = 1 if B > 1 and any(kd == KIND_RANK1 for lv in case[0] for kd, _, _ in lv[4]) else 0  # (only the all -inf row)
        if int((~live).sum()) == dead and bool(torch.isfinite(want[live]).all()) and float(log_share(want[live].numpy()).min()) >= MIN_LOG_SHARE:
            want32 = _hand_path_log_m(case, cplx, torch.float32).expand(B, -1)
            return case, want, want32, seed
    raise AssertionError("no seed gives states above the share")
