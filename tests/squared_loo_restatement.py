"""Leave-one-out conditionals of a squared circuit (cirkit_amd/squared_loo.py, csrc/ck_sqloo.hip) restated in torch on the host, in
the dtype they are given.

`restated_loo_log_marginals` is the ALGORITHM: one derivative pass over c ITSELF that carries ``D = log dc/du`` for the K units of
every fold whose scope holds a query variable (the down folds, here from explicit scope sets).  From the output fold (log 1 at unit
0) downwards, a fold with weights turns D into ``P_i = log sum_k W[k, i] exp(D_k)`` -- shifted by the row's largest real part, the
complex exponential taken by parts (`S.leaf_log_m` says why), summed in linear space on the REAL part (real parameters: every
argument is a multiple of pi), argument pi where the sum is negative, -inf where it is exactly 0 -- a Hadamard fold passes D on, and
every child that is a down fold receives P plus the VALUES of the other children in slot order, never the total minus its own
value.  The leaf of variable v is ``log m(s) = 2 (log |sum_k Re exp(D_k - m) a_k(s)| + m)``.

Its yardstick is `S.enumerated_state_log_marginals(plan, tensors, x, v, empty mask, states)`: oracle forwards of the rows with
``x_v = s``.  The comparison is `squared_down_restatement.check`; `check_entries` is the same rule for the per-entry conditionals
``log p(x_v | x_-v)``, where an entry's share is its own probability.
"""
import functools

import numpy as np
import torch

import squared_down_restatement as P
import squared_marginal_restatement as R
import squared_sampling_restatement as S
from cirkit_amd.plan import resolve_fold_index
from cirkit_amd.squared_sampling import path_plan


def _re(v):
    return v.real if v.is_complex() else v


def lin(d, m):
    """The real part of exp(d - m), by parts."""
    if d.is_complex():
        return torch.exp(d.real - m) * torch.cos(d.imag)
    return torch.exp(d - m)


def shift_of(d):
    """(B, 1): the clamped largest real part of each row."""
    re = _re(d)
    fi = torch.finfo(re.dtype)
    return torch.clamp(re.amax(dim=1, keepdim=True), min=fi.min, max=fi.max)


def signed_log(y, m, cplx):
    """log of the real linear values y plus the shift m, as the pass carries it."""
    mag = torch.where(y == 0, torch.full_like(y, -np.inf), torch.log(y.abs()) + m)
    if not cplx:
        return torch.where(y < 0, torch.full_like(y, np.nan), mag)
    return torch.complex(mag, torch.where(y < 0, torch.full_like(y, np.pi), torch.zeros_like(y)))


def layer_down(d, w, values, down_slots):
    """One fold of the pass: d (B or 1, Ko) signed logarithms, w the real (Ko, Ki) weights or None (a Hadamard fold), `values` the
    (B, Ki) values of ALL children in slot order -> {slot: D of that child}."""
    if w is not None:
        m = shift_of(d)
        d = signed_log(lin(d, m) @ w.to(_re(d).dtype), m, d.is_complex())
    out = {}
    for h in down_slots:
        dc = d
        for h2, v in enumerate(values):
            if h2 != h:
                dc = dc + v
        out[h] = dc
    return out


def leaf_log_m(d, a):
    """(B, C): 2 (log |sum_k Re exp(d_k - m) a_k(s)| + m), -inf where the sum is 0; a (C, K) real linear values."""
    m = shift_of(d)
    A = lin(d, m) @ _re(a).to(_re(d).dtype).T
    return torch.where(A == 0, torch.full_like(A, -np.inf), 2 * (torch.log(A.abs()) + m))


def derivatives(plan, tensors, x, qvars, dtype):
    """{(layer, fold): (B, K) log dc/du} of every down fold, from the output fold downwards, and the launch order."""
    from oracle.torch_oracle import eval_param, evaluate_plan

    tt = R._cast(tensors, dtype)
    _, c_out = evaluate_plan(plan, tt, torch.as_tensor(x), return_all=True)
    folds = [l.num_folds for l in plan.layers]
    children = [None if l.inputs is None else resolve_fold_index(l.inputs, folds) for l in plan.layers]
    down = P.down_folds(plan, qvars)
    top = P.output_fold(plan)
    K0 = plan.layers[top[0]].num_output_units
    d0 = torch.full((1, K0), -np.inf, dtype=c_out[0][0].dtype)
    d0[0, 0] = 0
    D, order = {top: d0}, []
    for i in range(len(plan.layers) - 1, -1, -1):
        l = plan.layers[i]
        fs = sorted(f for p, f in down if p == i)
        if l.inputs is None or not fs:
            continue
        order.append((i, fs))
        w = eval_param(l.params["weight"], tt) if l.type != "hadamard" else None
        for f in fs:
            ch = [(int(p), int(g)) for p, g in children[i][f]]
            got = layer_down(D[(i, f)], None if w is None else w[f], [c_out[p][g] for p, g in ch], [h for h, c in enumerate(ch) if c in down])
            for h, dc in got.items():
                assert ch[h] not in D, "a fold with two readers: not a tree"
                D[ch[h]] = dc
    return D, order


def restated_loo_log_marginals(plan, tensors, x, qvars, states, dtype=torch.float64):
    """(B, |Q|, C) unnormalised ``log |c(x_-v, s)|^2`` in `dtype`'s real type, the Q axis in ascending variable order."""
    qvars = sorted(int(v) for v in qvars)
    D, _ = derivatives(plan, tensors, x, qvars, dtype)
    B = torch.as_tensor(x).shape[0]
    return torch.stack([leaf_log_m(D[path_plan(plan, v).leaf], S.leaf_values(plan, tensors, v, states, dtype)).expand(B, -1)
                        for v in qvars], dim=1)


def expected_loo_log_marginals(plan, tensors, x, qvars, states):
    """(B, |Q|, C) fp64: the yardstick, the enumeration with nothing integrated."""
    none = np.zeros(plan.num_variables, dtype=bool)
    return torch.stack([S.enumerated_state_log_marginals(plan, tensors, x, v, none, states) for v in sorted(int(v) for v in qvars)], dim=1)


def normalise(t):
    t = torch.as_tensor(t)
    return t - torch.logsumexp(t, dim=-1, keepdim=True)


def entries(table, x, qvars):
    """(B, |Q|): the column of every query variable's observed state."""
    x = torch.as_tensor(x)[:, sorted(int(v) for v in qvars)].to(table.device)
    return torch.gather(table, 2, x[:, :, None])[:, :, 0]


def check_entries(got, want, what="", min_log_share=S.MIN_LOG_SHARE):
    """`P.check` for (B, |Q|) conditionals ``log p(x_v | x_-v)``: an entry of probability at least e^-4 is held to `R.bound` on the
    logarithm, the others to `S.EPS` on the probability; which is which is decided from the fp64 expectation, and at most a
    quarter of the entries may take the linear route.  Returns (worst error of the log route as a fraction of the bound, worst
    linear error, entries on the linear route, entries)."""
    got = torch.as_tensor(got).detach().cpu().double().numpy()
    want = torch.as_tensor(want).detach().cpu().double().numpy()
    assert got.shape == want.shape, (got.shape, want.shape)
    fin = np.isfinite(want)
    assert bool((got[~fin] == want[~fin]).all()), f"{what}: where the expected value is not finite"
    by_log = fin & (want >= min_log_share)
    by_lin = fin & ~by_log
    with np.errstate(all="ignore"):
        log_err = np.abs(got - want) / R.bound(want)
        lin_err = np.abs(np.exp(got) - np.exp(want))
    worst_log = float(log_err[by_log].max()) if by_log.any() else 0.0
    worst_lin = float(lin_err[by_lin].max()) if by_lin.any() else 0.0
    print(f"{what}: worst error {worst_log:.3f} of the bound; {int(by_lin.sum())} of {int(fin.sum())} entries below e^{S.MIN_LOG_SHARE:g}, "
          f"worst linear error {worst_lin:.1e}")
    assert 4 * int(by_lin.sum()) <= int(fin.sum()), f"{what}: more than a quarter of the entries take the linear route"
    assert not np.isnan(got[fin]).any(), f"{what}: NaN"
    assert worst_log <= 1.0, f"{what}: {worst_log} of the bound on the logarithm"
    assert worst_lin <= S.EPS, f"{what}: linear error {worst_lin}"
    return worst_log, worst_lin, int(by_lin.sum()), int(fin.sum())


# ---- the cases the CPU and the GPU tests share ------------------------------------------------------------------------------
TINY_QUERIES = [list(range(6)), [0, 1, 4], [3]]
EMB32_QUERIES = [list(range(16)), [1, 6, 11, 12]]
CAT_QUERY = [0, 6, 15]


def cases():
    """name -> (plan, tensors, states, rows, queries, min_log_share): every case the GPU tests run."""
    out = {}
    for sp in ("cp", "cp-t"):
        plan, tensors, states = R.tiny_case(sp)
        out[f"tiny-{sp}-3"] = (plan, tensors, states, P.tiny_rows(), TINY_QUERIES, S.MIN_LOG_SHARE)
        big, bt = R.pad_tiny_to_32(plan, tensors, sp)
        out[f"tiny-{sp}-32"] = (big, bt, states, P.tiny_rows(), TINY_QUERIES, S.MIN_LOG_SHARE)
    plan, tensors, states = R.emb32_case()
    out["emb32"] = (plan, tensors, states, P.emb32_rows(), EMB32_QUERIES, S.MIN_LOG_SHARE)
    plan, tensors, states = R.cat_case()
    out["cat"] = (plan, tensors, states, P.cat_rows(), [CAT_QUERY, list(range(16))], -np.inf)  # (no signed cancellation: `P.check`)
    return out


# ---- hand-built layers for the kernels alone ----------------------------------------------------------------------------------
LAYER_STATES = 7
LAYER_FOLDS = 2  # folds per launch; fold j reads weight fold j + 1 of 4
LAYER_SHAPES = {  # name -> (weights, Ki, Ko, the folds are output folds, [the child is a down fold])
    "stage32": (1, 32, 32, False, [True, True]),
    "root32": (1, 32, 1, True, [True]),
    "hadamard2": (0, 32, 32, False, [True, False]),
    "generic33": (1, 3, 3, False, [True, True]),
    "generic52": (1, 5, 2, False, [False, True]),
}


def _hand_layer(cplx, shape, B, seed):
    """A hand-built layer of two folds.  One weight column is 0 (a linear sum that is exactly 0: a -inf unit of P in every row);
    with B > 1 the last row's derivative is all -inf (every child's D and every state -inf, not NaN) and the row before it has one
    -inf entry.  Signed weights, tables and arguments 0 / pi under c32; positive weights and a table of logarithms under float."""
    wt, Ki, Ko, top, slots = LAYER_SHAPES[shape]
    g = torch.Generator().manual_seed(seed)

    def signs(*sh):
        return torch.where(torch.rand(*sh, generator=g) < 0.1, -1.0, 1.0).double()

    def values(*sh):
        re = torch.randn(*sh, generator=g, dtype=torch.float64)
        return torch.complex(re, (signs(*sh) < 0).double() * np.pi) if cplx else re

    w = None
    if wt:
        w = torch.randn(4, Ko, Ki, generator=g, dtype=torch.float64).abs() + 0.05
        if cplx:
            w = w * signs(4, Ko, Ki)
        w[:, :, Ki - 1] = 0.0
    folds = []
    for _ in range(LAYER_FOLDS):
        din = None
        if not top:
            din = values(B, Ko)
            if B > 1:
                din[B - 1] = torch.full((Ko,), -np.inf, dtype=torch.float64).to(din.dtype)
                din[B - 2, 0] = torch.tensor(-np.inf, dtype=torch.float64).to(din.dtype)
        folds.append((din, [values(B, Ki) for _ in slots]))
    tlog = 0 if cplx else 1
    table = torch.randn(LAYER_FOLDS * len(slots), LAYER_STATES + 1, Ki, generator=g, dtype=torch.float64)  # one per (fold, slot)
    if not tlog:
        table = (table.abs() + 0.05) * signs(*table.shape)
    x = torch.randint(0, LAYER_STATES, (B, LAYER_FOLDS * len(slots)), generator=g)
    return dict(w=w, Ki=Ki, Ko=Ko, top=top, slots=slots, folds=folds, table=table, tlog=tlog, x=x, cplx=cplx)


def hand_layer_run(case, dtype=torch.float64):
    """Per fold {slot: D of the down child} and per (fold, down slot) its ``log m`` (B, C), in `dtype`."""
    cplx = case["cplx"]
    cdt = (torch.complex128 if dtype == torch.float64 else torch.complex64) if cplx else dtype
    Ds, lms = [], {}
    nslots = len(case["slots"])
    for j, (din, kids) in enumerate(case["folds"]):
        if din is None:
            d = torch.full((1, case["Ko"]), -np.inf, dtype=cdt)
            d[0, 0] = 0
        else:
            d = din.to(cdt)
        w = None if case["w"] is None else case["w"][j + 1].to(dtype)
        out = layer_down(d, w, [v.to(cdt) for v in kids], [h for h, dn in enumerate(case["slots"]) if dn])
        Ds.append(out)
        for h, dc in out.items():
            t = case["table"][j * nslots + h, :LAYER_STATES]
            lms[(j, h)] = leaf_log_m(dc, (torch.exp(t) if case["tlog"] else t).to(dtype))
    return Ds, lms


def _small(lm, x_cols=None):
    """How many live values of the (B, C) fp64 table `lm` lie below e^-4 of their row's largest (of the normalised entries at
    `x_cols`: below e^-4), and how many there are."""
    live = torch.isfinite(lm).any(dim=1)
    t = lm[live]
    if x_cols is None:
        return int((t - t.amax(dim=1, keepdim=True) < S.MIN_LOG_SHARE).sum()), t.numel()
    e = torch.gather(normalise(t), 1, x_cols[live, None])
    return int((e < S.MIN_LOG_SHARE).sum()), e.numel()


@functools.lru_cache(maxsize=None)
def hand_layer(cplx, shape, B):
    """`_hand_layer` at the first seed from 97 + B on at which, in the fp64 expectation, at most an EIGHTH of the states and of
    the per-entry conditionals lie below e^-4 (half of what `P.check` lets onto the linear route): data chosen for the comparison
    rule, as `S.hand_path_case` chooses its own."""
    for seed in range(97 + B, 97 + B + 50):
        case = _hand_layer(cplx, shape, B, seed)
        _, lms = hand_layer_run(case)
        nslots = len(case["slots"])
        counts = [_small(lm.expand(B, -1)) for lm in lms.values()] + \
                 [_small(lm.expand(B, -1), case["x"][:, j * nslots + h]) for (j, h), lm in lms.items()]
        if all(8 * sum(c[0] for c in part) <= sum(c[1] for c in part) for part in (counts[: len(lms)], counts[len(lms):])):
            return case
    raise AssertionError("no seed keeps the states above the share")


def linear_error(got, want):
    """Worst |exp(got - max) - exp(want - max)| over (B, n) signed logarithms (numpy; complex: with their arguments), max the
    largest expected real part of the row; -inf must be met exactly."""
    gr, wr = (got.real, want.real) if np.iscomplexobj(want) else (got, want)
    assert not np.isnan(gr).any()
    dead = np.isneginf(wr)
    assert bool((gr[dead] == wr[dead]).all())
    with np.errstate(all="ignore"):
        mx = np.where(dead, -np.inf, wr).max(axis=1, keepdims=True)
        mx = np.where(np.isfinite(mx), mx, 0.0)
        f = lambda v, r: np.exp(r - mx) * (np.exp(1j * np.where(np.isneginf(r), 0.0, v.imag)) if np.iscomplexobj(v) else 1.0)
        return float(np.abs(f(got, gr) - f(want, wr)).max())
