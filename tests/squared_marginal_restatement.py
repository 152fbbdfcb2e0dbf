"""Marginals of a squared circuit (cirkit_amd/squared.py, csrc/ck_sqmar.hip) restated in torch on the host, and their
yardstick.

`restated_log_marginal` is the ALGORITHM of the product: classify every fold of c for the mask (here from explicit scope
sets, not by propagating classes), read an observed fold as the outer product of c's own outputs with their conjugates
(the lift, unit k K + l = y_k + conj(y_l)), an integrated fold from the partition-function circuit evaluated once, and
evaluate only the mixed folds at K^2 units: the Hadamard product of the children, then the two TensorDot stages.  It runs
in the dtype it is given (fp64: exact to rounding; fp32: the rounding the GPU kernels can be held to).

`enumerated_log_marginal` is the yardstick: c evaluated in fp64 by the repository's oracle on every completion of the
missing variables, ``logsumexp(2 Re log c)`` over them.
"""
import itertools

import numpy as np
import torch

from cirkit_amd.functional import squared_partition_plan
from cirkit_amd.plan import resolve_fold_index

OBSERVED, INTEGRATED, MIXED = 0, 1, 2


def fold_scopes(plan):
    """Per layer, per fold, the frozenset of variables under it."""
    folds = [l.num_folds for l in plan.layers]
    out = []
    for l in plan.layers:
        if l.inputs is None:
            out.append([frozenset(int(v) for v in row) for row in l.scope_idx])
        else:
            ch = resolve_fold_index(l.inputs, folds)
            out.append([frozenset().union(*(out[int(p)][int(f)] for p, f in row)) for row in ch])
    return out


def classes_from_scopes(plan, mask):
    M = frozenset(int(v) for v in np.nonzero(np.asarray(mask))[0])
    return [np.asarray([OBSERVED if not (s & M) else (INTEGRATED if s <= M else MIXED) for s in layer], dtype=np.int8)
            for layer in fold_scopes(plan)]


def _cast(tensors, dtype):
    return {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in tensors.items()}


def _stage(v, w):
    """One TensorDot stage in log space: v (B, Kj, Kq), real w (Kk, Kj) -> (B, Kq, Kk); the shift is the clamped maximum
    of the real parts over j (semiring.py:383-408, 441-476)."""
    re = v.real if v.is_complex() else v
    m = torch.clamp(re.amax(dim=1, keepdim=True), min=torch.finfo(re.dtype).min, max=torch.finfo(re.dtype).max)
    a = torch.exp(v - m)
    y = torch.einsum("bjq,kj->bqk", a, w.to(a.dtype))
    return torch.log(y) + m.transpose(1, 2)


def restated_log_marginal(plan, tensors, x, mask, dtype=torch.float64, return_tables=False):
    """(B,) unnormalised log marginal and log Z, both in `dtype`'s real type; x (B, D) with any value at masked variables."""
    from oracle.torch_oracle import eval_param, evaluate_plan

    mask = np.asarray(mask, dtype=bool)
    tt = _cast(tensors, dtype)
    x = torch.as_tensor(x).clone()
    x[:, torch.from_numpy(mask)] = 0
    if x.is_floating_point():
        x = x.to(dtype)
    _, c_out = evaluate_plan(plan, tt, x, return_all=True)
    z_plan, z_of = squared_partition_plan(plan, return_layer_map=True)
    z_root, z_out = evaluate_plan(z_plan, tt, None, return_all=True)
    cls = classes_from_scopes(plan, mask)
    folds = [l.num_folds for l in plan.layers]
    full = {}
    conj = plan.semiring == "complex-lse-sum"

    def child(p, f):
        if cls[p][f] == MIXED:
            return full[(p, f)]
        if cls[p][f] == INTEGRATED:
            return z_out[z_of[p]][f]  # (1, K^2): no row stride
        y = c_out[p][f]  # (B, K): the lift
        return (y[:, :, None] + (y.conj() if conj else y)[:, None, :]).flatten(1)

    tables = []
    for i, l in enumerate(plan.layers):
        if l.inputs is None:
            continue
        ch = resolve_fold_index(l.inputs, folds)
        mixed = [f for f in range(l.num_folds) if cls[i][f] == MIXED]
        if mixed:
            tables.append((i, mixed, [[int(cls[int(p)][int(g)]) for p, g in ch[f]] for f in mixed]))
        w = eval_param(l.params["weight"], tt) if "weight" in l.params else None
        for f in mixed:
            v = sum(child(int(p), int(g)) for p, g in ch[f])
            if l.type != "hadamard":
                K = l.num_input_units
                v = _stage(v.reshape(-1, K, K), w[f])  # contracts the slow factor with W
                v = _stage(v, w[f]).flatten(1)  # then the other one (real weights: conj W = W)
            full[(i, f)] = v
    op, of = (int(v) for v in resolve_fold_index(plan.output, folds).reshape(-1, 2)[0])
    B = x.shape[0]
    if cls[op][of] == MIXED:
        val = full[(op, of)][:, 0]
    elif cls[op][of] == INTEGRATED:
        val = z_out[z_of[op]][of][:, 0].expand(B)
    else:
        val = 2 * c_out[op][of][:, 0].real if conj else 2 * c_out[op][of][:, 0]
    val = val.real if val.is_complex() else val
    lz = z_root.reshape(-1)[0]
    lz = lz.real if lz.is_complex() else lz
    return (val, lz, cls, tables) if return_tables else (val, lz)


def all_worlds(num_variables, states):
    return torch.tensor(list(itertools.product(range(states), repeat=num_variables)), dtype=torch.int64)


def log_c2_of(plan, tensors, rows):
    """2 Re log c in fp64 (the oracle) of the given rows."""
    from oracle.torch_oracle import evaluate_plan

    y = evaluate_plan(plan, _cast(tensors, torch.float64), rows).reshape(rows.shape[0], -1)[:, 0]
    return 2 * (y.real if y.is_complex() else y)


def oracle_log_z(plan, tensors):
    """log Z in fp64 from the oracle's run of `squared_partition_plan` -- pinned to the enumeration over all worlds where
    that can be enumerated and to the reference's committed output (tests/test_functional.py)."""
    from oracle.torch_oracle import evaluate_plan

    z = evaluate_plan(squared_partition_plan(plan), _cast(tensors, torch.float64), None).reshape(-1)[0]
    return z.real if z.is_complex() else z


MAX_WORLDS = 70000  # (256^2 completions of two 8-bit pixels still are)


def log_c2_of_float(plan, tensors, rows):
    """2 log c in fp64 of float rows (Gaussian inputs)."""
    from oracle.torch_oracle import evaluate_plan

    return 2 * evaluate_plan(plan, _cast(tensors, torch.float64), rows.to(torch.float64)).reshape(rows.shape[0], -1)[:, 0]


def enumerated_log_marginal(plan, tensors, x, mask, states):
    """(B,) fp64: logsumexp over every completion of the masked variables of 2 Re log c (unnormalised).  More than
    `MAX_WORLDS` completions per row (all 16 pixels of a 4 x 4 image: 3^16) cannot be enumerated in a test: with EVERY
    variable masked the value is Z, taken from `oracle_log_z`; anything else that large is refused."""
    mask = np.asarray(mask, dtype=bool)
    miss = np.nonzero(mask)[0]
    x = torch.as_tensor(x).to(torch.int64)
    if states ** len(miss) > MAX_WORLDS:
        assert mask.all(), "too many completions to enumerate"
        return oracle_log_z(plan, tensors).expand(x.shape[0]).clone()
    if len(miss) == 0:
        return log_c2_of(plan, tensors, x)
    comp = all_worlds(len(miss), states)  # (W, |M|)
    rows = x[:, None, :].repeat(1, comp.shape[0], 1)
    rows[:, :, torch.from_numpy(miss)] = comp[None]
    lc = log_c2_of(plan, tensors, rows.reshape(-1, x.shape[1])).reshape(x.shape[0], -1)
    return torch.logsumexp(lc, dim=1)


def bound(want):
    """The project's bound for Z on the GPU (tests/test_functional.py), on the log value."""
    return 1e-4 * np.maximum(1.0, np.abs(np.asarray(want, dtype=np.float64)))


# ---- the cases the CPU and the GPU tests share ------------------------------------------------------------------------------
def tiny_case(sum_product):
    """`_tiny` of tests/test_functional.py: quad_tree(2, 3), Embedding with 3 states, K = 3, weights 0.5 x seed 5."""
    from cirkit_amd.initializers import init_plan_tensors
    from cirkit_amd.templates import InputSpec, build_plan, quad_tree

    plan = build_plan(quad_tree(2, 3), input_layer=InputSpec("embedding", 3), sum_product=sum_product, num_input_units=3,
                      num_sum_units=3, sum_activation="none", semiring="complex-lse-sum")
    tensors = {n: 0.5 * v for n, v in init_plan_tensors(plan, seed=5).items()}
    return plan, tensors, 3


def pad_tiny_to_32(plan, tensors, sum_product):
    """The same function on 32 units: the plan rebuilt with K = 32 and the K = 3 values embedded in its tensors.  A padded
    unit is a COPY of unit 0 of its layer (same Embedding row, same weight row) and every weight that multiplies a padded
    input unit is 0, the scheme of cirkit_amd/padding.py."""
    from cirkit_amd.templates import InputSpec, build_plan, quad_tree

    big = build_plan(quad_tree(2, 3), input_layer=InputSpec("embedding", 3), sum_product=sum_product, num_input_units=32,
                     num_sum_units=32, sum_activation="none", semiring="complex-lse-sum")
    assert list(big.tensors) == list(plan.tensors)
    kinds = {}
    for l in big.layers:
        for g in l.params.values():
            for n in g.nodes:
                if n.op == "tensor":
                    kinds[n.config["tensor"]] = l.type
    out = {}
    for name, (shape, _) in big.tensors.items():
        v = np.asarray(tensors[name])
        p = np.zeros(shape, dtype=v.dtype)
        if kinds[name] == "embedding":  # (F, K, states): units copied
            p[:, : v.shape[1]] = v
            p[:, v.shape[1]:] = v[:, :1]
        else:  # (F, Ko, Ki): rows copied, padded columns 0
            p[:, : v.shape[1], : v.shape[2]] = v
            p[:, v.shape[1]:, : v.shape[2]] = v[:, :1]
        out[name] = p
    return big, out


def emb32_case(scale=0.25, seed=11):
    """image_data((1, 4, 4), 'quad-tree-2') with Embedding inputs over 3 states, 32 units, `cp` layers, signed weights."""
    from cirkit_amd.initializers import init_plan_tensors
    from cirkit_amd.templates import InputSpec, build_plan, quad_tree

    plan = build_plan(quad_tree(4, 4), input_layer=InputSpec("embedding", 3), sum_product="cp", num_input_units=32,
                      num_sum_units=32, sum_activation="none", semiring="complex-lse-sum")
    tensors = {n: scale * v for n, v in init_plan_tensors(plan, seed=seed).items()}
    return plan, tensors, 3


def masks_4x4(seed=3, most=6):
    """None; all; {0}; {15}; a 2 x 2 block plus two scattered pixels; two random masks of at most `most` variables."""
    rng = np.random.default_rng(seed)
    block = [0, 1, 4, 5, 2, 15][:most]  # (an aligned 2 x 2 block is an INTEGRATED fold: const children)
    ids = [[], list(range(16)), [0], [15], block] + [sorted(rng.choice(16, size=int(rng.integers(2, most + 1)), replace=False).tolist())
                                                       for _ in range(2)]
    out = []
    for i in ids:
        m = np.zeros(16, dtype=bool)
        m[i] = True
        out.append(m)
    return out


def rows_of(num_variables, states, B, seed=1):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, states, size=(B, num_variables)))


def child_kind_pairs(plan, mask):
    """The unordered pairs of child classes that meet in some Hadamard product of a mixed fold."""
    cls = classes_from_scopes(plan, mask)
    folds = [l.num_folds for l in plan.layers]
    pairs = set()
    for i, l in enumerate(plan.layers):
        if l.inputs is None or l.arity < 2:
            continue
        ch = resolve_fold_index(l.inputs, folds)
        for f in range(l.num_folds):
            if cls[i][f] == MIXED:
                ks = [int(cls[int(p)][int(g)]) for p, g in ch[f]]
                pairs |= {tuple(sorted((a, b))) for a, b in itertools.combinations(ks, 2)}
    return pairs


def yardstick(plan, tensors, x, mask, states):
    """The expected unnormalised log marginal in fp64: the enumeration where the completions can be enumerated (and Z itself
    with everything masked), else -- three or more 256-state pixels -- the fp64 run of the restatement, which the CPU tests pin
    to the enumeration on every mask that can be enumerated."""
    mask = np.asarray(mask, dtype=bool)
    if states ** int(mask.sum()) <= MAX_WORLDS or mask.all():
        return enumerated_log_marginal(plan, tensors, x, mask, states)
    return restated_log_marginal(plan, tensors, x, mask)[0]


def cat_case():
    """The `sq_cat_qt4x4_k5` fixture: a real circuit (Categorical inputs over 256 states, K = 5) under lse-sum."""
    from conftest import load_case
    from cirkit_amd.initializers import init_plan_tensors

    plan, _, _ = load_case("sq_cat_qt4x4_k5")
    return plan, init_plan_tensors(plan, seed=6), 256


def gauss_case():
    from conftest import load_case
    from cirkit_amd.initializers import init_plan_tensors

    plan, _, g = load_case("sq_gauss_qt4x4_k4")
    return plan, init_plan_tensors(plan, seed=8), torch.from_numpy(g["x"]).to(torch.float64)


def gauss_quadrature(plan, tensors, x, v, n=4001, half_width=12.0):
    """(B,) fp64: log of the trapezoid integral of c(x)^2 over variable v on n points of [-half_width, half_width], and the
    relative change of the integral against the grid of (n - 1) / 2 + 1 points (every second point)."""
    grid = torch.linspace(-half_width, half_width, n, dtype=torch.float64)
    rows = x[:, None, :].repeat(1, n, 1)
    rows[:, :, v] = grid[None]
    from oracle.torch_oracle import evaluate_plan

    lc = 2 * evaluate_plan(plan, _cast(tensors, torch.float64), rows.reshape(-1, x.shape[1])).reshape(x.shape[0], n)
    m = lc.amax(dim=1, keepdim=True)
    f = torch.exp(lc - m)
    fine = torch.trapezoid(f, grid, dim=1)
    coarse = torch.trapezoid(f[:, ::2], grid[::2], dim=1)
    return torch.log(fine) + m[:, 0], ((fine - coarse).abs() / fine).max()


def img8_case(scale=0.25, seed=13):
    """image_data((1, 8, 8), 'quad-tree-2') with Embedding inputs over 4 states, 32 units: past what can be enumerated."""
    from cirkit_amd.initializers import init_plan_tensors
    from cirkit_amd.templates import InputSpec, build_plan, quad_tree

    plan = build_plan(quad_tree(8, 8), input_layer=InputSpec("embedding", 4), sum_product="cp", num_input_units=32,
                      num_sum_units=32, sum_activation="none", semiring="complex-lse-sum")
    return plan, {n: scale * v for n, v in init_plan_tensors(plan, seed=seed).items()}, 4


def img8_masks(seed=7):
    """Three random masks M of 8 .. 24 of the 64 pixels and, for each, three variables outside it."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(3):
        m = np.zeros(64, dtype=bool)
        m[rng.choice(64, size=int(rng.integers(8, 25)), replace=False)] = True
        out.append((m, [int(v) for v in rng.choice(np.nonzero(~m)[0], size=3, replace=False)]))
    return out
