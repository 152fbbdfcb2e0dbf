"""The restatement of interval evidence (tests/interval_restatement.py; DESIGN.md section 11, "Interval evidence") pinned on
the CPU: against brute force over the enumerated points of small boxes (the oracle's marginal forward, summed), its Gaussian
leaf against a 60-digit mpmath evaluation, and whole Gaussian plans against the oracle's integrated forward and a 1-D
quadrature of its forward.  The GPU tests (tests/test_interval.py) compare `HipCircuit.interval_log_prob` with this
restatement."""
import itertools

import numpy as np
import pytest
import torch

from interval_restatement import gaussian_leaf, interval_restated
from test_mpe import _case
from test_posterior_marginals import _states

DISCRETE = ["kat_bernoulli_f0o0", "kat_bernoulli_f1o1", "binomial_qg6x6_k4", "quadtree_4x4_kron_k3", "plan_quadgraph_1x4x4_cp",
            "quadgraph_6x6_tucker_k4"]
Z_GRID = [0.0, 0.5, -0.5, 3.0, -3.0, 8.0, -8.0, 12.0, -12.0, 30.0, -30.0]
WIDTHS = [1 / 1024, 1 / 256, 0.04, 1.0, 5.0, np.inf]


def small_boxes(states: np.ndarray, B: int, rng, max_points: int = 4096) -> tuple[np.ndarray, np.ndarray]:
    """(lo, hi) int64 (B, D): most variables a point or the full range, up to three proper sub-ranges per row, the number of
    points of a row's box over its NOT full-range variables at most `max_points`."""
    D = len(states)
    lo = np.zeros((B, D), dtype=np.int64)
    hi = np.zeros((B, D), dtype=np.int64)
    for n in range(B):
        full = rng.random(D) < 0.5
        pt = rng.integers(0, states)
        lo[n], hi[n] = np.where(full, 0, pt), np.where(full, states - 1, pt)
        budget = max_points
        for v in rng.choice(D, size=min(3, D), replace=False):
            C = int(states[v])
            w = int(rng.integers(2, min(C, 12) + 1))  # states in the range
            if C < 3 or w >= C or w > budget:
                continue
            a = int(rng.integers(0, C - w + 1))
            lo[n, v], hi[n, v] = a, a + w - 1
            budget //= w
    return lo, hi


def _brute_force(plan, tensors, lo, hi) -> np.ndarray:
    """(B,) log of the sum of the oracle's marginal forward over the enumerated points of every row's box, the full-range
    variables integrated by the oracle itself."""
    from oracle.torch_oracle import as_torch, evaluate_plan

    tt = {k: v.double() for k, v in as_torch(tensors).items()}
    states = _states(plan)
    want = np.empty(lo.shape[0])
    for n in range(lo.shape[0]):
        full = (lo[n] == 0) & (hi[n] == states - 1) & (states > 1)
        axes = [[0] if full[v] else list(range(lo[n, v], hi[n, v] + 1)) for v in range(len(states))]
        pts = np.array(list(itertools.product(*axes)), dtype=np.int64).reshape(-1, len(states))
        assert 0 < len(pts) <= 4096
        y = evaluate_plan(plan, tt, torch.from_numpy(pts), integrate_mask=torch.from_numpy(full))[:, 0, 0]
        want[n] = float(torch.logsumexp(y, 0))
    return want


@pytest.mark.parametrize("name", DISCRETE)
def test_restatement_equals_the_sum_over_the_points_of_the_box(name):
    plan, tensors = _case(name)
    states = _states(plan)
    lo, hi = small_boxes(states, 6, np.random.default_rng(21))
    assert states.max() <= 2 or ((hi > lo) & ~((lo == 0) & (hi == states - 1))).any()  # (proper sub-ranges where a variable has any)
    got = interval_restated(plan, tensors, lo, hi)["y"][:, 0, 0]
    # (the oracle's Binomial takes lgamma of an integer tensor in torch's default dtype: fp64 for both sides, as the posterior test)
    default = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        want = _brute_force(plan, tensors, lo, hi)
    finally:
        torch.set_default_dtype(default)
    assert np.isfinite(want).all()
    err = np.abs(got - want) / (1 + np.abs(want))
    assert err.max() <= 1e-9, err.max()
    # an empty set in one variable: probability 0
    lo[::2, 1], hi[::2, 1] = 1, 0
    got = interval_restated(plan, tensors, lo, hi)["y"][:, 0, 0]
    assert (got[::2] == -np.inf).all() and np.isfinite(got[1::2]).all()


def _mp_gaussian_leaf(lo: float, hi: float, mean: float, sd: float) -> float:
    import mpmath as mp

    mp.mp.dps = 60
    cdf = lambda t: mp.mpf(1) if t == np.inf else mp.mpf(0) if t == -np.inf else mp.ncdf((mp.mpf(t) - mp.mpf(mean)) / mp.mpf(sd))  # noqa: E731
    a, b = (mp.mpf(lo) - mean) / sd if np.isfinite(lo) else None, (mp.mpf(hi) - mean) / sd if np.isfinite(hi) else None
    # (the difference of two 60-digit CDFs, on the side where they are small: 60 digits lose 30 at |z| = 30 at most... taken on
    #  the lower tails, Phi(b) - Phi(a) = Phi(-a) - Phi(-b))
    if a is not None and b is not None and a + b > 0 or (a is not None and b is None):
        mass = (mp.ncdf(-a) if a is not None else mp.mpf(1)) - (mp.ncdf(-b) if b is not None else mp.mpf(0))
    else:
        mass = cdf(hi) - cdf(lo)
    return float(mp.log(mass))


def gaussian_grid(mean: float = 0.0, sd: float = 1.0):
    """(lo, hi) pairs: the z / width grid, the interval on either side of the point z, mapped through (mean, sd)."""
    out = []
    for z in Z_GRID:
        for w in WIDTHS:
            for side in (1, -1):
                a, b = (z, z + w) if side > 0 else (z - w, z)
                out.append((mean + sd * a, mean + sd * b))
    return out


def test_restated_gaussian_leaf_equals_mpmath():
    worst = 0.0
    for lo, hi in gaussian_grid():
        want = _mp_gaussian_leaf(lo, hi, 0.0, 1.0)
        got = float(gaussian_leaf(lo, hi, 0.0, 1.0))
        assert np.isfinite(want) and np.isfinite(got), (lo, hi, got, want)
        worst = max(worst, abs(got - want) / (1 + abs(want)))
    print(f"  Gaussian leaf against mpmath at 60 digits: {worst:.3e}")
    assert worst <= 1e-12, worst
    assert gaussian_leaf(1.0, 1.0, 0.0, 1.0) == -np.inf and gaussian_leaf(2.0, 1.0, 0.0, 1.0) == -np.inf
    assert gaussian_leaf(np.nan, 1.0, 0.0, 1.0, 0.25) == 0.25 and gaussian_leaf(-np.inf, np.inf, 0.0, 1.0, 0.25) == 0.25
    far = float(gaussian_leaf(40.0, 41.0, 0.0, 1.0))
    assert far == -np.inf or np.isfinite(far)


@pytest.mark.parametrize("name", ["kat_gaussian_f1o1", "pd_gauss_6x6_k4"])
def test_restated_gaussian_plans(name):
    from scipy.integrate import quad

    from oracle.torch_oracle import as_torch, evaluate_plan

    plan, tensors = _case(name)
    D, B = plan.num_variables, 4
    tt = {k: v.double() for k, v in as_torch(tensors).items()}
    rng = np.random.default_rng(22)
    inf = np.full((B, D), np.inf)
    x = rng.normal(size=(B, D))
    whole = evaluate_plan(plan, tt, torch.from_numpy(x), integrate_mask=torch.ones(D, dtype=torch.bool)).numpy()
    got = interval_restated(plan, tensors, -inf, inf)["y"]
    assert np.abs(got - whole).max() <= 1e-12 * (1 + np.abs(whole).max())
    # a box in ONE variable, every other variable at a point of density... integrated: the quadrature of the oracle's forward
    for v in (0, D - 1):
        lo, hi = -inf.copy(), inf.copy()
        lo[:, v], hi[:, v] = x[:, v] - 0.7, x[:, v] + 0.4
        got = interval_restated(plan, tensors, lo, hi)["y"][:, 0, 0]
        mask = torch.ones(D, dtype=torch.bool)
        mask[v] = False
        for n in range(B):
            def density(t: float) -> float:
                xs = torch.from_numpy(x[n : n + 1].copy())
                xs[0, v] = t
                return float(torch.exp(evaluate_plan(plan, tt, xs, integrate_mask=mask)[0, 0, 0]))

            mass, _ = quad(density, lo[n, v], hi[n, v], epsabs=1e-13, epsrel=1e-13)
            assert abs(got[n] - np.log(mass)) <= 1e-7, (v, n, got[n], np.log(mass))


def test_interval_entry_points_are_declared():
    from cirkit_amd import _capi as capi

    for n in ("ck_interval_stage", "ck_interval_block_sums", "ck_categorical_interval_fwd", "ck_gaussian_interval_fwd"):
        assert n in capi.SIGNATURES
