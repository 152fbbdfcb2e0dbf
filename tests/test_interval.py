"""Interval (box) evidence on the GPU (`HipCircuit.interval_log_prob`, `HipCircuit.log_cdf`, cirkit_amd/interval.py,
cirkit_amd/csrc/ck_interval.hip; DESIGN.md section 11, "Interval evidence").

The reference has no such query.  The fp64 restatement of the contract (tests/interval_restatement.py) is pinned on the CPU
against brute force, mpmath and quadrature (tests/test_interval_restatement.py); here the GPU is compared with it.

Bit identity.  A point emits its table entry and the full range the integral row, so on an all-discrete circuit
``interval_log_prob(x, x)`` must equal the layer-wise forward of ``x`` bit for bit.  The query runs on the layer-wise circuit
of the plan the `HipCircuit` evaluates; the comparison circuit ``z`` is layer-wise on the user's plan, so the `HipCircuit` of
that test is built without unit padding: padded units change which sum kernels run and in which order they add, and no part
of this library promises equal bits across that.  (Padded circuits are compared with the restatement below.)

GPU tolerance, the project's rule: ``max |got - want| / (1 + |want|)`` over the finite ``want`` of the fp64 restatement must be
within 4 x the same figure of the restatement run in fp32 on the test's own plan and boxes, at least 1e-6, computed by the test
before it asserts; where ``want`` is -inf, so is ``got``.  The Gaussian leaf alone is held to 4 x 2^-24 (1 + |want|): its value
is computed in fp64 and rounded once.  Measured yardsticks and GPU errors: DESIGN.md section 11, "Interval evidence".
"""
import numpy as np
import pytest
import torch

from interval_restatement import gaussian_leaf, interval_restated
from test_interval_restatement import DISCRETE, WIDTHS, Z_GRID, gaussian_grid
from test_mpe import _case, _hc
from test_posterior_marginals import _states

NEW_ENTRY_POINTS = ("ck_interval_stage", "ck_interval_block_sums", "ck_categorical_interval_fwd", "ck_gaussian_interval_fwd")
GAUSSIAN = ["kat_gaussian_f1o1", "pd_gauss_6x6_k4"]
TEMPLATED = ["cat256_k32", "cat17_k3"]
ROWS = (1, 33, 70)


def _templated(name, logit_std=None):
    """cat256_k32: a 4 x 4 image, 256-state Categorical inputs, 32 units (vector path, 16 blocks of 16 states);
    cat17_k3: 5 variables of 17 states, 3 units (scalar path, a ragged last block).  `logit_std`: the input layers' logits
    drawn with that standard deviation (they reach the table through the plan's softmax)."""
    from cirkit_amd.initializers import init_plan_tensors
    from cirkit_amd.templates import InputSpec, build_plan, image_data, random_binary_tree

    if name == "cat256_k32":
        plan = image_data((1, 4, 4), region_graph="quad-tree-2", input_layer="categorical", num_input_units=32,
                          sum_product_layer="cp", num_sum_units=32)
    else:
        plan = build_plan(random_binary_tree(5), input_layer=InputSpec("categorical", 17), num_input_units=3, num_sum_units=3)
    tensors = init_plan_tensors(plan, seed=5)
    if logit_std is not None:
        rng = np.random.default_rng(31)
        for l in plan.layers:
            if l.inputs is None:
                for n in l.params["probs"].nodes:
                    if n.op == "tensor":
                        t = n.config["tensor"]
                        tensors[t] = (logit_std * rng.normal(size=tensors[t].shape)).astype(np.float32)
    return plan, tensors


def _plan(name):
    return _templated(name) if name in TEMPLATED else _case(name)


def _gaussian_vars(plan) -> np.ndarray:
    g = np.zeros(plan.num_variables, dtype=bool)
    for l in plan.layers:
        if l.type == "gaussian":
            g[l.scope_idx[:, 0]] = True
    return g


def _boxes(plan, B, kind, seed=0):
    """(lo, hi) float64 (B, D), holding what the device reads: integers for the discrete variables, fp32 values for the
    Gaussian ones.  random: a third points (narrow bins for a Gaussian variable), a third full ranges, a third proper
    sub-ranges; point / full: all of one sort; empty: random, with one variable's set empty in every third row."""
    rng = np.random.default_rng(seed)
    D = plan.num_variables
    states, gauss = _states(plan), _gaussian_vars(plan)
    C = np.where(gauss, 1, np.maximum(states, 1))
    sort = {"point": np.zeros((B, D), dtype=np.int64), "full": np.ones((B, D), dtype=np.int64)}.get(kind)
    if sort is None:
        sort = rng.integers(0, 3, size=(B, D))
    a = rng.integers(0, C, size=(B, D))
    b = rng.integers(0, C, size=(B, D))
    a, b = np.minimum(a, b), np.maximum(a, b)
    lo = np.where(sort == 0, a, np.where(sort == 1, 0, a)).astype(np.float64)
    hi = np.where(sort == 0, a, np.where(sort == 1, C - 1, b)).astype(np.float64)
    x = rng.normal(size=(B, D))
    w = rng.choice([1 / 512, 0.3, 2.0], size=(B, D))
    glo = np.where(sort == 0, x - 1 / 512, np.where(sort == 1, -np.inf, x - w))
    ghi = np.where(sort == 0, x + 1 / 512, np.where(sort == 1, np.inf, np.where(rng.random((B, D)) < 0.3, np.inf, x + w)))
    lo, hi = np.where(gauss, glo, lo), np.where(gauss, ghi, hi)
    if kind == "empty":
        v = int(rng.integers(0, D))
        lo[::3, v], hi[::3, v] = (0.5, -0.5) if gauss[v] else (1, 0)
    if gauss.any():
        lo, hi = lo.astype(np.float32).astype(np.float64), hi.astype(np.float32).astype(np.float64)
    return lo, hi


def _to_device(plan, lo, hi, dev):
    dt = torch.float32 if _gaussian_vars(plan).any() else torch.int64
    return torch.from_numpy(lo).to(dt).to(dev), torch.from_numpy(hi).to(dt).to(dev)


def _rel(got: np.ndarray, want: np.ndarray) -> float:
    fin = np.isfinite(want)
    if not fin.any():
        return 0.0
    with np.errstate(invalid="ignore"):
        return float((np.abs(got.astype(np.float64) - want)[fin] / (1 + np.abs(want[fin]))).max())


def _check(plan, tensors, lo, hi, got, cap=None):
    """`got` against the fp64 restatement under the project's rule; returns (GPU error, yardstick)."""
    want = interval_restated(plan, tensors, lo, hi)["y"]
    y32 = interval_restated(plan, tensors, lo, hi, dtype=np.float32)["y"]
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32, (got.shape, want.shape)
    yard = _rel(y32, want)
    print(f"  fp32-restatement yardstick {yard:.3e}")
    if cap is not None:
        assert yard < cap, (yard, cap)
    bound = max(4 * yard, 1e-6)
    assert not np.isnan(got).any()
    assert np.array_equal(got == -np.inf, want == -np.inf)
    assert not (got == np.inf).any()
    e = _rel(got, want)
    print(f"  GPU error {e:.3e} (bound {bound:.3e})")
    assert e <= bound, (e, bound)
    return e, yard, want


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.gpu
def test_interval_surface(hip_device):
    from cirkit_amd import _capi as capi
    from cirkit_amd.circuit import HipCircuit

    lib = capi.load()
    for n in NEW_ENTRY_POINTS:
        assert hasattr(lib, n) and n in capi.SIGNATURES
    assert callable(HipCircuit.interval_log_prob) and callable(HipCircuit.log_cdf)


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.gpu
@pytest.mark.parametrize("name", DISCRETE + ["cfg2_qt784"])
def test_points_and_full_ranges_are_the_layerwise_forward_bit_for_bit(hip_device, name):
    plan, tensors = _case(name)
    D, states = plan.num_variables, _states(plan)
    hc = _hc(plan, tensors, hip_device, pad_units=False)
    z = _hc(plan, tensors, hip_device, fuse=False, pad_units=False, use_graph=False)
    rng = np.random.default_rng(3)
    for B in ((33,) if name == "cfg2_qt784" else ROWS):
        x = rng.integers(0, states, size=(B, D))
        x[rng.random((B, D)) < 1 / 9] = -1  # sentinels: integrated, as the forward reads them
        x = torch.from_numpy(x).to(hip_device)
        got = hc.interval_log_prob(x, x)
        assert got.dtype == torch.float32 and tuple(got.shape) == tuple(z(x).shape)
        assert torch.equal(got, z(x)), name
        full_hi = torch.from_numpy(np.broadcast_to(states - 1, (B, D)).copy()).to(hip_device)
        got = hc.interval_log_prob(torch.zeros_like(x), full_hi)
        assert torch.equal(got, z(x, integrate_vars=range(D))), name
    hc.check_inputs()


# ---------------------------------------------------------------------------------------------------------------- 3, 4
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["random", "point", "full", "empty"])
@pytest.mark.parametrize("name", DISCRETE + GAUSSIAN + ["plan_clt_mixed6_cp", "cfg2_qt784"] + TEMPLATED)
def test_gpu_interval_equals_restatement(hip_device, name, kind):
    plan, tensors = _plan(name)
    hc = _hc(plan, tensors, hip_device)
    B = 33 if name == "cfg2_qt784" else ROWS[-1]
    lo, hi = _boxes(plan, B, kind, seed=4)
    dlo, dhi = _to_device(plan, lo, hi, hip_device)
    got = hc.interval_log_prob(dlo, dhi)
    _, _, want = _check(plan, tensors, lo, hi, got)
    if kind == "empty":  # only the rows with an empty set are -inf
        dead = np.zeros(B, dtype=bool)
        dead[::3] = True
        assert (want[dead] == -np.inf).all() and np.isfinite(want[~dead]).all()
    else:
        assert np.isfinite(want).all()
    if name != "cfg2_qt784" and kind == "random":  # the other row counts: the same rows, on their own
        for n in ROWS[:-1]:
            sub = hc.interval_log_prob(dlo[:n], dhi[:n]).cpu().numpy()
            e = _rel(sub, want[:n])
            assert np.array_equal(sub == -np.inf, want[:n] == -np.inf) and e <= max(4 * _rel(
                interval_restated(plan, tensors, lo[:n], hi[:n], dtype=np.float32)["y"], want[:n]), 1e-6), (n, e)


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.gpu
def test_gpu_narrow_tail_intervals(hip_device):
    """Ranges of 1 to 4 states of 256-state softmax rows with logit standard deviation 3: a difference of fp32 prefix sums
    returns mass 0 here; a sum of the terms does not."""
    plan, tensors = _templated("cat256_k32", logit_std=3.0)
    hc = _hc(plan, tensors, hip_device)
    B, D = 70, plan.num_variables
    rng = np.random.default_rng(6)
    w = rng.integers(1, 5, size=(B, D))
    lo = rng.integers(0, 256 - w + 1)
    hi = lo + w - 1
    got = hc.interval_log_prob(torch.from_numpy(lo).to(hip_device), torch.from_numpy(hi).to(hip_device))
    _, _, want = _check(plan, tensors, lo.astype(np.float64), hi.astype(np.float64), got, cap=1e-5)
    assert np.isfinite(want).all()


# ---------------------------------------------------------------------------------------------------------------- 6
def _one_gaussian(mean: float, sd: float):
    """The two-variable Gaussian fixture with every unit N(mean, sd^2), identity sum weights and a root that reads unit 0: with
    variable 1 integrated the output IS the input unit's value for variable 0."""
    plan, tensors = _case("kat_gaussian_f1o1")
    tensors = {k: np.array(v) for k, v in tensors.items()}
    g, s, c = plan.layers
    name = lambda l, p: l.params[p].nodes[0].config["tensor"]  # noqa: E731
    tensors[name(g, "mean")] = np.full((2, 2), mean, dtype=np.float32)
    tensors[name(g, "stddev")] = np.full((2, 2), sd, dtype=np.float32)
    tensors[name(s, "weight")] = np.broadcast_to(np.eye(2, dtype=np.float32), (2, 2, 2)).copy()
    tensors[name(c, "weight")] = np.array([[[1.0, 0.0]]], dtype=np.float32)
    return plan, tensors


@pytest.mark.gpu
@pytest.mark.parametrize("sd", [0.05, 1.0, 20.0])
@pytest.mark.parametrize("mean", [0.0, 3.0])
def test_gpu_gaussian_leaf_alone(hip_device, mean, sd):
    plan, tensors = _one_gaussian(mean, sd)
    hc = _hc(plan, tensors, hip_device)
    mean32, sd32 = float(np.float32(mean)), float(np.float32(sd))
    grid = np.array(gaussian_grid(mean32, sd32), dtype=np.float32)  # what the device reads: fp32 bounds
    assert len(grid) == len(Z_GRID) * len(WIDTHS) * 2
    extra = np.array([[1.0, 1.0], [2.0, 1.0], [np.nan, 1.0], [0.0, np.nan], [mean + 40 * sd, mean + 41 * sd],
                      [mean - 41 * sd, mean - 40 * sd], [-np.inf, np.inf], [np.inf, np.inf]], dtype=np.float32)
    b = np.concatenate([grid, extra])
    B = len(b)
    lo = np.stack([b[:, 0], np.full(B, -np.inf, dtype=np.float32)], axis=1)
    hi = np.stack([b[:, 1], np.full(B, np.inf, dtype=np.float32)], axis=1)
    got = hc.interval_log_prob(torch.from_numpy(lo).to(hip_device), torch.from_numpy(hi).to(hip_device))[:, 0, 0].cpu().numpy()
    want = gaussian_leaf(lo[:, 0].astype(np.float64), hi[:, 0].astype(np.float64), mean32, sd32)
    n = len(grid)
    fin = np.isfinite(want[:n])
    # (an fp32 bound can round a 1/1024-wide interval at |z| = 30 to a point: then -inf on both sides)
    assert np.array_equal(got[:n] == -np.inf, want[:n] == -np.inf) and fin.sum() >= n - 8
    err = float((np.abs(got[:n].astype(np.float64) - want[:n])[fin] / (1 + np.abs(want[:n][fin]))).max())
    print(f"  Gaussian leaf (mean {mean}, stddev {sd}): {err:.3e} (bound {4 * 2.0**-24:.3e})")
    assert err <= 4 * 2.0**-24, err
    e = got[n:]
    assert e[0] == -np.inf and e[1] == -np.inf  # lo == hi, lo > hi
    assert e[2] == 0.0 and e[3] == 0.0 and e[6] == 0.0  # NaN bounds integrate; the whole line has mass 1
    assert e[7] == -np.inf
    for v in e[4:6]:  # |z| = 40: -inf or correct, never NaN or +inf
        assert v == -np.inf or (np.isfinite(v) and v < -700)


# ---------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["plan_quadgraph_1x4x4_cp", "pd_gauss_6x6_k4", "plan_clt_mixed6_cp"])
def test_gpu_interval_chunking_does_not_change_results(hip_device, name):
    plan, tensors = _case(name)
    hc = _hc(plan, tensors, hip_device)
    lo, hi = _to_device(plan, *_boxes(plan, 70, "random", seed=7), hip_device)
    res = [hc.interval_log_prob(lo, hi, rows_per_chunk=r) for r in (None, 1, 7)]
    assert torch.equal(res[0], res[1]) and torch.equal(res[0], res[2])
    assert res[0].data_ptr() != res[1].data_ptr()  # the caller's own tensors
    with pytest.raises(ValueError):
        hc.interval_log_prob(lo, hi, rows_per_chunk=0)


# ---------------------------------------------------------------------------------------------------------------- 8
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["plan_quadgraph_1x4x4_cp", "binomial_qg6x6_k4", "pd_gauss_6x6_k4", "plan_clt_mixed6_cp"])
def test_gpu_integrate_vars_and_log_cdf(hip_device, name):
    plan, tensors = _case(name)
    D, B = plan.num_variables, 33
    hc = _hc(plan, tensors, hip_device)
    states, gauss = _states(plan), _gaussian_vars(plan)
    lo, hi = _boxes(plan, B, "random", seed=8)
    ids = list(range(0, D, 2))
    flo, fhi = lo.copy(), hi.copy()
    flo[:, ids] = np.where(gauss[ids], -np.inf, 0)
    fhi[:, ids] = np.where(gauss[ids], np.inf, states[ids] - 1)
    explicit = hc.interval_log_prob(*_to_device(plan, flo, fhi, hip_device))
    dlo, dhi = _to_device(plan, lo, hi, hip_device)
    assert torch.equal(hc.interval_log_prob(dlo, dhi, integrate_vars=ids), explicit)
    mask = torch.zeros(D, dtype=torch.bool)
    mask[ids] = True
    assert torch.equal(hc.interval_log_prob(dlo, dhi, integrate_vars=mask), explicit)
    assert torch.equal(hc.interval_log_prob(dlo, dhi, integrate_vars=mask[None].expand(B, D)), explicit)
    with pytest.raises(ValueError):
        hc.interval_log_prob(dlo, dhi, integrate_vars=[D])
    with pytest.raises(ValueError):
        hc.interval_log_prob(dlo, dhi, integrate_vars=torch.zeros(D, dtype=torch.int64))
    # log_cdf(x) = interval_log_prob(0 or -inf, x)
    bottom = torch.full_like(dhi, float("-inf")) if dhi.is_floating_point() else torch.zeros_like(dhi)
    assert torch.equal(hc.log_cdf(dhi), hc.interval_log_prob(bottom, dhi))
    assert torch.equal(hc.log_cdf(dhi, integrate_vars=ids), hc.interval_log_prob(bottom, dhi, integrate_vars=ids))


# ---------------------------------------------------------------------------------------------------------------- 9
@pytest.mark.gpu
def test_gpu_interval_refusals(hip_device):
    from cirkit_amd.initializers import init_plan_tensors
    from cirkit_amd.templates import image_data

    plan, tensors = _case("cfg5_sos_c_k32")
    hc = _hc(plan, tensors, hip_device)
    x = torch.zeros((4, plan.num_variables), dtype=torch.int64, device=hip_device)
    with pytest.raises(ValueError, match="lse-sum"):
        hc.interval_log_prob(x, x)
    with pytest.raises(ValueError, match="lse-sum"):
        hc.log_cdf(x)
    emb = image_data((1, 2, 2), region_graph="quad-tree-2", input_layer="embedding", num_input_units=4,
                     sum_product_layer="cp", num_sum_units=4)
    he = _hc(emb, init_plan_tensors(emb), hip_device)
    xe = torch.zeros((4, 4), dtype=torch.int64, device=hip_device)
    with pytest.raises(TypeError, match="Embedding"):
        he.interval_log_prob(xe, xe)
    assert getattr(he, "_sampler", None) is None
    plan, tensors = _case("plan_quadgraph_1x4x4_cp")
    D = plan.num_variables
    hc = _hc(plan, tensors, hip_device)
    x = torch.zeros((4, D), dtype=torch.int64, device=hip_device)
    for lo, hi in [(x[0], x[0]), (x, x[:3]), (x, x.to(torch.float32)), (x[:, : D - 1], x[:, : D - 1]), (x, x[:, : D - 1]),
                   (x[:0], x[:0]), (x.bool(), x.bool())]:
        with pytest.raises(ValueError):
            hc.interval_log_prob(lo, hi)
    assert hc._sampler._key is None and hc._sampler._zc is None and hc._sampler._interval._key is None
    assert tuple(hc.interval_log_prob(x, x + 3).shape) == (4, 1, 1)
    hc.check_inputs()
