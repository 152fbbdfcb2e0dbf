"""The fp64 restatement of the parameter prologue (tests/prologue_restatement.py) against the oracle on committed
fixtures: what tests/test_gpu_param_prologue.py compares the kernels with has to be the reference's own arithmetic first.
Everything here is fp64 and agrees to 1e-12."""
import numpy as np
import pytest
import torch

from conftest import load_case
from prologue_restatement import (binomial_table, integral_row, log_table, softmax_rows, table_dense, tiled_positions,
                                  to_tiled, transpose_last2)

TOL = 1e-12


def _f64(tensors):
    from oracle.torch_oracle import as_torch

    return {k: v.double() for k, v in as_torch(tensors).items()}


@pytest.mark.parametrize("name", ["cfg1_rbt8", "binomial_qg6x6_k4"])
def test_softmax_rows_is_the_oracles_softmax_parameter(name):
    from oracle.torch_oracle import eval_param

    plan, tensors, _ = load_case(name)
    tt = _f64(tensors)
    seen = 0
    for l in plan.layers:
        for pg in l.params.values():
            if pg.ops != ["tensor", "softmax"]:
                continue
            want = eval_param(pg, tt)
            got = softmax_rows(tt[pg.nodes[0].config["tensor"]])
            assert got.shape == want.shape and float((got - want).abs().max()) <= TOL
            seen += 1
    assert seen >= 4


def test_log_table_is_the_oracles_categorical_layer():
    """probs = softmax(tensor) (kind 1): row x of the table is the layer's output at the value x."""
    from oracle.torch_oracle import _LSE, _layer_forward, eval_param

    plan, tensors, _ = load_case("cfg1_rbt8")
    tt = _f64(tensors)
    l = plan.layers[0]
    assert l.type == "categorical" and l.params["probs"].ops == ["tensor", "softmax"]
    C = int(l.config["num_categories"])
    table = log_table(tt[l.params["probs"].nodes[0].config["tensor"]])
    x = torch.arange(C)[None, :, None].expand(l.num_folds, C, 1)
    want = _layer_forward(_LSE, l, {"probs": eval_param(l.params["probs"], tt)}, x)  # (F, B = C, K)
    assert float((table[:, :C] - want).abs().max()) <= TOL
    assert (table[:, C] == 0).all()


@pytest.mark.parametrize("name", ["kat_bernoulli_f0o0", "kat_bernoulli_f1o1"])
def test_transposed_log_is_the_oracles_categorical_layer_with_plain_probs(name):
    """probs a plain tensor (the per-node path: `transpose_last2` with take_log, integral row mode 0)."""
    from oracle.torch_oracle import _LSE, _layer_forward

    plan, tensors, _ = load_case(name)
    tt = _f64(tensors)
    l = plan.layers[0]
    assert l.type == "categorical" and l.params["probs"].ops == ["tensor"]
    probs = tt[l.params["probs"].nodes[0].config["tensor"]]
    C = int(l.config["num_categories"])
    rows = transpose_last2(probs, take_log=True)  # (F, C, K)
    x = torch.arange(C)[None, :, None].expand(l.num_folds, C, 1)
    want = _layer_forward(_LSE, l, {"probs": probs}, x)
    assert float((rows - want).abs().max()) <= TOL
    table = torch.cat([rows, torch.full((l.num_folds, 1, rows.shape[2]), 7.0, dtype=rows.dtype)], dim=1)
    assert (integral_row(table, 0) == 0).all()
    assert float((integral_row(table, 1) - torch.logsumexp(rows, dim=1)).abs().max()) <= TOL
    assert (integral_row(table, 2) == 1).all()
    assert integral_row(table, 3).flatten().tolist() == [1.0, 0.0] * (table.shape[0] * table.shape[2] // 2)


def test_binomial_table_is_the_oracles_binomial_layer():
    from oracle.torch_oracle import _LSE, _layer_forward, eval_param

    plan, tensors, _ = load_case("binomial_qg6x6_k4")
    tt = _f64(tensors)
    l = plan.layers[0]
    assert l.type == "binomial"
    n = int(l.config["total_count"])
    p = eval_param(l.params["probs"], tt)  # (F, K)
    default = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)  # (the oracle's lgamma of an integer tensor comes out in the default dtype)
    try:
        x = torch.arange(n + 1)[None, :, None].expand(l.num_folds, n + 1, 1)
        want = _layer_forward(_LSE, l, {"probs": p}, x)
        want_l = _layer_forward(_LSE, l, {"logits": torch.log(p) - torch.log1p(-p)}, x)
    finally:
        torch.set_default_dtype(default)
    got = binomial_table(p, False, n)
    assert float((got[:, : n + 1] - want).abs().max()) <= TOL * float(want.abs().max())
    assert (got[:, n + 1] == 0).all()
    got_l = binomial_table(torch.log(p) - torch.log1p(-p), True, n)
    assert float((got_l[:, : n + 1] - want_l).abs().max()) <= TOL * float(want_l.abs().max())
    assert (got_l[:, n + 1] == 0).all()


@pytest.mark.parametrize("with_idx", [False, True])
def test_table_dense_is_the_oracles_categorical_then_dense_layer(with_idx):
    """Kind 4 / 5: a Categorical layer (F folds) read fold by fold -- through a map with repeats when Fd != F -- by a dense
    sum layer, evaluated by the oracle at every category, and at a marginalised variable for row C."""
    from cirkit_amd.plan import IDX_ARRAY, IDX_NONE, FoldIndex, LayerSpec, ParamGraph, ParamNode
    from oracle.torch_oracle import _LSE, _integrate_input, _layer_forward, eval_param

    F, K, C = 3, 4, 5
    g = torch.Generator().manual_seed(5)
    idx = [2, 0, 2, 1, 0] if with_idx else list(range(F))
    Fd = len(idx)
    theta = torch.randn(F, K, C, generator=g, dtype=torch.float64) * 2
    dense = torch.randn(Fd, K, K, generator=g, dtype=torch.float64) * 2

    def softmax_graph(name, nf, shape):
        nodes = [ParamNode("tensor", nf, shape, {"tensor": name}, []),
                 ParamNode("softmax", nf, shape, {"dim": len(shape) - 1}, [FoldIndex([0], IDX_NONE)])]
        return ParamGraph(nodes, FoldIndex([1], IDX_NONE), nf, shape)

    cat = LayerSpec("categorical", F, 1, 1, K, {"num_output_units": K, "num_categories": C}, {"probs": softmax_graph("th", F, (K, C))},
                    None, np.arange(F, dtype=np.int64)[:, None])
    dl = LayerSpec("sum", Fd, 1, K, K, {"num_input_units": K, "num_output_units": K, "arity": 1}, {"weight": softmax_graph("w", Fd, (K, K))},
                   FoldIndex([0], IDX_ARRAY, np.asarray(idx, dtype=np.int64)[:, None]))
    tt = {"th": theta, "w": dense}
    probs = {"probs": eval_param(cat.params["probs"], tt)}
    x = torch.arange(C)[None, :, None].expand(F, C, 1)
    y_cat = _layer_forward(_LSE, cat, probs, x)  # (F, C, K)
    y_int = _integrate_input(_LSE, cat, probs, y_cat[:, :1], torch.ones(F, dtype=torch.bool))  # (F, 1, K): the integral
    y_all = torch.cat([y_cat, y_int], dim=1)
    want = _layer_forward(_LSE, dl, {"weight": eval_param(dl.params["weight"], tt)}, y_all[torch.tensor(idx)][:, None])  # (Fd, C + 1, K)
    got = table_dense(theta, dense, idx if with_idx else None)
    assert got.shape == want.shape == (Fd, C + 1, K)
    assert float((got - want).abs().max()) <= TOL
    assert float(got[:, C].abs().max()) <= TOL  # log sum_k W[o, k] = 0


def test_tiled_layout_is_a_bijection():
    pos = tiled_positions()
    assert pos.shape == (1024, 2)
    assert len({(int(o), int(i)) for o, i in pos}) == 1024
    assert pos.min() == 0 and pos.max() == 31
    # every run of 4 dwords holds 4 consecutive inputs of one output: the 16-byte operand of an MFMA step
    runs = pos.reshape(256, 4, 2)
    assert (runs[:, :, 0] == runs[:, :1, 0]).all() and (np.diff(runs[:, :, 1], axis=1) == 1).all()
    w = torch.arange(2 * 1024, dtype=torch.float64).reshape(2, 32, 32)
    t = to_tiled(w)
    assert sorted(t[1].tolist()) == w[1].flatten().tolist()
    assert t[0, 0] == w[0, 0, 0] and t[0, 4 * 32] == w[0, 0, 4] and t[0, 256] == w[0, 0, 8]  # lane 32 -> inputs 4..7; q = 1 -> 8..


def test_table_job_bound_has_one_source():
    """The sizes the host registers for the batched prologue are the ones the launcher accepts: both ask
    `ck_param_table_job_fits` (K (C + 4) + 2 K (+ K^2) words, or C (K + 1) for the transposed kind-1 tile, in 160 KB)."""
    from cirkit_amd import _capi as capi

    try:
        capi.load()
    except (capi.HipExtensionError, OSError) as e:  # pragma: no cover - the extension is built before the suite runs
        pytest.fail(f"the HIP extension must be built: {e}")
    words = 160 * 1024 // 4
    for kind, K in [(1, 128), (1, 64), (1, 32), (4, 32), (4, 64), (5, 32)]:
        extra = K * K if kind >= 4 else 0
        cmax = max(c for c in range(1, 2000) if max(K * (c + 4) + 2 * K + extra, c * (K + 1) if kind == 1 else 0) <= words)
        assert capi.table_job_fits(kind, cmax, K) and not capi.table_job_fits(kind, cmax + 1, K), (kind, K, cmax)
    assert not capi.table_job_fits(1, 316, 128) and capi.table_job_fits(1, 314, 128)  # (the host guard used to take 315 .. 317)
    assert not capi.table_job_fits(0, 32, 32) and not capi.table_job_fits(3, 32, 32)
