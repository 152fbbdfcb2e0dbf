"""The algorithm of the squared circuits' marginals (cirkit_amd/squared.py) against fp64 enumeration, on the host: the torch
restatement (tests/squared_marginal_restatement.py) in fp64 reproduces ``logsumexp(2 Re log c)`` over every completion of
the missing variables; in fp32 -- the precision the GPU kernels work in -- its worst error stays below a QUARTER of the bound
the GPU tests assert (``1e-4 max(1, |want|)`` on the log value, the bound of Z in tests/test_functional.py), so a kernel that
meets the bound is not passing by the skin of a badly conditioned case; and the product's host-side classification
(`fold_classes`, `mixed_plan`) gives the class tables worked out by hand.

Worst fp32 errors as fractions of the bound (printed by the tests): tiny 0.030, tiny padded to 32 units 0.004, 32 signed
units 0.056, the Categorical fixture 0.001, the Gaussian fixture and the 8 x 8 image 0.001 (LAB_NOTES.md R7.16)."""
import numpy as np
import pytest
import torch

import squared_marginal_restatement as R
from cirkit_amd import _capi as capi
from cirkit_amd.squared import INTEGRATED, MIXED, OBSERVED, fold_classes, mixed_plan


def _all_masks(d):
    return [np.array([(i >> v) & 1 for v in range(d)], dtype=bool) for i in range(1 << d)]


def _frac(got, want):
    return float(((got.double() - want).abs() / torch.from_numpy(R.bound(want))).max())


@pytest.mark.parametrize("sum_product", ["cp-t", "cp"])
def test_every_mask_of_the_tiny_circuits(sum_product):
    plan, tensors, states = R.tiny_case(sum_product)
    x = R.rows_of(6, states, 5)
    log_z = R.enumerated_log_marginal(plan, tensors, x[:1], np.ones(6, dtype=bool), states)[0]
    worst64 = worst32 = 0.0
    for mask in _all_masks(6):
        want = R.enumerated_log_marginal(plan, tensors, x, mask, states)
        got, lz = R.restated_log_marginal(plan, tensors, x, mask)
        worst64 = max(worst64, float((got - want).abs().max()), abs(float(lz - log_z)))
        got32, lz32 = R.restated_log_marginal(plan, tensors, x, mask, torch.float32)
        worst32 = max(worst32, _frac(got32, want), _frac(got32 - lz32, want - log_z))
        # the product's classification is the one from explicit scopes
        assert all(np.array_equal(a, b) for a, b in zip(fold_classes(plan, mask), R.classes_from_scopes(plan, mask)))
    print(f"{sum_product}: worst fp64 error {worst64:.2e}, worst fp32 error {worst32:.3f} of the bound")
    assert worst64 < 1e-11
    assert worst32 < 0.25


@pytest.mark.parametrize("sum_product", ["cp-t", "cp"])
def test_tiny_circuit_padded_to_32_units_is_the_same_function(sum_product):
    plan, tensors, states = R.tiny_case(sum_product)
    big, bt = R.pad_tiny_to_32(plan, tensors, sum_product)
    x = R.rows_of(6, states, 5)
    worst = 0.0
    for mask in _all_masks(6)[::5]:
        want = R.enumerated_log_marginal(plan, tensors, x, mask, states)
        assert float((R.restated_log_marginal(big, bt, x, mask)[0] - want).abs().max()) < 1e-11
        worst = max(worst, _frac(R.restated_log_marginal(big, bt, x, mask, torch.float32)[0], want))
    print(f"padded {sum_product}: worst fp32 error {worst:.3f} of the bound")
    assert worst < 0.25


def test_class_tables_of_three_hand_checked_masks():
    """quad_tree(2, 3) with cp-t layers (6 leaves, then 3, 1, 1 folds).  None missing: every fold observed, no launch; all
    missing: every fold integrated, no launch; variable 4 missing: its leaf integrated, the other leaves observed, and the
    mixed folds exactly the ancestors of that leaf (read off the plan's own child tables), one per inner layer."""
    plan, _, _ = R.tiny_case("cp-t")
    D = plan.num_variables
    folds = [l.num_folds for l in plan.layers]
    none, every = np.zeros(D, dtype=bool), np.ones(D, dtype=bool)
    for mask, cl in ((none, OBSERVED), (every, INTEGRATED)):
        assert all((c == cl).all() for c in fold_classes(plan, mask))
        mp = mixed_plan(plan, mask)
        assert mp.layers == [] and mp.num_mixed == 0 and mp.root[0] == cl
    one = none.copy()
    one[4] = True
    cls = fold_classes(plan, one)
    scopes = R.fold_scopes(plan)
    leaf = [f for f, s in enumerate(scopes[0]) if s == frozenset({4})]
    assert len(leaf) == 1
    assert [int(c) for c in cls[0]] == [INTEGRATED if f == leaf[0] else OBSERVED for f in range(folds[0])]
    # the mixed folds are exactly the ancestors of that leaf: one per inner layer of the tree
    from cirkit_amd.plan import resolve_fold_index

    anc, cur = [], (0, leaf[0])
    for i in range(1, len(plan.layers)):
        ch = resolve_fold_index(plan.layers[i].inputs, folds)
        hit = [f for f in range(folds[i]) if any((int(p), int(g)) == cur for p, g in ch[f])]
        if hit:
            assert len(hit) == 1
            cur = (i, hit[0])
            anc.append(cur)
    assert len(anc) == len(plan.layers) - 1 and [a[0] for a in anc] == [1, 2, 3]
    assert {(i, f) for i in range(len(cls)) for f in range(folds[i]) if cls[i][f] == MIXED} == set(anc)
    mp = mixed_plan(plan, one)
    assert [(m.layer, m.folds.tolist()) for m in mp.layers] == [(i, [f]) for i, f in anc]
    # the first mixed fold multiplies the integrated leaf with its observed sibling, the others a mixed with an observed child
    assert sorted(mp.layers[0].kind[0].tolist()) == [capi.CK_SQ_CONST, capi.CK_SQ_RANK1]
    for m in mp.layers[1:]:
        assert sorted(m.kind[0].tolist()) == [capi.CK_SQ_FULL, capi.CK_SQ_RANK1]
    assert mp.root == (MIXED, 3, 0)


def test_the_4x4_masks_put_every_pair_of_child_kinds_into_a_product():
    plan, _, _ = R.emb32_case()
    pairs = set()
    for mask in R.masks_4x4():
        pairs |= R.child_kind_pairs(plan, mask)
    assert pairs == {(OBSERVED, INTEGRATED), (OBSERVED, MIXED), (INTEGRATED, MIXED), (MIXED, MIXED)}


def test_fp32_error_of_32_signed_units():
    plan, tensors, states = R.emb32_case()
    x = R.rows_of(16, states, 33)
    log_z = R.oracle_log_z(plan, tensors)
    worst = 0.0
    for mask in R.masks_4x4():
        want = R.enumerated_log_marginal(plan, tensors, x, mask, states)
        assert float((R.restated_log_marginal(plan, tensors, x, mask)[0] - want).abs().max()) < 1e-10
        got32, lz32 = R.restated_log_marginal(plan, tensors, x, mask, torch.float32)
        worst = max(worst, _frac(got32, want), _frac(got32 - lz32, want - log_z))
    print(f"32 signed units: worst fp32 error {worst:.3f} of the bound")
    assert worst < 0.25


def test_fp32_error_of_the_categorical_fixture():
    plan, tensors, states = R.cat_case()
    x = torch.from_numpy(np.random.default_rng(2).integers(0, states, size=(3, 16)))
    worst = 0.0
    for mask in R.masks_4x4(most=5):
        want = R.yardstick(plan, tensors, x, mask, states)
        if states ** int(mask.sum()) <= R.MAX_WORLDS:  # (enumerated: the fp64 restatement is pinned to it)
            assert float((R.restated_log_marginal(plan, tensors, x, mask)[0] - want).abs().max()) < 1e-10
        worst = max(worst, _frac(R.restated_log_marginal(plan, tensors, x, mask, torch.float32)[0], want))
    print(f"categorical fixture: worst fp32 error {worst:.3f} of the bound")
    assert worst < 0.25


def test_gaussian_fixture_against_quadrature():
    plan, tensors, x = R.gauss_case()
    x = x[:3]
    mask = np.zeros(16, dtype=bool)
    mask[5] = True
    want, moved = R.gauss_quadrature(plan, tensors, x, 5)
    assert float(moved) < 1e-9  # the grid is accepted only if doubling it moves the integral by less than that
    got, _ = R.restated_log_marginal(plan, tensors, x, mask)
    assert float((got - want).abs().max()) < 1e-8
    worst = _frac(R.restated_log_marginal(plan, tensors, x, mask, torch.float32)[0], want)
    print(f"gaussian fixture: worst fp32 error {worst:.3f} of the bound")
    assert worst < 0.25


def test_fp32_error_of_the_8x8_image():
    plan, tensors, states = R.img8_case()
    x = R.rows_of(64, states, 4)
    worst = 0.0
    for mask, extra in R.img8_masks():
        for m in [mask] + [mask | (np.arange(64) == v) for v in extra]:
            want = R.restated_log_marginal(plan, tensors, x, m)[0]
            worst = max(worst, _frac(R.restated_log_marginal(plan, tensors, x, m, torch.float32)[0], want))
    print(f"8 x 8 image: worst fp32 error {worst:.3f} of the bound")
    assert worst < 0.25
