"""Soft and interval evidence of squared circuits on the host: the torch restatement (tests/squared_soft_restatement.py) against
fp64 enumeration with the repository's oracle, the fp32 rounding of every case the GPU tests use (tests/test_squared_soft_evidence.py)
against half of their bound, the host plan with ``soft=`` (`cirkit_amd.squared.mixed_plan`) and the refusals of
cirkit_amd/squared_soft.py that need no device."""
import numpy as np
import pytest
import torch

import squared_marginal_restatement as R
import squared_soft_restatement as RS


def _worst(got, want):
    return float(((got.double() - want.double()).abs() / torch.from_numpy(R.bound(want))).max())


@pytest.mark.parametrize("sum_product", ["cp", "cp-t"])
def test_fp64_restatement_is_the_enumeration_on_the_tiny_circuits(sum_product):
    """6 variables, 3 states: every subset of three variables as S, with and without an integrated variable, and S = all."""
    plan, tensors, x, cases = RS.tiny_expected(sum_product)
    for s, m, ll, want in cases:
        got, _ = RS.restated_soft(plan, tensors, x, ll, RS.mask_of(s, 6), RS.mask_of(m, 6), 3)
        assert float((got - want).abs().max()) < 1e-11, (s, m)
    ll = RS.log_lik_of(5, 6, 3, 7)
    every, none = np.ones(6, dtype=bool), np.zeros(6, dtype=bool)
    got, _ = RS.restated_soft(plan, tensors, x, ll, every, none, 3)
    assert float((got - RS.enumerated_soft(plan, tensors, x, ll, every, none, 3)).abs().max()) < 1e-11


def test_fp64_restatement_is_the_enumeration_where_32_units_can_be_listed():
    """The splits of the 32-unit circuit that can be enumerated pin the restatement that serves as the yardstick of S = all."""
    plan, tensors, x, cases, _ = RS.emb32_expected()
    for s, m, ll, want in cases[:3]:
        got, _ = RS.restated_soft(plan, tensors, x[:3], ll[:3], RS.mask_of(s, 16), RS.mask_of(m, 16), 3)
        assert float((got - want[:3]).abs().max()) < 1e-9, (s, m)


def test_special_weights_restate_the_other_queries():
    """All-zero log weights are the marginal over S + M; one-hot log weights are the point evidence; 0/1 weights a box."""
    plan, tensors, x, _ = RS.tiny_expected("cp")
    s, m = RS.mask_of((0, 2), 6), RS.mask_of((3,), 6)
    zero = torch.zeros(5, 2, 3, dtype=torch.float64)
    got, _ = RS.restated_soft(plan, tensors, x, zero, s, m, 3)
    assert float((got - R.enumerated_log_marginal(plan, tensors, x, s | m, 3)).abs().max()) < 1e-11
    hot = torch.full((5, 2, 3), float("-inf"), dtype=torch.float64)
    hot.scatter_(2, x[:, [0, 2]][:, :, None], 0.0)
    got, _ = RS.restated_soft(plan, tensors, x, hot, s, m, 3)
    assert float((got - R.enumerated_log_marginal(plan, tensors, x, m, 3)).abs().max()) < 1e-11
    lo, hi = torch.zeros(5, 6, dtype=torch.int64), torch.ones(5, 6, dtype=torch.int64)
    box = RS.interval_log_lik(lo, hi, (0, 2), 3)
    got, _ = RS.restated_soft(plan, tensors, x, box, s, m, 3)
    assert float((got - RS.enumerated_soft(plan, tensors, x, box, s, m, 3)).abs().max()) < 1e-11


def test_fp32_restatement_stays_below_half_the_gpu_bound():
    """Every (circuit, S, M, log_lik) of the GPU tests, run through the restatement in fp32."""
    worst = {}
    for sp in ("cp", "cp-t"):
        plan, tensors, x, cases = RS.tiny_expected(sp)
        for s, m, ll, want in cases:
            got, _ = RS.restated_soft(plan, tensors, x, ll, RS.mask_of(s, 6), RS.mask_of(m, 6), 3, dtype=torch.float32)
            worst[f"tiny {sp} S={s} M={m}"] = _worst(got, want)
    plan, tensors, x, cases, _ = RS.emb32_expected()
    for s, m, ll, want in cases:
        got, _ = RS.restated_soft(plan, tensors, x, ll, RS.mask_of(s, 16), RS.mask_of(m, 16), 3, dtype=torch.float32)
        worst[f"emb32 |S|={len(s)}"] = _worst(got, want)
    plan, tensors, x, cases = RS.cat_expected()
    for s, m, ll, want in cases:
        got, _ = RS.restated_soft(plan, tensors, x, ll, RS.mask_of(s, 16), RS.mask_of(m, 16), 256, dtype=torch.float32)
        worst[f"cat |S|={len(s)}"] = _worst(got, want)
    top = max(worst, key=worst.get)
    print(f"worst fp32 error: {worst[top]:.3f} of the bound ({top})")
    assert worst[top] < 0.5, worst


# ---- the host plan -------------------------------------------------------------------------------------------------------------
def test_soft_none_reproduces_the_plan_of_today():
    from cirkit_amd.squared import mixed_plan

    plan, _, _ = R.emb32_case()
    for mask in R.masks_4x4():
        a, b = mixed_plan(plan, mask), mixed_plan(plan, mask, soft=None)
        assert b.leaves == [] and a.root == b.root and len(a.layers) == len(b.layers)
        assert all(np.array_equal(p, q) for p, q in zip(a.classes, b.classes))
        for p, q in zip(a.layers, b.layers):
            assert p.layer == q.layer and np.array_equal(p.folds, q.folds) and np.array_equal(p.kind, q.kind) and np.array_equal(p.src, q.src)
        empty = mixed_plan(plan, mask, soft=np.zeros(16, dtype=bool))  # (an empty soft set classifies nothing anew)
        assert empty.leaves == [] and all(np.array_equal(p, q) for p, q in zip(a.classes, empty.classes))


def test_host_plan_classes_and_leaf_records():
    from cirkit_amd import _capi as capi
    from cirkit_amd.squared import mixed_plan
    from cirkit_amd.squared_graph import INTEGRATED, MIXED, OBSERVED, FoldGraph

    plan, _, _ = R.emb32_case()
    graph = FoldGraph(plan)
    for s, m in RS.EMB32_SPLITS + (((2, 9), (3, 8, 12)),):
        soft, mask = RS.mask_of(s, 16), RS.mask_of(m, 16)
        mp = mixed_plan(plan, mask, graph=graph, soft=soft)
        want = RS.soft_classes(plan, soft, mask)
        assert all(np.array_equal(a, b) for a, b in zip(mp.classes, want))
        for i, scopes in enumerate(R.fold_scopes(plan)):
            for f, sc in enumerate(scopes):
                expect = OBSERVED if not sc & (set(s) | set(m)) else (INTEGRATED if sc <= set(m) else MIXED)
                assert mp.classes[i][f] == expect
        # the leaf records: every input fold over a soft variable, per input layer, with its position on the S axis
        got = {(lf.layer, int(f)): (int(v), int(p)) for lf in mp.leaves for f, v, p in zip(lf.folds, lf.var, lf.pos)}
        expect = {(i, f): (int(l.scope_idx[f][0]), sorted(s).index(int(l.scope_idx[f][0]))) for i, l in enumerate(plan.layers)
                  if l.inputs is None for f in range(l.num_folds) if int(l.scope_idx[f][0]) in s}
        assert got == expect and all(plan.layers[lf.layer].inputs is None for lf in mp.leaves)
        assert all(np.array_equal(lf.folds, np.sort(lf.folds)) for lf in mp.leaves)
        # every evaluated inner fold reads a soft leaf as FULL at its position among the leaf record's folds
        leaf_pos = {(lf.layer, int(f)): j for lf in mp.leaves for j, f in enumerate(lf.folds)}
        seen = 0
        for la in mp.layers:
            for j, f in enumerate(la.folds):
                for h, (p, g) in enumerate(graph.children[la.layer][f].tolist()):
                    if (p, g) in leaf_pos:
                        assert la.kind[j, h] == capi.CK_SQ_FULL and tuple(la.src[j, h]) == (p, leaf_pos[(p, g)])
                        seen += 1
        assert seen == len(leaf_pos)
        assert mp.root[0] == MIXED


class _Rows:
    """What `HipSquaredCircuit._row_bytes` reads of a circuit."""

    def __init__(self, plan, esize):
        from cirkit_amd.squared import HipSquaredCircuit
        from cirkit_amd.squared_graph import FoldGraph

        self.plan, self.graph, self._esize = plan, FoldGraph(plan), esize
        self._special = HipSquaredCircuit._special
        self.row_bytes = lambda mp: HipSquaredCircuit._row_bytes(self, mp)


def test_row_bytes_counts_the_leaf_blocks():
    from cirkit_amd.squared import mixed_plan

    plan, _, _ = R.emb32_case()
    rows = _Rows(plan, 8)
    arena_c = sum(l.num_folds * l.num_output_units for l in plan.layers)

    def inner(mp):  # 32 x 32 units per evaluated fold, one for the output fold; 32 units everywhere: no block between the stages
        return sum(len(la.folds) * plan.layers[la.layer].num_output_units ** 2 for la in mp.layers)

    for s, m in RS.EMB32_SPLITS:
        mp = mixed_plan(plan, RS.mask_of(m, 16), graph=rows.graph, soft=RS.mask_of(s, 16))
        assert rows.row_bytes(mp) == 8 * (arena_c + inner(mp) + len(s) * 1024)
    hard = mixed_plan(plan, RS.mask_of((4,), 16), graph=rows.graph)  # (without a soft set: as before)
    assert rows.row_bytes(hard) == 8 * (arena_c + inner(hard))


# ---- refusals that need no device --------------------------------------------------------------------------------------------------
def test_set_refusals():
    from cirkit_amd.squared_graph import FoldGraph
    from cirkit_amd.squared_soft import check_sets

    plan, _, _ = R.emb32_case()
    graph = FoldGraph(plan)
    none = np.zeros(16, dtype=bool)
    with pytest.raises(ValueError, match="at least one soft variable"):
        check_sets(graph, none, none, "soft evidence")
    with pytest.raises(ValueError, match="both soft and integrated"):
        check_sets(graph, RS.mask_of((1, 2), 16), RS.mask_of((2, 3), 16), "soft evidence")
    with pytest.raises(ValueError, match="both in the box and integrated"):
        check_sets(graph, RS.mask_of((1, 2), 16), RS.mask_of((2, 3), 16), "interval evidence")
    check_sets(graph, RS.mask_of((1, 2), 16), RS.mask_of((3,), 16), "soft evidence")
    gplan, _, _ = R.gauss_case()
    with pytest.raises(NotImplementedError, match="Gaussian layer"):
        check_sets(FoldGraph(gplan), RS.mask_of((5,), 16), none, "soft evidence")
    with pytest.raises(NotImplementedError, match="Gaussian layer"):
        check_sets(FoldGraph(gplan), RS.mask_of((5,), 16), none, "interval evidence")


class _Stub:
    """The plan and the fold graph: all the argument checks read before they touch a device."""

    def __init__(self, plan):
        from cirkit_amd.squared_graph import FoldGraph

        self.plan, self.graph = plan, FoldGraph(plan)


def test_argument_refusals():
    from cirkit_amd.squared_soft import interval_log_prob, log_cdf, soft_evidence_log_prob

    plan, _, _ = R.emb32_case()
    sq = _Stub(plan)
    x = R.rows_of(16, 3, 4)
    ll = torch.zeros(4, 2, 3)
    with pytest.raises(ValueError, match=r"shape \(B, S, C\)"):
        soft_evidence_log_prob(sq, ll[0], x, soft_vars=[1, 2])
    with pytest.raises(ValueError, match=r"shape \(B, S, C\)"):
        soft_evidence_log_prob(sq, ll.long(), x, soft_vars=[1, 2])
    with pytest.raises(ValueError, match="2 soft variables, soft_vars names 3"):
        soft_evidence_log_prob(sq, ll, x, soft_vars=[1, 2, 3])
    with pytest.raises(ValueError, match="has 2 states, the soft variables have up to 3"):
        soft_evidence_log_prob(sq, ll[:, :, :2], x, soft_vars=[1, 2])
    with pytest.raises(ValueError, match="x is required"):
        soft_evidence_log_prob(sq, ll, None, soft_vars=[1, 2])
    with pytest.raises(ValueError, match="4 rows and x 3"):
        soft_evidence_log_prob(sq, ll, x[:3], soft_vars=[1, 2])
    with pytest.raises(ValueError, match="at least one soft variable"):
        soft_evidence_log_prob(sq, ll, x, soft_vars=[])
    with pytest.raises(ValueError, match="both soft and integrated"):
        soft_evidence_log_prob(sq, ll, x, soft_vars=[1, 2], integrate_vars=[2])
    with pytest.raises(ValueError, match="subset of the circuit scope"):
        soft_evidence_log_prob(sq, ll, x, soft_vars=[1, 16])
    with pytest.raises(ValueError, match="ONE scope"):
        soft_evidence_log_prob(sq, ll, x, soft_vars=torch.zeros((4, 16), dtype=torch.bool))
    lo = torch.zeros(4, 16, dtype=torch.int64)
    with pytest.raises(ValueError, match="integer tensor of shape"):
        interval_log_prob(sq, lo.float(), lo, x, box_vars=[1])
    with pytest.raises(ValueError, match="integer tensor of shape"):
        interval_log_prob(sq, lo[:, :15], lo, x, box_vars=[1])
    with pytest.raises(ValueError, match="x is required"):
        interval_log_prob(sq, lo, lo, None, box_vars=[1])
    with pytest.raises(ValueError, match="both in the box and integrated"):
        interval_log_prob(sq, lo, lo, x, box_vars=[1], integrate_vars=[1])
    with pytest.raises(ValueError, match="integer tensor"):
        log_cdf(sq, x.float())
