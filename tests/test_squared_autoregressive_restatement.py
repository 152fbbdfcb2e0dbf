"""The algorithm of the autoregressive conditionals of squared circuits (cirkit_amd/squared_autoregressive.py) on the host:
the step-by-step restatement (tests/squared_autoregressive_restatement.py) in fp64 reproduces the enumeration for every state of
every step; in fp32 it stays below a quarter of the bound the GPU tests assert (`R.bound`, on the states and the (row, step)
pairs that hold at least e^-4 of their row's largest state); `tree_order` needs no mixed step; the quantiser of
tests/autoregressive_restatement.py gives valid tables on ``exp`` of the restated conditionals; the coder round-trips when the
fp64 restatement provides its tables; the recorded expectations (tests/golden/sq_autoregressive_expected.npz) are what the
restatement gives; and `ck_squared_path_steps` refuses bad host words before it launches anything."""
import ctypes

import numpy as np
import pytest
import torch

import squared_autoregressive_restatement as A
import squared_marginal_restatement as R
import squared_sampling_restatement as S
from cirkit_amd.squared_sampling import path_plan, tree_order


@pytest.mark.parametrize("sum_product", ["cp-t", "cp"])
def test_choice_of_the_tiny_rows(sum_product):
    """The rows of `A.TINY_AR_ROWS_SEED` on both tiny circuits and the three orders: fp64 to rounding at EVERY state; at most 5 %
    of the (row, step) pairs are left out of the log-probability comparison; the fp32 restatement (K = 3 and padded to 32 units)
    stays below a quarter of the bound on the kept pairs and the kept states."""
    plan, tensors, states = R.tiny_case(sum_product)
    big = R.pad_tiny_to_32(plan, tensors, sum_product)
    x = A.tiny_rows()
    kept = total = 0
    for name, order in A.tiny_orders(plan).items():
        wm, wc, wl = A.enumerated(plan, tensors, x, order, states)
        gm, gc, gl = A.restated(plan, tensors, x, order, states)
        assert float((gm - wm).abs().max()) < 1e-10 and float((gc - wc).abs().max()) < 1e-10 and float((gl - wl).abs().max()) < 1e-10
        pairs, st = A.kept_pairs(wc, x, order), A.kept_states(wc)
        kept, total = kept + int(pairs.sum()), total + pairs.numel()
        assert float(torch.logsumexp(wc, dim=2).abs().max()) < 1e-12
        for run in ((plan, tensors), big):
            _, c32, l32 = A.restated(*run, x, order, states, dtype=torch.float32)
            fl, fc = A.frac_of_bound(l32, wl, pairs), A.frac_of_bound(c32, wc, st)
            print(f"{sum_product} {name} K={run[0].layers[0].num_output_units}: log probabilities {fl:.3f}, conditionals {fc:.3f} of the bound")
            assert fl < 0.25 and fc < 0.25
    print(f"{sum_product}: {kept} of {total} (row, step) pairs kept")
    assert 1.0 - kept / total <= A.MAX_LEFT_OUT


def test_recorded_share_of_the_chosen_seed():
    kept = 0
    for sum_product in ("cp-t", "cp"):
        plan, tensors, states = R.tiny_case(sum_product)
        for order in A.tiny_orders(plan).values():
            kept += int(A.kept_pairs(A.enumerated(plan, tensors, A.tiny_rows(), order, states)[1], A.tiny_rows(), order).sum())
    assert kept == A.TINY_AR_MEASURED[A.TINY_AR_ROWS_SEED][0]


@pytest.mark.parametrize("sum_product", ["cp-t", "cp"])
def test_the_steps_sum_to_the_log_probability(sum_product):
    plan, tensors, states = R.tiny_case(sum_product)
    x = A.tiny_rows()
    want = R.log_c2_of(plan, tensors, x) - R.oracle_log_z(plan, tensors)
    for order in A.tiny_orders(plan).values():
        assert float((A.restated(plan, tensors, x, order, states)[2].sum(dim=1) - want).abs().max()) < 1e-10


def test_integrated_variables_stay_integrated():
    """`integrate_vars` = {1, 4}: step i is the conditional given the prefix with 1, 4 and the later variables summed out."""
    plan, tensors, states = R.tiny_case("cp")
    x = A.tiny_rows()
    base = np.zeros(6, dtype=bool)
    base[[1, 4]] = True
    order = [v for v in tree_order(plan) if not base[v]]
    wm, wc, wl = A.enumerated(plan, tensors, x, order, states, integrated=base)
    gm, gc, gl = A.restated(plan, tensors, x, order, states, integrated=base)
    assert float((gc - wc).abs().max()) < 1e-10
    want = R.enumerated_log_marginal(plan, tensors, x, base, states) - R.oracle_log_z(plan, tensors)
    assert float((wl.sum(dim=1) - want).abs().max()) < 1e-10


def _plans():
    from cirkit_amd.templates import InputSpec, build_plan, quad_tree

    out = {"tiny": R.tiny_case("cp")[0]}
    for side in (4, 8):
        out[f"{side}x{side}"] = build_plan(quad_tree(side, side), input_layer=InputSpec("embedding", 3), sum_product="cp", num_input_units=2,
                                           num_sum_units=2, sum_activation="none", semiring="complex-lse-sum")
    return out


@pytest.mark.parametrize("name", ["tiny", "4x4", "8x8"])
def test_tree_order_needs_no_mixed_step(name):
    """At every step of `tree_order` every sibling of the path is entirely before or entirely after the step's variable -- in its
    reverse too; a permutation / raster order does meet split siblings."""
    plan = _plans()[name]
    D = plan.num_variables
    order = tree_order(plan)
    assert sorted(order) == list(range(D))

    def split(o):
        n = 0
        for i, v in enumerate(o):
            mask = np.zeros(D, dtype=bool)
            mask[o[i:]] = True
            cls = R.classes_from_scopes(plan, mask)
            n += any(cls[p][g] == R.MIXED for lv in path_plan(plan, v).levels for p, g in lv.siblings)
        return n

    assert split(order) == 0
    assert split(order[::-1]) == 0  # (the reverse of a depth-first walk is the depth-first walk of the mirrored tree)
    other = A.tiny_orders(plan)["permuted"] if name == "tiny" else list(range(D))  # (raster order on the images)
    assert split(other) > 0


def _check_tables(t, states, precision):
    T = 1 << precision
    assert t.dtype == np.int32 and bool((t[..., 0] == 0).all()) and bool((t[..., states:] == T).all())
    assert bool((np.diff(t[..., : states + 1].astype(np.int64), axis=-1) >= 1).all())


@pytest.mark.parametrize("precision", [8, 16, 24])
def test_quantiser_on_the_restated_conditionals(precision):
    plan, tensors, states = R.tiny_case("cp")
    x = A.tiny_rows()
    cond = A.restated(plan, tensors, x, tree_order(plan), states, dtype=torch.float32)[1].numpy()
    t = A.tables_of(cond, [states], precision)
    assert t.shape == (5, 6, states + 1)
    _check_tables(t, states, precision)
    counts = np.diff(t.astype(np.int64), axis=2) / float(1 << precision)
    assert float(np.abs(counts - np.exp(cond.astype(np.float64))).max()) <= (2.0 * states + 2) / (1 << precision) + 1e-6
    spoilt = cond.copy()
    spoilt[1] = np.nan  # a NaN row: the uniform table, the others keep their integers
    u = A.tables_of(spoilt, [states], precision)
    T = 1 << precision
    flat = np.concatenate([[0], np.cumsum([T // states + (T - (T // states) * states if c == 0 else 0) for c in range(states)])])
    assert bool((u[1] == flat[None, :]).all()) and np.array_equal(u[[0, 2, 3, 4]], t[[0, 2, 3, 4]])
    g = A.golden()
    tc = A.tables_of(g["cat_cond"].astype(np.float32), [256], max(precision, 10))
    _check_tables(tc, 256, max(precision, 10))


@pytest.mark.parametrize("sum_product", ["cp-t", "cp"])
def test_the_coder_round_trips_on_the_fp64_restatement(sum_product):
    from cirkit_amd import codec

    plan, tensors, states = R.tiny_case(sum_product)
    x = A.tiny_rows().numpy()
    for order in A.tiny_orders(plan).values():
        tables = A.restated_tables(plan, tensors, order, states, 16)
        blobs, counts = codec.encode(tables, x, order, precision=16, return_counts=True)
        assert np.array_equal(codec.decode(tables, blobs, order, 6, precision=16), x)
        bits = np.asarray([8 * len(b) for b in blobs])
        assert bool((bits <= codec.ideal_bits(counts, 16) + codec.OVERHEAD_BITS).all())


def test_recorded_expectations_of_the_categorical_fixture():
    """The golden file is what the fp64 restatement gives; at the two steps that can be enumerated it is the enumeration; the
    fp32 restatement stays below a quarter of the bound on the kept states and pairs."""
    plan, tensors, states = R.cat_case()
    x, order = A.cat_rows(), tree_order(plan)
    g = A.golden()
    lm, cond, logp = A.cat_expected()
    assert g["cat_log_m"].shape == (3, 16, 256) and g["cat_logp"].shape == (3, 16)
    for k, v in (("cat_log_m", lm), ("cat_cond", cond), ("cat_logp", logp)):
        assert np.allclose(g[k], v, rtol=0, atol=1e-10), k
    wm = A.enumerated(plan, tensors, x, order, states, positions=[14, 15])[0]
    assert float((wm - torch.from_numpy(lm[:, 14:])).abs().max()) < 1e-9
    _, c32, l32 = A.restated(plan, tensors, x, order, states, dtype=torch.float32)
    wc = torch.from_numpy(cond)
    pairs = A.kept_pairs(wc, x, order)
    fc, fl = A.frac_of_bound(c32, wc, A.kept_states(wc)), A.frac_of_bound(l32, torch.from_numpy(logp), pairs)
    print(f"categorical fixture: conditionals {fc:.3f}, log probabilities {fl:.3f} of the bound; {int(pairs.sum())} of 48 pairs kept")
    assert fc < 0.25 and fl < 0.25


def test_the_entry_point_refuses_bad_host_words_before_it_launches():
    from cirkit_amd import _capi as capi

    lib = capi.load()
    assert lib.ck_abi_version() == 51 and "ck_squared_path_steps" in capi.SIGNATURES
    W = capi.CK_SQ_PATH_LEVEL_WORDS + 2
    lev = np.zeros((2, 1, W), dtype=np.int64)
    leaf = np.zeros((2, capi.CK_SQ_STEP_LEAF_WORDS), dtype=np.int64)
    fake = 4096  # (an address nobody reads: every call below is refused on the host words)
    lev[:, 0, :7] = (capi.CK_SQ_PATH_STAGES, 0, 3, 1, fake, fake, 1)
    lev[:, 0, 8:10] = (capi.CK_SQ_RANK1, 0)
    leaf[:] = (fake, 0, 3, 3, 0, 1, 1, 0)

    def call(lev=lev, leaf=leaf, step0=0, n=2, out=fake, rank1=fake, C=3, D=4, lm_step=3):
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        return lib.ck_squared_path_steps(None, None, rank1, p(lev), fake, W, 1, p(leaf), fake, step0, n, fake, D, None, out, 2 * lm_step, lm_step,
                                         None, 0, 0, None, 0, 0, C, 2, 1, 0, None)

    for kw, word in (({"out": None}, b"no output"), ({"n": 0}, b"bad sizes"), ({"rank1": None}, b"null pointer"), ({"C": 2}, b"leaf words"),
                     ({"D": 1}, b"leaf words"), ({"lm_step": 2}, b"output strides")):
        assert call(**kw) == -1
        assert b"ck_squared_path_steps" in lib.ck_last_error() and word in lib.ck_last_error(), lib.ck_last_error()
    bad = lev.copy()
    bad[1, 0, 2] = 5  # the second step's path ends on 5 units, its input fold has 3
    assert call(lev=bad) == -1 and b"step 1" in lib.ck_last_error()
    bad = lev.copy()
    bad[1, 0, 8] = 7
    assert call(lev=bad) == -1 and b"child kind" in lib.ck_last_error()
    bad = leaf.copy()
    bad[0, 6] = 2  # more levels than a step has room for
    assert call(leaf=bad) == -1 and b"leaf words" in lib.ck_last_error()
