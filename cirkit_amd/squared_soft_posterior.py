"""Posteriors and sampling under soft evidence of a squared circuit ``p(x) = |c(x)|^2 / Z`` on the GPU:
`HipSquaredCircuit.soft_query_log_marginals`, `soft_posterior_marginals` and `sample_soft` ("Posteriors and
sampling under soft evidence of squared circuits").  Thin over cirkit_amd/squared_soft.py and cirkit_amd/squared_posterior.py.

With a weight per state ``lambda_v`` on every variable of ``S``, ``I`` integrated out and the rest observed,

    ``m_b(v, s) = lambda_v(s) sum_{x: x_v = s} |c(x)|^2 prod_{u in S - v} lambda_u(x_u) = lambda_v(s) sum_kl G_b^v[k, l] a_k(s) conj(a_l(s))``

for every ``v`` in ``S`` at once.  The down pass of `posterior_marginals` computes "all children but this one" at every fold, so
walked over a SOFT bottom-up pass (`mixed_plan(..., soft=, readers=)`: every fold above a soft variable at ``K^2`` units, the
leaf Gram blocks FULL children) the ``G`` that reaches the input fold of ``v`` holds every other variable's weight and not
``lambda_v``, which the leaf launch adds (`ck_squared_soft_down_leaf`, cirkit_amd/csrc/ck_sqsoftdown.hip).  One chunk: ``c``'s
forward, the leaf Gram launches, the mixed launches, the root (the evidence), the `ck_squared_down_bwd` launches, the leaf launch.

`sample_soft` draws the soft variables one after the other (`squared_sampling._Sampler`): one soft bottom-up pass per chunk,
whose arena stays alive, then per variable ``c``'s forward on the rows with the draws written in and one path launch
(`ck_squared_path_soft_bwd`) that adds the variable's own weights.  A sibling of the path holds either no drawn soft variable --
its value from the soft pass is still valid -- or no undrawn one -- it is classified as `sample_conditional` classifies it;
an order that leaves a sibling partly drawn is refused while planning.

Out of scope: MPE under soft evidence (not tractable for squared circuits); posteriors of variables that carry no weight (pass
``log_lik = 0`` for them); boxes read from their bounds (pass the 0 / ``-inf`` weights); per-row soft sets; orders that leave a
sibling partly drawn; Gaussian inputs; gradients; moving `posterior_marginals` itself onto the MFMA leaf.
"""

from __future__ import annotations

import numpy as np
import torch

from . import _capi as capi
from . import squared_posterior as P
from .squared import put_bounded
from .squared_sampling import sampler
from .squared_soft import _rows, _sets, launch_leaves, soft_plan, soft_weights


def plan_of(sq, soft: np.ndarray, integrate: np.ndarray) -> P.DownPlan:
    """The `DownPlan` of a call -- the down folds of ``S``, its soft mixed plan under ``I`` -- cached on (I, S).  Refuses what
    `squared_posterior.host_plan` refuses: a variable read by several input folds, a fold above one with several readers."""
    sampler(sq)  # (Gaussian inputs are refused here)
    key = (np.packbits(integrate).tobytes(), np.packbits(soft).tobytes())
    dp = sq._soft_down_plans.get(key)
    if dp is None:
        ids = np.nonzero(soft)[0].tolist()
        for v in ids:  # (the refusals come before the partition-function circuit is evaluated)
            sq.graph.path(v)
        dp = put_bounded(sq._soft_down_plans, key, P.host_plan(sq.plan, ids, integrate, sq._const_available(), sq.graph, soft=soft), 8)
    return dp


def row_bytes(sq, dp: P.DownPlan) -> int:
    """Bytes per row of c's arena, the mixed arena with its leaf blocks, and the down arena."""
    return P.row_bytes(sq, dp)


def _arguments(sq, log_lik, x, soft_vars, integrate_vars):
    """What the three queries check before anything is allocated, as `soft_evidence_log_prob` checks it: the sets, ``log_lik``
    (`squared_soft.soft_weights`); `rows()` then cleans ``x``."""
    soft, integrate = _sets(sq, soft_vars, integrate_vars, "soft evidence")
    B, states, weights = soft_weights(sq, log_lik, soft)
    return soft, integrate, B, states, weights, lambda: _rows(sq, x, B, soft, integrate)


def _chunk(sq, dp: P.DownPlan, xw: torch.Tensor, ll: torch.Tensor, out: torch.Tensor, ev: torch.Tensor, form: int, mark) -> None:
    """The cleaned rows `xw` (B, D) and their weights `ll` (B, |S|, Cl): ``log m`` into `out` (B, |S|, C), the unnormalised log
    evidence into `ev` (B,)."""
    B = int(xw.shape[0])
    bd_c = sq.c._run(xw)
    mark("c_forward")
    bd_z = sq._z_binding()
    tb = sq._tables(dp.mixed, B, bd_c, bd_z)
    sq.last_soft_launches += launch_leaves(sq, tb, B, ll, None, None)
    mark("soft_leaves")
    sq.last_launches += sq._launch_mixed(tb.launches, tb.arena, tb.mid, bd_c, bd_z, B)
    mark("mixed")
    ev.copy_(sq._mixed_root(tb, dp.mixed, B))  # (the output fold holds a soft variable: it is evaluated)
    bt = P.bind(sq, dp, B, bd_c, bd_z, tb, positions=np.arange(len(dp.qvars)))
    down = P._down_arena(sq, bt.total)
    P.launch_down(sq, bt, tb.arena, down, bd_c, bd_z, B)
    mark("down")
    with torch.cuda.device(sq.device):
        capi.call("ck_squared_soft_down_leaf", down.data_ptr(), down.numel(), bt.vars_host.ctypes.data, bt.vars_dev.data_ptr(),
                  len(dp.qvars), int(out.shape[2]), ll.data_ptr(), int(ll.shape[1]), int(ll.shape[2]), out.data_ptr(), B,
                  sq.rows_per_block, 1 if sq._complex else 0, form, torch.cuda.current_stream(sq.device).cuda_stream)
    mark("leaf")
    sq.last_down_launches += len(bt.launches) + 1


def soft_query_log_marginals(sq, log_lik, x=None, *, soft_vars=None, integrate_vars=None, normalized=True, return_log_evidence=False,
                             rows_per_chunk=None, form: int = 0, mark=None):
    """`form` 1 forces the plain leaf launch; `mark`: called with the name of each phase when its launches have been issued
    (scripts/bench_squared_soft_posterior.py)."""
    soft, integrate, B, states, weights, rows = _arguments(sq, log_lik, x, soft_vars, integrate_vars)
    dp = plan_of(sq, soft, integrate)
    xw, bad = rows()
    step = sq._chunk_rows(rows_per_chunk, lambda: row_bytes(sq, dp))
    out = torch.empty((B, len(dp.qvars), states), dtype=torch.float32, device=sq.device)
    ev = torch.empty(B, dtype=torch.float32, device=sq.device)
    sq.last_launches = sq.last_soft_launches = sq.last_down_launches = 0
    mark = mark or (lambda name: None)
    for r0 in range(0, B, step):
        ll, wrong = weights(r0, r0 + step)
        _chunk(sq, dp, xw[r0: r0 + step], ll, out[r0: r0 + step], ev[r0: r0 + step], form, mark)
        bad[r0: r0 + step] |= wrong
    if normalized:
        lz = sq._root_of_z()
        out, ev = out - lz, ev - lz
    nan = torch.full((), float("nan"), device=sq.device)
    out = torch.where(bad[:, None, None], nan, out)
    return (out, torch.where(bad, nan, ev)) if return_log_evidence else out


def soft_posterior_marginals(sq, log_lik, x=None, *, soft_vars=None, integrate_vars=None, return_log_evidence=False, rows_per_chunk=None,
                             form: int = 0):
    lm, ev = soft_query_log_marginals(sq, log_lik, x, soft_vars=soft_vars, integrate_vars=integrate_vars, normalized=False,
                                      return_log_evidence=True, rows_per_chunk=rows_per_chunk, form=form)
    post = lm - torch.logsumexp(lm, dim=2, keepdim=True)
    return (post, ev - sq._root_of_z()) if return_log_evidence else post


def sample_soft(sq, log_lik, x=None, *, soft_vars=None, integrate_vars=None, seed=None, order=None, rows_per_chunk=None) -> torch.Tensor:
    from .sampling import _seed

    sm = sampler(sq)  # (Gaussian inputs are refused here)
    soft, integrate, B, _, weights, rows = _arguments(sq, log_lik, x, soft_vars, integrate_vars)
    ids = np.nonzero(soft)[0].tolist()
    if order is None:
        order = [v for v in sq.graph.tree_order() if soft[v]]
    order = [int(v) for v in order]
    if sorted(order) != ids:
        raise ValueError("order must be a permutation of the soft variables")
    # (the tree refusals, and an order that leaves a sibling partly drawn, are refused here, before anything is allocated)
    op = sm.order_plan(order, integrate, soft=soft)
    # the soft pass of `soft_evidence_log_prob`, not the down plan's: a path launch reads the siblings of ONE path, all of which meet
    # S or are classified by the step; the down folds' further children (`readers=`) would be evaluated for nobody
    mp = soft_plan(sq, integrate, soft)
    xw, bad = rows()
    D = sq.plan.num_variables
    out = torch.zeros((B, D), dtype=torch.int64, device=sq.device) if x is None else x.to(sq.device).to(torch.int64).clone()
    seed = _seed(seed)
    step = sq._chunk_rows(rows_per_chunk, lambda: sm.row_bytes(op, mp))
    sq.last_launches = sq.last_soft_launches = sq.last_mixed_launches = 0
    dead = torch.empty(B, dtype=torch.int32, device=sq.device)
    for r0 in range(0, B, step):
        ll, wrong = weights(r0, r0 + step)
        dead[r0: r0 + step] = (bad[r0: r0 + step] | wrong).to(torch.int32)
        sm.run(op, xw[r0: r0 + step], out=out[r0: r0 + step], dead=dead[r0: r0 + step], seed=seed, row0=r0, soft=mp, log_lik=ll)
    return out
