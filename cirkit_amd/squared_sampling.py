"""Exact sampling and all-state conditionals of a squared circuit ``p(x) = |c(x)|^2 / Z`` (`HipSquaredCircuit`).

A squared circuit is not monotonic -- a sum of ``c`` may carry a negative weight -- so no top-down walk samples it.  The exact
sampler is autoregressive: draw ``x_{o_0}``, then ``x_{o_1} | x_{o_0}``, ...; each step needs the marginal of ONE variable
``v`` over ALL its states with the earlier variables observed and the later ones integrated out,

    ``m_b(s) = integral of |c(x_O, X_v = s, x_M)|^2 dx_M = sum_kl G_b[k, l] a_k(s) conj(a_l(s))``,

``a_k(s)`` the value of unit ``k`` of the input fold that reads ``v`` and ``G_b`` the derivative of the root of the product
circuit with respect to that fold's ``K^2`` squared units: the product circuit is multilinear in them.  ``G`` is walked from
the root down the ancestors of ``v`` by ONE launch per step (`ck_squared_path_bwd`, cirkit_amd/csrc/ck_sqpath.hip), which also
evaluates the ``C`` states and draws.  The other children of the ancestors are read by kind, as the mixed pass reads them
(cirkit_amd/squared.py); in the depth-first order of ``c``'s fold tree (`tree_order`) every one of them is entirely sampled or
entirely integrated at every step, so a step is ``c``'s forward plus that launch.  With another order, or scattered
evidence, the mixed ones are evaluated first by the `ck_squared_mixed_fwd` launches of the mixed pass.

Only path-shaped ancestries: the variable is read by exactly one input fold and every ancestor has exactly one reader (trees:
QuadTree, linear, random binary).  A DAG (QuadGraph, Poon-Domingos) is refused by `path_plan`.  Gaussian inputs are refused
(no continuous inverse CDF).  Out of scope: per-row masks or orders, recomputing only the changed ancestors in ``c``'s forward
between two steps, fusing that forward with the path launch.
"""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

from . import _capi as capi
from .squared import INTEGRATED, MIXED, MixedPlan, _mask_of, mixed_plan, put_bounded
from .squared_graph import PathLevel, PathPlan, fold_class, mask_bits, path_plan, scope_bits, tree_order  # noqa: F401 (also for callers)

_HEAD = capi.CK_SQ_PATH_LEVEL_WORDS


@dataclass
class StepPlan:
    """One step: the path of its variable, per (level, sibling) the class of the sibling for the step's integrated set, and
    the mixed folds (if any) the siblings need evaluated first."""

    path: PathPlan
    cls: list[list[int]]
    mixed: MixedPlan | None


@dataclass
class OrderPlan:
    steps: list[StepPlan]
    max_siblings: int
    max_levels: int
    dev: dict = field(default_factory=dict)  # batch size -> `PathTables`


@dataclass
class PathTables:
    """The level tables of every step of an order at a batch size, stacked (steps, levels, words) on the host and on the
    device, the mixed launches of the steps that have any, and one mixed arena for all of them."""

    key: tuple
    host: np.ndarray
    dev: torch.Tensor
    launches: list  # per step a list of `MixedLaunch`, or None
    arena: torch.Tensor | None
    mid: torch.Tensor | None


def _check_discrete(sq) -> None:
    if any(l.inputs is None and l.type == "gaussian" for l in sq.plan.layers):
        raise NotImplementedError("HipSquaredCircuit: sampling and all-state conditionals of Gaussian input layers (no continuous "
                                  "inverse CDF); log_marginal and conditional_log_prob take them")


class _Sampler:
    """What the four queries share, kept on the `HipSquaredCircuit` (`sq._sampler`)."""

    def __init__(self, sq) -> None:
        self.sq = sq
        self.graph = sq.graph
        self.orders: dict[bytes, OrderPlan] = {}

    # -- host plans ------------------------------------------------------------------------------------------------------------
    def _step(self, v: int, integrated: np.ndarray) -> StepPlan:
        """`integrated`: (D,) bool without v."""
        sq, path = self.sq, self.graph.path(v)
        mbits = mask_bits(integrated)
        const = sq._const_available()
        cls = [[fold_class(self.graph.bits[p][g], mbits) for p, g in lv.siblings] for lv in path.levels]
        need = any(c == MIXED or (c == INTEGRATED and not const(p))
                   for lv, row in zip(path.levels, cls) for (p, _), c in zip(lv.siblings, row))
        mp = None
        if need:
            m = integrated.copy()
            m[v] = True
            mp = mixed_plan(sq.plan, m, const, path=path.folds(), graph=self.graph)
        return StepPlan(path, cls, mp)

    def order_plan(self, order: list[int], integrated: np.ndarray) -> OrderPlan:
        """The steps of drawing `order` one variable after the other; `integrated`: what stays integrated out throughout
        (nothing, for the samplers).  Cached on the bytes of both."""
        key = np.asarray(order, dtype=np.int64).tobytes() + b"|" + np.packbits(integrated).tobytes()
        op = self.orders.get(key)
        if op is None:
            for v in order:  # (the refusals come before anything is built)
                self.graph.path(v)
            left = integrated.copy()
            left[order] = True
            steps = []
            for v in order:
                left[v] = False
                steps.append(self._step(v, left))
            op = put_bounded(self.orders, key, OrderPlan(steps, max([len(lv.siblings) for s in steps for lv in s.path.levels] + [0]),
                                                         max([len(s.path.levels) for s in steps] + [1])), 8)
        return op

    def row_bytes(self, op: OrderPlan) -> int:
        sq = self.sq
        n = sum(l.num_folds * l.num_output_units for l in sq.plan.layers)
        extra = 0
        for s in op.steps:
            if s.mixed is not None:
                extra = max(extra, sq._row_bytes(s.mixed) // sq._esize - n)
        return (n + extra) * sq._esize

    # -- device tables -----------------------------------------------------------------------------------------------------------
    def bind(self, op: OrderPlan, B: int, bd_c, bd_z) -> PathTables:
        """The `PathTables` of an order at batch size B."""
        sq = self.sq
        layers = sq.plan.layers
        weights = {}
        for s in op.steps:
            for lv in s.path.levels:
                l = layers[lv.layer]
                if l.type != "hadamard" and lv.layer not in weights:
                    weights[lv.layer] = sq._stage_weights(lv.layer, l.num_output_units, l.num_input_units)
        key = (bd_c.arena.data_ptr(), bd_z.arena.data_ptr(), tuple(w.data_ptr() for ws in weights.values() for w in ws))
        hit = op.dev.get(B)
        if hit is not None and hit.key == key:
            return hit
        W = _HEAD + 2 * op.max_siblings
        host = np.zeros((len(op.steps), op.max_levels, W), dtype=np.int64)
        launches, total, mid = [], 1, 0
        for si, s in enumerate(op.steps):
            tb = None if s.mixed is None else sq._tables(s.mixed, B, bd_c, bd_z, alloc=False)
            launches.append(None if tb is None else tb.launches)
            if tb is not None:
                total, mid = max(total, tb.total), max(mid, tb.mid_size)
            for li, lv in enumerate(s.path.levels):
                l = layers[lv.layer]
                K = l.num_input_units
                row = host[si, li]
                if l.type != "hadamard":
                    w1, w2 = weights[lv.layer]
                    row[0], row[3], row[4], row[5] = capi.CK_SQ_PATH_STAGES, l.num_output_units, w1.data_ptr(), w2.data_ptr()
                else:
                    row[3] = K
                row[1], row[2], row[6] = lv.fold, K, len(lv.siblings)
                for h, ((p, g), c) in enumerate(zip(lv.siblings, s.cls[li])):
                    row[_HEAD + 2 * h: _HEAD + 2 * h + 2] = sq.child(p, g, K, B, c, tb, bd_c, bd_z)
        dt = torch.complex64 if sq._complex else torch.float32
        any_mixed = any(la is not None for la in launches)
        return put_bounded(op.dev, B, PathTables(key, host, torch.from_numpy(host).to(sq.device), launches,
                                                 torch.empty(total, dtype=dt, device=sq.device) if any_mixed else None,
                                                 torch.empty(mid, dtype=dt, device=sq.device) if mid else None), 2)

    # -- the steps ---------------------------------------------------------------------------------------------------------------
    def run(self, op: OrderPlan, xw: torch.Tensor, *, out: torch.Tensor | None = None, dead: torch.Tensor | None = None,
            log_m: torch.Tensor | None = None, seed: int = 0, row0: int = 0) -> None:
        """Every step of `op` on the rows `xw` (B, D) int64, contiguous, negative entries cleaned: c's forward, the mixed
        launches the step needs, the path launch -- which writes ``log m`` into `log_m` (B, C) and / or draws into column v
        of `out` and of `xw` itself, so that the next forward reads the draw.  Nothing here waits for the device."""
        sq = self.sq
        B, D = int(xw.shape[0]), int(xw.shape[1])
        bd_z = sq._z_binding()
        stream = torch.cuda.current_stream(sq.device).cuda_stream
        fold_base = self.graph.fold_base
        tb = None
        for si, s in enumerate(op.steps):
            bd_c = sq.c._run(xw)
            if tb is None or tb.key[0] != bd_c.arena.data_ptr():
                tb = self.bind(op, B, bd_c, bd_z)
            arena = tb.arena
            if tb.launches[si] is not None:
                sq.last_mixed_launches += sq._launch_mixed(tb.launches[si], arena, tb.mid, bd_c, bd_z, B)
            pl, fl = s.path.leaf
            table, C, K, tlog = sq._leaf_table(pl)
            L = len(s.path.levels)
            with torch.cuda.device(sq.device):
                capi.call("ck_squared_path_bwd", None if arena is None else arena.data_ptr(), bd_z.arena.data_ptr(), bd_c.arena.data_ptr(),
                          tb.host[si].ctypes.data if L else None, tb.dev[si].data_ptr() if L else None, L, op.max_siblings,
                          table.data_ptr(), fl, C, K, tlog, None if log_m is None else log_m.data_ptr(), xw.data_ptr(),
                          None if out is None else out.data_ptr(), None if dead is None else dead.data_ptr(), D, s.path.var,
                          int(fold_base[pl]) + fl, seed, row0, B, sq.rows_per_block, 1 if sq._complex else 0, stream)


def sampler(sq) -> _Sampler:
    if getattr(sq, "_sampler", None) is None:
        _check_discrete(sq)
        sq._sampler = _Sampler(sq)
    return sq._sampler


def state_log_marginals(sq, x, var, integrate_vars=None, *, normalized=True, rows_per_chunk=None) -> torch.Tensor:
    sm = sampler(sq)
    D = sq.plan.num_variables
    var = int(var)
    if not 0 <= var < D:
        raise ValueError("The variable must be in the circuit scope")
    mask = _mask_of(integrate_vars, D)
    if mask[var]:
        raise ValueError("a query variable cannot be integrated out")
    op = sm.order_plan([var], mask)
    ignored = mask.copy()
    ignored[var] = True
    xw, bad = sq._clean(x, ignored)
    B = int(xw.shape[0])
    out = torch.empty((B, sq.graph.num_states(var)), dtype=torch.float32, device=sq.device)
    step = sq._chunk_rows(rows_per_chunk, lambda: sm.row_bytes(op))
    sq.last_mixed_launches = 0
    for r0 in range(0, B, step):
        sm.run(op, xw[r0: r0 + step], log_m=out[r0: r0 + step])
    if normalized:
        out = out - sq._root_of_z()
    return torch.where(bad[:, None], torch.full((), float("nan"), device=sq.device), out)


def posterior(sq, x, var, integrate_vars=None, *, rows_per_chunk=None) -> torch.Tensor:
    lm = state_log_marginals(sq, x, var, integrate_vars, normalized=False, rows_per_chunk=rows_per_chunk)
    return lm - torch.logsumexp(lm, dim=1, keepdim=True)


def sample_conditional(sq, x, sample_vars, *, seed=None, order=None, rows_per_chunk=None) -> torch.Tensor:
    from .sampling import _seed

    sm = sampler(sq)
    D = sq.plan.num_variables
    drawn = _mask_of(sample_vars, D, "sample")
    if order is None:
        order = [v for v in sq.graph.tree_order() if drawn[v]]
    order = [int(v) for v in order]
    if sorted(order) != np.nonzero(drawn)[0].tolist():
        raise ValueError("order must be a permutation of the sampled variables")
    xw, bad = sq._clean(x, drawn)
    out = x.to(sq.device).to(torch.int64).clone()
    if not order:
        return out
    seed = _seed(seed)
    op = sm.order_plan(order, np.zeros(D, dtype=bool))
    dead = bad.to(torch.int32).contiguous()
    B = int(xw.shape[0])
    step = sq._chunk_rows(rows_per_chunk, lambda: sm.row_bytes(op))
    sq.last_mixed_launches = 0
    for r0 in range(0, B, step):
        sm.run(op, xw[r0: r0 + step], out=out[r0: r0 + step], dead=dead[r0: r0 + step], seed=seed, row0=r0)
    return out


def sample(sq, num_samples, *, seed=None, order=None, rows_per_chunk=None) -> torch.Tensor:
    if int(num_samples) <= 0:
        raise ValueError("num_samples must be positive")
    sampler(sq)  # (the refusals come before the batch is allocated)
    D = sq.plan.num_variables
    x = torch.zeros((int(num_samples), D), dtype=torch.int64, device=sq.device)
    return sample_conditional(sq, x, torch.ones(D, dtype=torch.bool), seed=seed, order=order, rows_per_chunk=rows_per_chunk)
