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
UNDRAWN = 3  # beside OBSERVED / INTEGRATED / MIXED: a sibling whose soft variables are all still to draw (`sample_soft`)


@dataclass
class StepPlan:
    """One step: the path of its variable, per (level, sibling) the class of the sibling for the step's integrated set (UNDRAWN:
    read from the soft pass of the chunk), and the mixed folds (if any) the siblings need evaluated first."""

    path: PathPlan
    cls: list[list[int]]
    mixed: MixedPlan | None


@dataclass
class OrderPlan:
    steps: list[StepPlan]
    max_siblings: int
    max_levels: int
    dev: dict = field(default_factory=dict)  # batch size -> `PathTables`
    soft_pos: dict | None = None  # (`sample_soft`) variable -> its position on the S axis of log_lik


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
    base: int = 0  # (`sample_soft`) where the steps' own mixed folds start in `arena`: behind the soft pass's
    soft: object = None  # (`sample_soft`) the `MixedTables` of the soft pass, without buffers of its own
    leaf: object = None  # (squared_autoregressive.py) the per-step leaf words of `ck_squared_path_steps`: (key, host, device)


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
    def _step(self, v: int, integrated: np.ndarray, undrawn: np.ndarray | None = None, drawn: np.ndarray | None = None) -> StepPlan:
        """`integrated`: (D,) bool without v.  `undrawn` / `drawn` (`sample_soft`): the soft variables still to draw after v and
        those drawn before it.  A sibling that holds undrawn ones and no drawn one is UNDRAWN: its value is the soft pass's.  One
        that holds no undrawn one is classified against `integrated` as ever.  One that holds both is refused."""
        sq, path = self.sq, self.graph.path(v)
        mbits = mask_bits(integrated)
        ubits = 0 if undrawn is None else mask_bits(undrawn)
        dbits = 0 if drawn is None else mask_bits(drawn)
        const = sq._const_available()
        cls = []
        for lv in path.levels:
            row = []
            for p, g in lv.siblings:
                b = self.graph.bits[p][g]
                if b & ubits and b & dbits:
                    raise NotImplementedError(f"HipSquaredCircuit.sample_soft: when variable {v} is drawn, fold {g} of layer {p} beside its "
                                              "path holds soft variables that are drawn and others that are not; the order must draw "
                                              "all soft variables of a sibling before or after the variable (tree_order does)")
                row.append(UNDRAWN if b & ubits else fold_class(b, mbits))
            cls.append(row)
        need = any(c == MIXED or (c == INTEGRATED and not const(p))
                   for lv, row in zip(path.levels, cls) for (p, _), c in zip(lv.siblings, row))
        mp = None
        if need:
            m = integrated.copy()
            m[v] = True
            mp = mixed_plan(sq.plan, m, const, path=path.folds(), graph=self.graph)
        return StepPlan(path, cls, mp)

    def order_plan(self, order: list[int], integrated: np.ndarray, soft: np.ndarray | None = None) -> OrderPlan:
        """The steps of drawing `order` one variable after the other; `integrated`: what stays integrated out throughout
        (nothing, for the samplers).  `soft` (`sample_soft`): `order` is a permutation of these variables, which carry a weight
        per state: the ones still to draw are not integrated but read from the soft pass.  Cached on the bytes of all three."""
        key = np.asarray(order, dtype=np.int64).tobytes() + b"|" + np.packbits(integrated).tobytes()
        if soft is not None:
            key += b"|soft|" + np.packbits(soft).tobytes()
        op = self.orders.get(key)
        if op is None:
            for v in order:  # (the refusals come before anything is built)
                self.graph.path(v)
            left = integrated.copy()
            steps = []
            if soft is None:
                left[order] = True
                for v in order:
                    left[v] = False
                    steps.append(self._step(v, left))
            else:
                undrawn, drawn = soft.copy(), np.zeros_like(soft)
                for v in order:
                    undrawn[v] = False
                    steps.append(self._step(v, left, undrawn, drawn))
                    drawn[v] = True
            op = put_bounded(self.orders, key, OrderPlan(steps, max([len(lv.siblings) for s in steps for lv in s.path.levels] + [0]),
                                                         max([len(s.path.levels) for s in steps] + [1])), 8)
            if soft is not None:
                op.soft_pos = {int(v): j for j, v in enumerate(np.nonzero(soft)[0])}
        return op

    def row_bytes(self, op: OrderPlan, soft: MixedPlan | None = None) -> int:
        """Bytes per row of c's arena and the largest mixed arena of a step; with `soft`, the soft pass's arena in front of it."""
        sq = self.sq
        n = sum(l.num_folds * l.num_output_units for l in sq.plan.layers)
        extra = 0
        for s in op.steps:
            if s.mixed is not None:
                extra = max(extra, sq._row_bytes(s.mixed) // sq._esize - n)
        return (n + extra) * sq._esize + (0 if soft is None else sq._row_bytes(soft) - n * sq._esize)

    # -- device tables -----------------------------------------------------------------------------------------------------------
    def bind(self, op: OrderPlan, B: int, bd_c, bd_z, soft: MixedPlan | None = None) -> PathTables:
        """The `PathTables` of an order at batch size B.  `soft` (`sample_soft`): the mixed plan of the chunk's soft pass; its
        arena is the front of the one arena the path launches read, the steps' own mixed folds lie behind it (`PathTables.base`)."""
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
        stb = None if soft is None else sq._tables(soft, B, bd_c, bd_z, alloc=False)
        base = 0 if stb is None else (stb.total + 3) // 4 * 4
        if stb is not None:
            mid = stb.mid_size
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
                    if c == UNDRAWN:  # the soft pass evaluated it (its scope meets the soft set): FULL in the front of the arena
                        kd, o = sq.child(p, g, K, B, MIXED, stb, bd_c, bd_z)
                        if kd != capi.CK_SQ_FULL:
                            raise RuntimeError(f"HipSquaredCircuit: the soft pass did not evaluate fold {g} of layer {p}")
                    else:
                        kd, o = sq.child(p, g, K, B, c, tb, bd_c, bd_z)
                        o += base if kd == capi.CK_SQ_FULL else 0
                    row[_HEAD + 2 * h: _HEAD + 2 * h + 2] = (kd, o)
        dt = torch.complex64 if sq._complex else torch.float32
        any_mixed = stb is not None or any(la is not None for la in launches)
        return put_bounded(op.dev, B, PathTables(key, host, torch.from_numpy(host).to(sq.device), launches,
                                                 torch.empty(base + total, dtype=dt, device=sq.device) if any_mixed else None,
                                                 torch.empty(mid, dtype=dt, device=sq.device) if mid else None, base, stb), 2)

    # -- the steps ---------------------------------------------------------------------------------------------------------------
    def run(self, op: OrderPlan, xw: torch.Tensor, *, out: torch.Tensor | None = None, dead: torch.Tensor | None = None,
            log_m: torch.Tensor | None = None, seed: int = 0, row0: int = 0, soft: MixedPlan | None = None,
            log_lik: torch.Tensor | None = None) -> None:
        """Every step of `op` on the rows `xw` (B, D) int64, contiguous, negative entries cleaned: c's forward, the mixed
        launches the step needs, the path launch -- which writes ``log m`` into `log_m` (B, C) and / or draws into column v
        of `out` and of `xw` itself, so that the next forward reads the draw.  Nothing here waits for the device.
        `soft`, `log_lik` (B, S, C) fp32 (`sample_soft`): behind the first forward -- nothing is drawn yet -- the soft pass of
        the chunk runs once into the front of the arena, which stays alive over the steps; every path launch then adds the
        weights of its own variable (`ck_squared_path_soft_bwd`)."""
        sq = self.sq
        B, D = int(xw.shape[0]), int(xw.shape[1])
        bd_z = sq._z_binding()
        stream = torch.cuda.current_stream(sq.device).cuda_stream
        fold_base = self.graph.fold_base
        tb = None
        for si, s in enumerate(op.steps):
            bd_c = sq.c._run(xw)
            if tb is None or tb.key[0] != bd_c.arena.data_ptr():
                if soft is not None and si > 0:
                    raise RuntimeError("HipSquaredCircuit: c's arena moved between two steps of a chunk; the soft pass's values are gone")
                tb = self.bind(op, B, bd_c, bd_z, soft)
            arena = tb.arena
            if soft is not None and si == 0:
                from .squared_soft import launch_leaves

                sq.last_soft_launches += launch_leaves(sq, tb.soft, B, log_lik, None, None, arena=arena)
                sq.last_launches += sq._launch_mixed(tb.soft.launches, arena, tb.mid, bd_c, bd_z, B)
            if tb.launches[si] is not None:
                sq.last_mixed_launches += sq._launch_mixed(tb.launches[si], arena[tb.base:] if tb.base else arena, tb.mid, bd_c, bd_z, B)
            pl, fl = s.path.leaf
            table, C, K, tlog = sq._leaf_table(pl)
            L = len(s.path.levels)
            head = (None if arena is None else arena.data_ptr(), bd_z.arena.data_ptr(), bd_c.arena.data_ptr(),
                    tb.host[si].ctypes.data if L else None, tb.dev[si].data_ptr() if L else None, L, op.max_siblings,
                    table.data_ptr(), fl, C, K, tlog)
            tail = (None if log_m is None else log_m.data_ptr(), xw.data_ptr(),
                    None if out is None else out.data_ptr(), None if dead is None else dead.data_ptr(), D, s.path.var,
                    int(fold_base[pl]) + fl, seed, row0, B, sq.rows_per_block, 1 if sq._complex else 0, stream)
            with torch.cuda.device(sq.device):
                if soft is None:
                    capi.call("ck_squared_path_bwd", *head, *tail)
                else:
                    capi.call("ck_squared_path_soft_bwd", *head, log_lik.data_ptr(), int(log_lik.shape[1]), int(log_lik.shape[2]),
                              op.soft_pos[s.path.var], *tail)


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
