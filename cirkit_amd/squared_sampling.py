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
from .plan import Plan, resolve_fold_index
from .squared import INTEGRATED, MIXED, OBSERVED, _CHUNK_BYTES, MixedPlan, _mask_of, mixed_plan

_HEAD = capi.CK_SQ_PATH_LEVEL_WORDS


@dataclass
class PathLevel:
    """One ancestor of a variable: fold `fold` of layer `layer`, which reads the fold below it on the path in child slot
    `slot` and the `siblings` ``(layer, fold)`` in its other slots."""

    layer: int
    fold: int
    slot: int
    siblings: list[tuple[int, int]]


@dataclass
class PathPlan:
    var: int
    leaf: tuple[int, int]  # the input fold that reads the variable
    levels: list[PathLevel]  # root first

    def folds(self) -> set[tuple[int, int]]:
        return {self.leaf} | {(lv.layer, lv.fold) for lv in self.levels}


def _children(plan: Plan):
    folds = [l.num_folds for l in plan.layers]
    return [None if l.inputs is None else resolve_fold_index(l.inputs, folds) for l in plan.layers]


def _output_fold(plan: Plan) -> tuple[int, int]:
    p, f = resolve_fold_index(plan.output, [l.num_folds for l in plan.layers]).reshape(-1, 2)[0]
    return int(p), int(f)


def _readers(plan: Plan) -> dict[tuple[int, int], list[tuple[int, int, int]]]:
    """``(layer, fold)`` -> the ``(layer, fold, slot)`` that read it."""
    out: dict[tuple[int, int], list[tuple[int, int, int]]] = {}
    for i, ch in enumerate(_children(plan)):
        if ch is None:
            continue
        for f in range(ch.shape[0]):
            for h in range(ch.shape[1]):
                out.setdefault((int(ch[f, h, 0]), int(ch[f, h, 1])), []).append((i, f, h))
    return out


def tree_order(plan: Plan) -> list[int]:
    """The variables in the order a depth-first walk of the fold tree below the output meets them.  Sampling in this order,
    every sibling of a fold on the path of the variable being drawn is entirely drawn or entirely still to draw."""
    children = _children(plan)
    order: list[int] = []
    seen: set[int] = set()
    stack = [_output_fold(plan)]
    while stack:
        p, f = stack.pop()
        if children[p] is None:
            for v in plan.layers[p].scope_idx[f]:
                if int(v) not in seen:
                    seen.add(int(v))
                    order.append(int(v))
            continue
        stack.extend((int(q), int(g)) for q, g in children[p][f][::-1])
    return order


def path_plan(plan: Plan, var: int, readers=None) -> PathPlan:
    """The ancestry of a variable, root first.  ``NotImplementedError`` unless it is a path: one input fold reads the
    variable and every fold on the way up has exactly one reader, up to the output fold (a region graph that is a tree)."""
    readers = _readers(plan) if readers is None else readers
    leaves = [(i, f) for i, l in enumerate(plan.layers) if l.inputs is None
              for f in range(l.num_folds) if int(var) in (int(v) for v in l.scope_idx[f])]
    if len(leaves) != 1:
        raise NotImplementedError(f"HipSquaredCircuit: variable {var} is read by {len(leaves)} input folds; sampling and all-state "
                                  "conditionals walk ONE path from the root to the variable (region graphs that are trees)")
    top = _output_fold(plan)
    levels: list[PathLevel] = []
    cur = leaves[0]
    children = _children(plan)
    while cur != top:
        rd = readers.get(cur, [])
        if len(rd) != 1:
            raise NotImplementedError(f"HipSquaredCircuit: fold {cur[1]} of layer {cur[0]} above variable {var} has {len(rd)} readers; "
                                      "sampling and all-state conditionals walk ONE path from the root to the variable (region graphs "
                                      "that are trees; a DAG such as a QuadGraph or Poon-Domingos is not supported)")
        i, f, h = rd[0]
        sib = [(int(p), int(g)) for k, (p, g) in enumerate(children[i][f]) if k != h]
        levels.append(PathLevel(i, f, h, sib))
        cur = (i, f)
    return PathPlan(int(var), leaves[0], levels[::-1])


def scope_bits(plan: Plan) -> list[list[int]]:
    """Per layer, per fold, the variables under it as the bits of an int."""
    out: list[list[int]] = []
    for l, ch in zip(plan.layers, _children(plan)):
        if ch is None:
            out.append([sum(1 << int(v) for v in row) for row in l.scope_idx])
        else:
            row_bits = []
            for row in ch:
                b = 0
                for p, g in row:
                    b |= out[int(p)][int(g)]
                row_bits.append(b)
            out.append(row_bits)
    return out


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
    dev: dict = field(default_factory=dict)  # batch size -> bound tables


def _check_discrete(sq) -> None:
    if any(l.inputs is None and l.type == "gaussian" for l in sq.plan.layers):
        raise NotImplementedError("HipSquaredCircuit: sampling and all-state conditionals of Gaussian input layers (no continuous "
                                  "inverse CDF); log_marginal and conditional_log_prob take them")


class _Sampler:
    """What the four queries share, kept on the `HipSquaredCircuit` (`sq._sampler`)."""

    def __init__(self, sq) -> None:
        self.sq = sq
        self.readers = _readers(sq.plan)
        self.bits = scope_bits(sq.plan)
        self.paths: dict[int, PathPlan] = {}
        self.orders: dict[bytes, OrderPlan] = {}
        self.fold_base = np.concatenate([[0], np.cumsum([l.num_folds for l in sq.plan.layers])])
        self._tree: list[int] | None = None

    def tree(self) -> list[int]:
        if self._tree is None:
            self._tree = tree_order(self.sq.plan)
        return self._tree

    def path(self, v: int) -> PathPlan:
        if v not in self.paths:
            self.paths[v] = path_plan(self.sq.plan, v, self.readers)
        return self.paths[v]

    # -- host plans ------------------------------------------------------------------------------------------------------------
    def _step(self, v: int, integrated: np.ndarray) -> StepPlan:
        """`integrated`: (D,) bool without v."""
        sq, path = self.sq, self.path(v)
        mbits = sum(1 << int(i) for i in np.nonzero(integrated)[0])
        views = sq._z_binding().views
        cls, need = [], False
        for lv in path.levels:
            row = []
            for p, g in lv.siblings:
                b = self.bits[p][g]
                c = OBSERVED if not (b & mbits) else (INTEGRATED if not (b & ~mbits) else MIXED)
                need = need or c == MIXED or (c == INTEGRATED and views[sq._z_of[p]] is None)
                row.append(c)
            cls.append(row)
        mp = None
        if need:
            m = integrated.copy()
            m[v] = True
            mp = mixed_plan(sq.plan, m, lambda p: views[sq._z_of[p]] is not None, path=path.folds())
        return StepPlan(path, cls, mp)

    def order_plan(self, order: list[int], integrated: np.ndarray) -> OrderPlan:
        """The steps of drawing `order` one variable after the other; `integrated`: what stays integrated out throughout
        (nothing, for the samplers).  Cached on the bytes of both."""
        key = np.asarray(order, dtype=np.int64).tobytes() + b"|" + np.packbits(integrated).tobytes()
        op = self.orders.get(key)
        if op is None:
            for v in order:  # (the refusals come before anything is built)
                self.path(v)
            left = integrated.copy()
            left[order] = True
            steps = []
            for v in order:
                left[v] = False
                steps.append(self._step(v, left))
            if len(self.orders) >= 8:
                self.orders.pop(next(iter(self.orders)))
            op = self.orders[key] = OrderPlan(steps, max([len(lv.siblings) for s in steps for lv in s.path.levels] + [0]),
                                              max([len(s.path.levels) for s in steps] + [1]))
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
    def bind(self, op: OrderPlan, B: int, bd_c, bd_z) -> dict:
        """The level tables of every step at batch size B, stacked (steps, levels, words) on the host and on the device, the
        mixed launches of the steps that have any, and one mixed arena for all of them."""
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
        if hit is not None and hit["key"] == key:
            return hit
        W = _HEAD + 2 * op.max_siblings
        host = np.zeros((len(op.steps), op.max_levels, W), dtype=np.int64)
        launches, total, mid = [], 1, 0
        for si, s in enumerate(op.steps):
            bases, pos = {}, {}
            if s.mixed is not None:
                tb = sq._tables(s.mixed, B, bd_c, bd_z, alloc=False)
                launches.append(tb["launches"])
                total, mid = max(total, tb["total"]), max(mid, tb["mid_size"])
                bases = {la["layer"]: la["base"] for la in tb["launches"]}
                pos = {m.layer: {int(f): j for j, f in enumerate(m.folds)} for m in s.mixed.layers}
            else:
                launches.append(None)
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
                    if layers[p].num_output_units != K:
                        raise ValueError("a layer's children do not all have its number of input units")
                    if g in pos.get(p, {}):
                        kd, off = capi.CK_SQ_FULL, bases[p] + pos[p][g] * B * K * K
                    elif c == OBSERVED:
                        kd, off = capi.CK_SQ_RANK1, bd_c.views[p].storage_offset() + g * B * K
                    else:
                        kd, off = capi.CK_SQ_CONST, bd_z.views[sq._z_of[p]].storage_offset() + g * K * K
                    row[_HEAD + 2 * h], row[_HEAD + 2 * h + 1] = kd, off
        dt = torch.complex64 if sq._complex else torch.float32
        any_mixed = any(la is not None for la in launches)
        hit = op.dev[B] = dict(key=key, host=host, dev=torch.from_numpy(host).to(sq.device), launches=launches,
                               arena=torch.empty(total, dtype=dt, device=sq.device) if any_mixed else None,
                               mid=torch.empty(mid, dtype=dt, device=sq.device) if mid else None)
        if len(op.dev) > 2:
            op.dev.pop(next(iter(op.dev)))
        return hit

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
        tb = None
        for si, s in enumerate(op.steps):
            bd_c = sq.c._run(xw)
            if tb is None or tb["key"][0] != bd_c.arena.data_ptr():
                tb = self.bind(op, B, bd_c, bd_z)
            arena = tb["arena"]
            if tb["launches"][si] is not None:
                sq.last_mixed_launches += sq._launch_mixed(tb["launches"][si], arena, tb["mid"], bd_c, bd_z, B)
            pl, fl = s.path.leaf
            layer = sq.c.layers[pl]
            table = layer._table
            C = int(table.shape[1]) - 1
            if table.dtype != torch.float32 or not table.is_contiguous():
                raise NotImplementedError("HipSquaredCircuit: an input table that is not real fp32")
            L = len(s.path.levels)
            with torch.cuda.device(sq.device):
                capi.call("ck_squared_path_bwd", None if arena is None else arena.data_ptr(), bd_z.arena.data_ptr(), bd_c.arena.data_ptr(),
                          tb["host"][si].ctypes.data if L else None, tb["dev"][si].data_ptr() if L else None, L, op.max_siblings,
                          table.data_ptr(), fl, C, int(table.shape[2]), 1 if sq.plan.layers[pl].type == "categorical" else 0,
                          None if log_m is None else log_m.data_ptr(), xw.data_ptr(), None if out is None else out.data_ptr(),
                          None if dead is None else dead.data_ptr(), D, s.path.var, int(self.fold_base[pl]) + fl, seed, row0, B,
                          sq.rows_per_block, 1 if sq._complex else 0, stream)

    def num_states(self, v: int) -> int:
        pl, _ = self.path(v).leaf
        cfg = self.sq.plan.layers[pl].config
        return int(cfg.get("num_states", cfg.get("num_categories", 0)))

    def clean(self, x: torch.Tensor, ignored: np.ndarray):
        """x on the device as int64 with 0 where it is ignored or absent; (B,) bool: rows with an absent OBSERVED entry."""
        sq = self.sq
        D = sq.plan.num_variables
        if x.dim() != 2 or x.shape[1] != D:
            raise ValueError(f"expected x of shape (B, {D}), found {tuple(x.shape)}")
        x = x.to(sq.device).to(torch.int64)
        mask = torch.from_numpy(ignored).to(sq.device)
        absent = x < 0
        return torch.where(mask | absent, torch.zeros((), dtype=torch.int64, device=sq.device), x).contiguous(), (absent & ~mask).any(dim=1)

    def chunk_rows(self, op: OrderPlan, rows_per_chunk) -> int:
        step = int(rows_per_chunk) if rows_per_chunk is not None else max(1, _CHUNK_BYTES // self.row_bytes(op))
        if step <= 0:
            raise ValueError("rows_per_chunk must be positive")
        return step


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
    xw, bad = sm.clean(x, ignored)
    B = int(xw.shape[0])
    out = torch.empty((B, sm.num_states(var)), dtype=torch.float32, device=sq.device)
    step = sm.chunk_rows(op, rows_per_chunk)
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
        order = [v for v in sm.tree() if drawn[v]]
    order = [int(v) for v in order]
    if sorted(order) != np.nonzero(drawn)[0].tolist():
        raise ValueError("order must be a permutation of the sampled variables")
    xw, bad = sm.clean(x, drawn)
    out = x.to(sq.device).to(torch.int64).clone()
    if not order:
        return out
    seed = _seed(seed)
    op = sm.order_plan(order, np.zeros(D, dtype=bool))
    dead = bad.to(torch.int32).contiguous()
    B = int(xw.shape[0])
    step = sm.chunk_rows(op, rows_per_chunk)
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
