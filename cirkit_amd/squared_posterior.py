"""Posterior marginals of a squared circuit ``p(x) = |c(x)|^2 / Z`` for a whole set of query variables at once
(`HipSquaredCircuit.query_log_marginals`, `posterior_marginals`).

For query variables ``Q``, further integrated variables ``I``, ``M = Q + I`` and the rest observed,

    ``m_b(v, s) = integral of |c(x_O, X_v = s, x_{M - v})|^2 dx_{M - v} = sum_kl G_b^v[k, l] a_k(s) conj(a_l(s))``

for every ``v`` in ``Q``: `state_log_marginals(x, v, M - v)`, whose walk from the root to ONE input fold
(cirkit_amd/squared_sampling.py) shares everything but the leaf with the walks of the other variables.  Here the derivative ``G``
is kept for every fold whose scope meets ``Q`` (the DOWN folds) and pushed down layer by layer: ``c``'s forward, the mixed pass under
``M`` (every sibling is read at its value with ALL of ``M`` integrated; its root is the evidence), one `ck_squared_down_bwd` launch
per layer of ``c`` that has down folds, from the output layer downwards, and one `ck_squared_down_leaf` launch for all the leaves
(cirkit_amd/csrc/ck_sqdown.hip).  The down arena holds ``K^2`` values per row for every down fold but the output fold, the input
folds included; nothing is released before the call ends.

Refused as `state_log_marginals` refuses: Gaussian inputs, and ancestries that are not paths (`path_plan`).  Out of scope:
leave-one-out conditionals (the other query variables observed: ``G`` is rank-1 there and has a K-sized pass of its own,
cirkit_amd/squared_loo.py; DESIGN.md section 11, "Leave-one-out conditionals of squared circuits"), per-row masks, DAG region graphs, complex parameter tensors, fusing ``c``'s forward or the mixed pass with the down
pass, gradients with respect to parameters.
"""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

from . import _capi as capi
from .plan import Plan
from .squared import INTEGRATED, MIXED, MixedPlan, MixedTables, _mask_of, mixed_plan, put_bounded
from .squared_graph import FoldGraph, graph_of
from .squared_sampling import sampler

_HEAD = capi.CK_SQ_DOWN_FOLD_WORDS
_LEAF = capi.CK_SQ_DOWN_LEAF_WORDS


@dataclass
class DownLayer:
    """The launch of one layer of ``c``: its down folds (ascending) and their children ``(n, H, 2)`` as (layer, fold)."""

    layer: int
    folds: list[int]
    children: np.ndarray


@dataclass
class DownPlan:
    qvars: list[int]  # ascending
    mask: np.ndarray  # (D,) bool: M = Q + I
    mixed: MixedPlan  # the values under M; its root is the evidence
    down: set  # (layer, fold) whose scope meets Q
    top: tuple[int, int]  # the output fold
    layers: list[DownLayer]  # output layer first
    leaves: list[tuple[int, int]]  # per query variable, the input fold that reads it
    dev: dict = field(default_factory=dict)  # batch size -> `DownTables`


@dataclass
class DownLaunch:
    """One launch of `ck_squared_down_bwd` at a batch size: the fold rows on the host and on the device, counts, weights."""

    layer: int
    host: np.ndarray
    dev: torch.Tensor
    n: int
    H: int
    Ki: int
    Ko: int
    stages: int
    w1: torch.Tensor | None
    w2: torch.Tensor | None


@dataclass
class DownTables:
    key: tuple
    launches: list[DownLaunch]
    total: int  # values of the down arena
    vars_host: np.ndarray  # the variable rows of the leaf launch
    vars_dev: torch.Tensor


def host_plan(plan: Plan, qvars, mask: np.ndarray, const_available=None, graph: FoldGraph | None = None,
              soft: np.ndarray | None = None) -> DownPlan:
    """The down folds of the query variables `qvars`, the mixed plan of ``M`` = `mask` (which holds them) and the layers to
    launch.  ``NotImplementedError`` where `path_plan` raises it: a variable read by several input folds, a fold above a query
    variable with several readers.  `soft` (cirkit_amd/squared_soft_posterior.py): the query variables carry a weight per state
    instead of being integrated -- `mask` then holds the integrated variables alone and the mixed plan is the soft one, leaves
    included."""
    graph = graph_of(plan, graph)
    qvars = sorted(int(v) for v in qvars)
    leaves = [graph.path(v).leaf for v in qvars]  # (the refusals come before anything is built)
    qbits = sum(1 << v for v in qvars)
    down = {(p, f) for p, row in enumerate(graph.bits) for f, b in enumerate(row) if b & qbits}
    mp = mixed_plan(plan, mask, const_available, readers=down, graph=graph, soft=soft)
    layers = []
    for i in range(len(plan.layers) - 1, -1, -1):  # (children sit below their readers)
        fs = sorted(f for p, f in down if p == i)
        if fs and graph.children[i] is not None:
            layers.append(DownLayer(i, fs, np.stack([graph.children[i][f] for f in fs]).astype(np.int64)))
    return DownPlan(qvars, mask, mp, down, graph.top, layers, leaves)


def down_row_values(sq, dp: DownPlan) -> int:
    """Values per row of the down arena: K^2 for every down fold but the output fold."""
    return sum(sq.graph.units(sq.plan.layers[p]) ** 2 for p, f in dp.down if (p, f) != dp.top)


def row_bytes(sq, dp: DownPlan) -> int:
    """Bytes per row of c's arena, the mixed arena and the down arena."""
    return sq._row_bytes(dp.mixed) + down_row_values(sq, dp) * sq._esize


def plan_of(sq, query_vars, integrate_vars) -> DownPlan:
    """The `DownPlan` of a call, cached on (Q, I)."""
    sampler(sq)  # (Gaussian inputs are refused here)
    D = sq.plan.num_variables
    q = _mask_of(query_vars, D, "query")
    m = _mask_of(integrate_vars, D)
    if not q.any():
        raise ValueError("query_log_marginals needs at least one query variable")
    if (q & m).any():
        raise ValueError("a query variable cannot be integrated out")
    key = np.packbits(q).tobytes() + b"|" + np.packbits(m).tobytes()
    dp = sq._down_plans.get(key)
    if dp is None:
        qvars = np.nonzero(q)[0].tolist()
        for v in qvars:  # (the refusals come before the partition-function circuit is evaluated)
            sq.graph.path(v)
        dp = put_bounded(sq._down_plans, key, host_plan(sq.plan, qvars, q | m, sq._const_available(), sq.graph), 8)
    return dp


def bind(sq, dp: DownPlan, B: int, bd_c, bd_z, tb: MixedTables, positions=None) -> DownTables:
    """The fold tables of every launch and the variable table of the leaf launch at batch size B, on the host and on the
    device, and the layout of the down arena.  `tb`: `sq._tables` of the mixed plan at this batch size.  `positions`: per query
    variable its position on the ``S`` axis of ``log_lik``, word 5 of its row (`ck_squared_soft_down_leaf`); None leaves it 0."""
    layers = sq.plan.layers
    weights = {dl.layer: sq._stage_weights(dl.layer, layers[dl.layer].num_output_units, layers[dl.layer].num_input_units)
               for dl in dp.layers if layers[dl.layer].type != "hadamard"}
    leaf = [sq._leaf_table(pl) for pl, _ in dp.leaves]  # (after c's forward, which builds the tables)
    for v, t in zip(dp.qvars, leaf):
        if t[1] != sq.graph.num_states(v):
            raise RuntimeError(f"HipSquaredCircuit: the table of variable {v} has {t[1]} states, its layer {sq.graph.num_states(v)}")
    key = (bd_c.arena.data_ptr(), bd_z.arena.data_ptr(), tb.arena.data_ptr(), tuple(w.data_ptr() for ws in weights.values() for w in ws),
           tuple(t[0].data_ptr() for t in leaf))
    hit = dp.dev.get(B)
    if hit is not None and hit.key == key:
        return hit
    off, total = {}, 0
    for p, f in sorted(dp.down):
        if (p, f) != dp.top:
            off[(p, f)] = total
            total += (B * sq.graph.units(layers[p]) ** 2 + 3) // 4 * 4
    cls = dp.mixed.classes
    launches = []
    for dl in dp.layers:
        l = layers[dl.layer]
        K, H = l.num_input_units, l.arity
        host = np.zeros((len(dl.folds), _HEAD + 3 * H), dtype=np.int64)
        for j, f in enumerate(dl.folds):
            row = host[j]
            row[0], row[1] = f, off.get((dl.layer, f), -1)
            is_down = [(p, g) in dp.down for p, g in dl.children[j].tolist()]
            for h, (p, g) in enumerate(dl.children[j].tolist()):
                kd, o = sq.child(p, g, K, B, cls[p][g], tb, bd_c, bd_z)
                if sum(is_down) - is_down[h] == 0:
                    kd, o = capi.CK_SQ_CONST, 0  # (no other slot is a down fold: this child's value is never read)
                row[_HEAD + 3 * h: _HEAD + 3 * h + 3] = (off[(p, g)] if is_down[h] else -1, kd, o)
        w1, w2 = weights.get(dl.layer, (None, None))
        launches.append(DownLaunch(dl.layer, host, torch.from_numpy(host).to(sq.device), len(dl.folds), H, K,
                                   l.num_output_units if w1 is not None else K, 2 if w1 is not None else 0, w1, w2))
    vars_host = np.zeros((len(leaf), _LEAF), dtype=np.int64)
    for j, ((table, C, K, tlog), lf) in enumerate(zip(leaf, dp.leaves)):
        vars_host[j, :5] = (table.data_ptr() + lf[1] * (C + 1) * K * 4, C, K, tlog, off.get(lf, -1))
    if positions is not None:
        vars_host[:, 5] = positions
    return put_bounded(dp.dev, B, DownTables(key, launches, max(total, 1), vars_host, torch.from_numpy(vars_host).to(sq.device)), 2)


def _down_arena(sq, n: int) -> torch.Tensor:
    """One down arena per circuit, grown to the largest call so far."""
    a = getattr(sq, "_down_buf", None)
    if a is None or a.numel() < n:
        sq._down_buf = None
        a = sq._down_buf = torch.empty(n, dtype=torch.complex64 if sq._complex else torch.float32, device=sq.device)
    return a


def launch_down(sq, bt: DownTables, arena: torch.Tensor, down: torch.Tensor, bd_c, bd_z, B: int) -> None:
    """The `ck_squared_down_bwd` launches of `bt`, output layer first, over the mixed arena `arena` into the down arena `down`."""
    stream = torch.cuda.current_stream(sq.device).cuda_stream
    with torch.cuda.device(sq.device):
        for la in bt.launches:
            capi.call("ck_squared_down_bwd", arena.data_ptr(), bd_z.arena.data_ptr(), bd_c.arena.data_ptr(), down.data_ptr(), down.numel(),
                      la.host.ctypes.data, la.dev.data_ptr(), la.n, la.H, None if la.w1 is None else la.w1.data_ptr(),
                      None if la.w2 is None else la.w2.data_ptr(), 0 if la.w1 is None else int(la.w1.shape[0]), la.Ki,
                      la.Ko, la.stages, B, sq.rows_per_block, 1 if sq._complex else 0, stream)


def _chunk(sq, dp: DownPlan, xw: torch.Tensor, out: torch.Tensor, ev: torch.Tensor, mark=None) -> None:
    """The cleaned rows `xw` (B, D): ``log m`` into `out` (B, |Q|, C), the unnormalised log evidence into `ev` (B,).  `mark`:
    called with the name of each phase when its launches have been issued (scripts/bench_squared_posterior.py times them)."""
    mark = mark or (lambda name: None)
    B = int(xw.shape[0])
    bd_c = sq.c._run(xw)
    mark("c_forward")
    bd_z = sq._z_binding()
    tb = sq._tables(dp.mixed, B, bd_c, bd_z)
    arena = tb.arena
    sq.last_mixed_launches += sq._launch_mixed(tb.launches, arena, tb.mid, bd_c, bd_z, B)
    mark("mixed")
    rc = dp.mixed.root[0]
    if rc == INTEGRATED:
        ev.copy_(sq._root_of_z().expand(B))
    elif rc == MIXED:
        ev.copy_(sq._mixed_root(tb, dp.mixed, B))
    else:
        raise RuntimeError("HipSquaredCircuit: the output fold holds no query variable")
    bt = bind(sq, dp, B, bd_c, bd_z, tb)
    down = _down_arena(sq, bt.total)
    stream = torch.cuda.current_stream(sq.device).cuda_stream
    cplx = 1 if sq._complex else 0
    launch_down(sq, bt, arena, down, bd_c, bd_z, B)
    mark("down")
    with torch.cuda.device(sq.device):
        capi.call("ck_squared_down_leaf", down.data_ptr(), down.numel(), bt.vars_host.ctypes.data, bt.vars_dev.data_ptr(),
                  len(dp.qvars), int(out.shape[2]), out.data_ptr(), B, cplx, stream)
    mark("leaf")
    sq.last_down_launches += len(bt.launches) + 1


def chunk_rows(sq, dp: DownPlan, rows_per_chunk=None) -> int:
    return sq._chunk_rows(rows_per_chunk, lambda: row_bytes(sq, dp))


def query_log_marginals(sq, x, query_vars, integrate_vars=None, *, normalized=True, return_log_evidence=False, rows_per_chunk=None,
                        mark=None):
    dp = plan_of(sq, query_vars, integrate_vars)
    xw, bad = sq._clean(x, dp.mask)
    B = int(xw.shape[0])
    step = chunk_rows(sq, dp, rows_per_chunk)
    C = max(sq.graph.num_states(v) for v in dp.qvars)
    out = torch.empty((B, len(dp.qvars), C), dtype=torch.float32, device=sq.device)
    ev = torch.empty(B, dtype=torch.float32, device=sq.device)
    sq.last_mixed_launches = 0
    sq.last_down_launches = 0
    for r0 in range(0, B, step):
        _chunk(sq, dp, xw[r0: r0 + step], out[r0: r0 + step], ev[r0: r0 + step], mark)
    if normalized:
        lz = sq._root_of_z()
        out, ev = out - lz, ev - lz
    nan = torch.full((), float("nan"), device=sq.device)
    out = torch.where(bad[:, None, None], nan, out)
    return (out, torch.where(bad, nan, ev)) if return_log_evidence else out


def posterior_marginals(sq, x, query_vars, integrate_vars=None, *, return_log_evidence=False, rows_per_chunk=None):
    lm, ev = query_log_marginals(sq, x, query_vars, integrate_vars, normalized=False, return_log_evidence=True, rows_per_chunk=rows_per_chunk)
    post = lm - torch.logsumexp(lm, dim=2, keepdim=True)
    return (post, ev - sq._root_of_z()) if return_log_evidence else post
