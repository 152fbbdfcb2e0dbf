"""Leave-one-out conditionals of a squared circuit ``p(x) = |c(x)|^2 / Z``: ``p(X_v = s | every other entry of the row)`` for every
variable ``v`` of a set at once (`HipSquaredCircuit.leave_one_out_log_marginals`, `leave_one_out`, `conditional_log_probs`).

With everything but ``v`` observed the derivative of the product circuit is rank-1,

    ``|c(x_{-v}, s)|^2 = |sum_k g_k a_k(s)|^2``,  ``g_k = dc(x) / du_k`` for the ``K`` units ``u_k`` of the input fold of ``v``,

so one derivative pass over ``c`` ITSELF gives ``g`` for every variable of every row: ``c``'s forward, one `ck_squared_loo_down`
launch per layer of ``c`` that has down folds (folds whose scope holds a query variable) from the output layer downwards, and one
`ck_squared_loo_leaf` launch for all the leaves (cirkit_amd/csrc/ck_sqloo.hip).  The pass carries ``log dc/du`` as a signed
logarithm -- not the flow ``g u / c``, which is 0 exactly where the observed state is impossible -- and every child receives its
parent's derivative plus the VALUES of its siblings, read from ``c``'s arena: never the total minus its own value.  The derivative
arena holds ``K`` values per row for every down fold but the output fold; no partition-function circuit, no mixed pass, no
``K^2`` block is touched (`HipSquaredCircuit.posterior_marginals` answers the same question at ``K^2`` cost and, in fp32, about 30
times less accurately: DESIGN.md section 11, "Leave-one-out conditionals of squared circuits").

Refused, before anything is allocated: Gaussian inputs, and ancestries that are not paths (`FoldGraph.path`).  Out of scope:
integrated variables (the derivative is then not rank-1: that is `posterior_marginals`), per-row masks, fusing the pass with
``c``'s forward, gradients with respect to parameters.
"""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

from . import _capi as capi
from .plan import Plan
from .squared import _mask_of, put_bounded
from .squared_graph import FoldGraph, graph_of

_HEAD = capi.CK_SQ_LOO_FOLD_WORDS
_LEAF = capi.CK_SQ_LOO_LEAF_WORDS


@dataclass
class LooLayer:
    """The launch of one layer of ``c``: its down folds (ascending) and their children ``(n, H, 2)`` as (layer, fold)."""

    layer: int
    folds: list[int]
    children: np.ndarray


@dataclass
class LooPlan:
    qvars: list[int]  # ascending
    down: set  # (layer, fold) whose scope holds a query variable
    top: tuple[int, int]  # the output fold
    layers: list[LooLayer]  # output layer first
    leaves: list[tuple[int, int]]  # per query variable, the input fold that reads it
    dev: dict = field(default_factory=dict)  # batch size -> `LooTables`


@dataclass
class LooLaunch:
    """One launch of `ck_squared_loo_down` at a batch size: the fold rows on the host and on the device, counts, weights."""

    layer: int
    host: np.ndarray
    dev: torch.Tensor
    n: int
    H: int
    Ki: int
    Ko: int
    w: torch.Tensor | None


@dataclass
class LooTables:
    key: tuple
    launches: list[LooLaunch]
    total: int  # values of the derivative arena
    vars_host: np.ndarray  # the variable rows of the leaf launch
    vars_dev: torch.Tensor


def host_plan(plan: Plan, qvars, graph: FoldGraph | None = None) -> LooPlan:
    """The down folds of the query variables `qvars` and the layers to launch, output layer first.  ``NotImplementedError`` for
    Gaussian inputs and where `FoldGraph.path` raises it: a variable read by several input folds, a fold above a query variable
    with several readers (a DAG region graph)."""
    if any(l.inputs is None and l.type == "gaussian" for l in plan.layers):
        raise NotImplementedError("HipSquaredCircuit: leave-one-out conditionals of Gaussian input layers (no table of states)")
    graph = graph_of(plan, graph)
    qvars = sorted(int(v) for v in qvars)
    if not qvars:
        raise ValueError("leave-one-out conditionals need at least one query variable")
    leaves = [graph.path(v).leaf for v in qvars]  # (the refusals come before anything is built)
    qbits = sum(1 << v for v in qvars)
    down = {(p, f) for p, row in enumerate(graph.bits) for f, b in enumerate(row) if b & qbits}
    layers = []
    for i in range(len(plan.layers) - 1, -1, -1):  # (children sit below their readers)
        fs = sorted(f for p, f in down if p == i)
        if fs and graph.children[i] is not None:
            layers.append(LooLayer(i, fs, np.stack([graph.children[i][f] for f in fs]).astype(np.int64)))
    return LooPlan(qvars, down, graph.top, layers, leaves)


def der_row_values(sq, lp: LooPlan) -> int:
    """Values per row of the derivative arena: K for every down fold but the output fold."""
    return sum(sq.graph.units(sq.plan.layers[p]) for p, f in lp.down if (p, f) != lp.top)


def row_bytes(sq, lp: LooPlan) -> int:
    """Bytes per row of c's arena and the derivative arena."""
    return (sum(l.num_folds * l.num_output_units for l in sq.plan.layers) + der_row_values(sq, lp)) * sq._esize


def plan_of(sq, query_vars) -> LooPlan:
    """The `LooPlan` of a call, cached on Q (None: every variable)."""
    D = sq.plan.num_variables
    q = np.ones(D, dtype=bool) if query_vars is None else _mask_of(query_vars, D, "query")
    if not q.any():
        raise ValueError("leave-one-out conditionals need at least one query variable")
    key = np.packbits(q).tobytes()
    lp = sq._loo_plans.get(key)
    if lp is None:
        lp = put_bounded(sq._loo_plans, key, host_plan(sq.plan, np.nonzero(q)[0].tolist(), sq.graph), 8)
    return lp


def bind(sq, lp: LooPlan, B: int, bd_c) -> LooTables:
    """The fold tables of every launch and the variable table of the leaf launch at batch size B, on the host and on the
    device, and the layout of the derivative arena."""
    layers = sq.plan.layers
    weights = {ll.layer: sq._stage_weights(ll.layer, layers[ll.layer].num_output_units, layers[ll.layer].num_input_units)[0]
               for ll in lp.layers if layers[ll.layer].type != "hadamard"}
    leaf = [sq._leaf_table(pl) for pl, _ in lp.leaves]  # (after c's forward, which builds the tables)
    for v, t in zip(lp.qvars, leaf):
        if t[1] != sq.graph.num_states(v):
            raise RuntimeError(f"HipSquaredCircuit: the table of variable {v} has {t[1]} states, its layer {sq.graph.num_states(v)}")
    key = (bd_c.arena.data_ptr(), tuple(w.data_ptr() for w in weights.values()), tuple(t[0].data_ptr() for t in leaf))
    hit = lp.dev.get(B)
    if hit is not None and hit.key == key:
        return hit
    off, total = {}, 0
    for p, f in sorted(lp.down):
        if (p, f) != lp.top:
            off[(p, f)] = total
            total += (B * sq.graph.units(layers[p]) + 3) // 4 * 4
    launches = []
    for ll in lp.layers:
        l = layers[ll.layer]
        K, H = l.num_input_units, l.arity
        host = np.zeros((len(ll.folds), _HEAD + 2 * H), dtype=np.int64)
        for j, f in enumerate(ll.folds):
            row = host[j]
            row[0], row[1] = f, off.get((ll.layer, f), -1)
            for h, (p, g) in enumerate(ll.children[j].tolist()):
                if sq.graph.units(layers[p]) != K:
                    raise ValueError("a layer's children do not all have its number of input units")
                row[_HEAD + 2 * h: _HEAD + 2 * h + 2] = (off[(p, g)] if (p, g) in lp.down else -1, bd_c.views[p].storage_offset() + g * B * K)
        w = weights.get(ll.layer)
        launches.append(LooLaunch(ll.layer, host, torch.from_numpy(host).to(sq.device), len(ll.folds), H, K,
                                  l.num_output_units if w is not None else K, w))
    vars_host = np.zeros((len(leaf), _LEAF), dtype=np.int64)
    for j, ((table, C, K, tlog), lf, v) in enumerate(zip(leaf, lp.leaves, lp.qvars)):
        vars_host[j] = (table.data_ptr() + lf[1] * (C + 1) * K * 4, C, K, tlog, off.get(lf, -1), v)
    return put_bounded(lp.dev, B, LooTables(key, launches, max(total, 1), vars_host, torch.from_numpy(vars_host).to(sq.device)), 2)


def _der_arena(sq, n: int) -> torch.Tensor:
    """One derivative arena per circuit, grown to the largest call so far."""
    a = sq._loo_buf
    if a is None or a.numel() < n:
        sq._loo_buf = None
        a = sq._loo_buf = torch.empty(n, dtype=torch.complex64 if sq._complex else torch.float32, device=sq.device)
    return a


def _chunk(sq, lp: LooPlan, xw: torch.Tensor, out: torch.Tensor, mode: int, mark=None, form: int = 0) -> None:
    """The cleaned rows `xw` (B, D) into `out`: (B, |Q|, C) in the table modes, (B, |Q|) per entry.  `mark`: called with the name
    of each phase when its launches have been issued; `form` 1 forces the VALU form of the down launches
    (scripts/bench_squared_loo.py)."""
    mark = mark or (lambda name: None)
    B = int(xw.shape[0])
    bd_c = sq.c._run(xw)
    mark("c_forward")
    sq._z_binding()  # (the weight blocks `_stage_weights` hands out are evaluated with the partition-function circuit, once)
    bt = bind(sq, lp, B, bd_c)
    der = _der_arena(sq, bt.total)
    stream = torch.cuda.current_stream(sq.device).cuda_stream
    cplx = 1 if sq._complex else 0
    with torch.cuda.device(sq.device):
        for la in bt.launches:
            capi.call("ck_squared_loo_down", bd_c.arena.data_ptr(), bd_c.arena.numel(), der.data_ptr(), der.numel(), la.host.ctypes.data,
                      la.dev.data_ptr(), la.n, la.H, None if la.w is None else la.w.data_ptr(), 0 if la.w is None else int(la.w.shape[0]),
                      la.Ki, la.Ko, B, cplx, form, stream)
        mark("down")
        capi.call("ck_squared_loo_leaf", der.data_ptr(), der.numel(), bt.vars_host.ctypes.data, bt.vars_dev.data_ptr(), len(lp.qvars),
                  int(out.shape[2]) if out.dim() == 3 else int(bt.vars_host[:, 1].max()), xw.data_ptr(), int(xw.shape[1]), out.data_ptr(), mode, B, cplx, stream)
    mark("leaf")
    sq.last_loo_launches += len(bt.launches) + 1


def _run(sq, x, query_vars, mode: int, rows_per_chunk=None, mark=None, form: int = 0) -> tuple[torch.Tensor, torch.Tensor, LooPlan]:
    lp = plan_of(sq, query_vars)
    xw, bad = sq._clean(x, np.zeros(sq.plan.num_variables, dtype=bool))
    B = int(xw.shape[0])
    step = sq._chunk_rows(rows_per_chunk, lambda: row_bytes(sq, lp))
    shape = (B, len(lp.qvars)) if mode == capi.CK_SQ_LOO_ENTRY else (B, len(lp.qvars), max(sq.graph.num_states(v) for v in lp.qvars))
    out = torch.empty(shape, dtype=torch.float32, device=sq.device)
    sq.last_loo_launches = 0
    for r0 in range(0, B, step):
        _chunk(sq, lp, xw[r0: r0 + step], out[r0: r0 + step], mode, mark, form)
    return out, bad, lp


def _nan_rows(sq, out: torch.Tensor, bad: torch.Tensor) -> torch.Tensor:
    return torch.where(bad.view(-1, *([1] * (out.dim() - 1))), torch.full((), float("nan"), device=sq.device), out)


def leave_one_out_log_marginals(sq, x, query_vars=None, *, normalized=True, rows_per_chunk=None, mark=None, form=0) -> torch.Tensor:
    out, bad, _ = _run(sq, x, query_vars, capi.CK_SQ_LOO_TABLE, rows_per_chunk, mark, form)
    if normalized:
        out = out - sq._root_of_z()
    return _nan_rows(sq, out, bad)


def leave_one_out(sq, x, query_vars=None, *, rows_per_chunk=None, mark=None, form=0) -> torch.Tensor:
    out, bad, _ = _run(sq, x, query_vars, capi.CK_SQ_LOO_NORMALISED, rows_per_chunk, mark, form)
    return _nan_rows(sq, out, bad)


def conditional_log_probs(sq, x, *, rows_per_chunk=None, mark=None, form=0) -> torch.Tensor:
    out, bad, _ = _run(sq, x, None, capi.CK_SQ_LOO_ENTRY, rows_per_chunk, mark, form)
    return _nan_rows(sq, out, bad)
