"""Soft and interval evidence of a squared circuit ``p(x) = |c(x)|^2 / Z`` on the GPU: `HipSquaredCircuit.soft_evidence_log_prob`,
`interval_log_prob` and `log_cdf` ("Soft and interval evidence of squared circuits").

Every soft variable of a row carries a non-negative weight per state, ``log_lik[n, s, c] = log lambda``; the query is

    ``Z(lambda)[n] = sum_{x_S, x_M} |c(x_O, x_S, x_M)|^2 prod_{v in S} lambda[n, v, x_v]``,

with ``M`` integrated out and the other variables ``O`` observed.  It is the product circuit ``c (x) conj(c)`` with one change at
the leaves: the input fold of a soft variable emits the weighted Gram matrix ``G_n[k, l] = sum_s lambda_n(s) e_k(s) conj(e_l(s))``,
``K^2`` values per row (`ck_squared_soft_leaf`, cirkit_amd/csrc/ck_sqsoft.hip: one launch per input layer with a soft fold), which
the mixed pass of `log_marginal` reads as a FULL child (`squared.mixed_plan` with ``soft=``): every fold whose scope meets ``S`` is
evaluated, nothing else changes.  A box ``lo <= x_v <= hi`` is the 0/1 case of the same leaf launch, read from the bounds
themselves: no ``(B, S, C)`` tensor is built.  The reference has no such query, as for `HipCircuit`'s soft and interval evidence.

Posteriors and sampling under soft evidence: cirkit_amd/squared_soft_posterior.py.  Out of scope: MPE under soft evidence; fusing
the leaf Gram into the first product layer, so that the ``|S| K^2`` block of a row is never written; exploiting the Gram's
symmetry; Gaussian boxes (Gaussian variables stay hard evidence or integrated); per-row soft sets; gradients.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _capi as capi
from .squared import MixedPlan, MixedTables, _mask_of, mixed_plan, put_bounded
from .squared_graph import FoldGraph


@dataclass
class SoftLaunch:
    """One launch of `ck_squared_soft_leaf`: the soft folds of one input layer -- (fold, position on the ``S`` axis) and (fold,
    variable) pairs on the host and on the device -- and where its output starts in the mixed arena."""

    layer: int
    n: int
    K: int
    base: int
    by_pos: np.ndarray  # (n, 2) int32
    by_var: np.ndarray
    by_pos_dev: torch.Tensor
    by_var_dev: torch.Tensor


def states_of(graph: FoldGraph, var: int) -> int:
    """The number of states of a variable: that of the (first) discrete input layer that reads it, 0 for a Gaussian one."""
    cfg = graph.plan.layers[graph.leaves[int(var)][0][0]].config
    return int(cfg.get("num_states", cfg.get("num_categories", 0)))


def check_sets(graph: FoldGraph, soft: np.ndarray, integrate: np.ndarray, what: str) -> None:
    """The refusals of a call, before anything is allocated: an empty soft set and one that meets the integrated set
    (``ValueError``), a soft variable outside every input layer's scope (``ValueError``), a Gaussian layer under one
    (``NotImplementedError``)."""
    if not soft.any():
        raise ValueError(f"{what} needs at least one soft variable")
    if (soft & integrate).any():
        raise ValueError(f"a variable cannot be both {'soft' if what == 'soft evidence' else 'in the box'} and integrated out: "
                         f"{np.nonzero(soft & integrate)[0][:8].tolist()}")
    ids = np.nonzero(soft)[0].tolist()
    missing = [v for v in ids if v not in graph.leaves]
    if missing:
        raise ValueError(f"soft variables {missing[:8]} are outside the scope of every input layer")
    gauss = [v for v in ids if any(graph.plan.layers[p].type == "gaussian" for p, _ in graph.leaves[v])]
    if gauss:
        raise NotImplementedError(f"{what} on variables {gauss[:8]} read by a Gaussian layer: pass them as hard evidence "
                                  "through x, or integrate them out")


def soft_plan(sq, integrate: np.ndarray, soft: np.ndarray) -> MixedPlan:
    """The `MixedPlan` of a call (its leaves included), cached on (M, S)."""
    key = (np.packbits(integrate).tobytes(), np.packbits(soft).tobytes())
    mp = sq._soft_plans.get(key)
    if mp is None:
        mp = put_bounded(sq._soft_plans, key, mixed_plan(sq.plan, integrate, sq._const_available(), graph=sq.graph, soft=soft), 8)
    return mp


def bind_leaves(sq, mp: MixedPlan, tb: MixedTables, B: int) -> None:
    """The blocks of the evaluated input folds in the mixed arena of `tb` (behind those laid out so far) and their launches."""
    for lf in mp.leaves:
        K = sq.graph.units(sq.plan.layers[lf.layer])
        tb.where.update(((lf.layer, int(f)), tb.total + j * B * K * K) for j, f in enumerate(lf.folds))
        by_pos = np.ascontiguousarray(np.stack([lf.folds, lf.pos], axis=1).astype(np.int32))
        by_var = np.ascontiguousarray(np.stack([lf.folds, lf.var], axis=1).astype(np.int32))
        tb.leaves.append(SoftLaunch(lf.layer, len(lf.folds), K, tb.total, by_pos, by_var, torch.from_numpy(by_pos).to(sq.device),
                                    torch.from_numpy(by_var).to(sq.device)))
        tb.total += (len(lf.folds) * B * K * K + 3) // 4 * 4


def unit_maxima(sq) -> dict:
    """Per input layer of ``c`` with a table of logarithms, the ``(F, K)`` clamped maxima of every unit's column over the states:
    the per-unit shifts of the leaf launch.  Rebuilt when a parameter changed; after c's forward, which builds the tables."""
    state = (sq.c.store.version, sq.c.store.state())
    if sq._soft_side is None or sq._soft_side[0] != state:
        side = {}
        big = torch.finfo(torch.float32).max
        for i, l in enumerate(sq.plan.layers):
            if l.inputs is None and l.type == "categorical":
                table, C, _, _ = sq._leaf_table(i)
                side[i] = table[:, :C, :].amax(dim=1).clamp(min=-big, max=big).contiguous()
        sq._soft_side = (state, side)
    return sq._soft_side[1]


def launch_leaves(sq, tb: MixedTables, B: int, log_lik, lo, hi, form: int = 0, arena: torch.Tensor | None = None) -> int:
    """The leaf launches of `tb` into its arena (or `arena`, where the caller brings one) -- soft evidence from `log_lik`
    (B, S, C) fp32, or a box from `lo` / `hi` (B, D) int64; how many there were.  `form` 1 forces the plain form
    (scripts/bench_squared_soft.py)."""
    arena = tb.arena if arena is None else arena
    side = unit_maxima(sq)
    stream = torch.cuda.current_stream(sq.device).cuda_stream
    with torch.cuda.device(sq.device):
        for la in tb.leaves:
            table, C, K, tlog = sq._leaf_table(la.layer)
            if K != la.K:
                raise RuntimeError(f"HipSquaredCircuit: the table of input layer {la.layer} has {K} units, its layer {la.K}")
            if log_lik is not None and int(log_lik.shape[2]) < C:
                raise ValueError(f"log_lik has {int(log_lik.shape[2])} states, the soft variables have up to {C}")
            mt = side.get(la.layer)
            soft = log_lik is not None
            capi.call("ck_squared_soft_leaf", table.data_ptr(), int(table.shape[0]), C, K, tlog, None if mt is None else mt.data_ptr(),
                      (la.by_pos if soft else la.by_var).ctypes.data, (la.by_pos_dev if soft else la.by_var_dev).data_ptr(), la.n,
                      log_lik.data_ptr() if soft else None, int(log_lik.shape[1]) if soft else 0, int(log_lik.shape[2]) if soft else 0,
                      None if soft else lo.data_ptr(), None if soft else hi.data_ptr(), 0 if soft else int(lo.shape[1]),
                      arena.data_ptr() + la.base * sq._esize, B, sq.rows_per_block, 1 if sq._complex else 0, form, stream)
    return len(tb.leaves)


def _chunk(sq, mp: MixedPlan, xw: torch.Tensor, log_lik, lo, hi, form: int = 0) -> torch.Tensor:
    """Unnormalised log evidence of the (cleaned) rows: c's forward, the leaf launches, the mixed launches."""
    B = int(xw.shape[0])
    bd_c = sq.c._run(xw)
    bd_z = sq._z_binding()
    tb = sq._tables(mp, B, bd_c, bd_z)
    sq.last_soft_launches += launch_leaves(sq, tb, B, log_lik, lo, hi, form)
    sq.last_launches += sq._launch_mixed(tb.launches, tb.arena, tb.mid, bd_c, bd_z, B)
    return sq._mixed_root(tb, mp, B).clone()


def _sets(sq, soft_vars, integrate_vars, what: str) -> tuple[np.ndarray, np.ndarray]:
    D = sq.plan.num_variables
    integrate = _mask_of(integrate_vars, D)
    soft = ~integrate if soft_vars is None else _mask_of(soft_vars, D, "weigh" if what == "soft evidence" else "bound")
    check_sets(sq.graph, soft, integrate, what)
    return soft, integrate


def _rows(sq, x, B: int, soft: np.ndarray, integrate: np.ndarray) -> tuple[torch.Tensor, torch.Tensor]:
    """The cleaned hard evidence and its absent rows; `x` may be None where no variable is left to observe."""
    D = sq.plan.num_variables
    if x is None:
        if not (soft | integrate).all():
            raise ValueError(f"x is required: variables {np.nonzero(~(soft | integrate))[0][:8].tolist()} are neither soft nor integrated")
        x = torch.zeros((B, D), dtype=torch.float32 if sq.c._float_input else torch.int64, device=sq.device)
    elif x.dim() != 2 or x.shape[1] != D:
        raise ValueError(f"expected x of shape (B, {D}), found {tuple(x.shape)}")
    elif int(x.shape[0]) != B:
        raise ValueError(f"the evidence has {B} rows and x {int(x.shape[0])}")
    return sq._clean(x, soft | integrate)


def _evaluate(sq, mp: MixedPlan, xw, bad, B: int, pieces, normalized: bool, rows_per_chunk, form: int = 0) -> torch.Tensor:
    step = sq._chunk_rows(rows_per_chunk, lambda: sq._row_bytes(mp))
    sq.last_launches = sq.last_soft_launches = 0
    out = torch.empty(B, dtype=torch.float32, device=sq.device)
    for r0 in range(0, B, step):
        ll, lo, hi, nan_rows = pieces(r0, r0 + step)
        out[r0: r0 + step] = _chunk(sq, mp, xw[r0: r0 + step], ll, lo, hi, form)
        if nan_rows is not None:
            bad[r0: r0 + step] |= nan_rows
    if normalized:
        out = out - sq._root_of_z()
    return torch.where(bad, torch.full((), float("nan"), device=sq.device), out)


def soft_weights(sq, log_lik, soft: np.ndarray):
    """What every query under soft evidence checks of ``log_lik`` (rank, dtype, the ``S`` axis, enough states) before anything is
    allocated: the batch size and `pieces(r0, r1)`, which gives the rows r0 .. r1 on the device as contiguous fp32 and the rows
    among them with a NaN or ``+inf`` in a read entry (those rows alone are NaN)."""
    from .soft_evidence import check_arguments

    ids = np.nonzero(soft)[0].tolist()
    check_arguments(sq.plan, log_lik, None, ids)  # (rank, dtype, S; x is checked against this circuit's own rules)
    B, _, Cl = (int(n) for n in log_lik.shape)
    counts = np.asarray([states_of(sq.graph, v) for v in ids])
    if Cl < counts.max():
        raise ValueError(f"log_lik has {Cl} states, the soft variables have up to {int(counts.max())}")
    read = None  # the entries a row reads, where the soft variables do not all have C states
    if (counts != Cl).any():
        read = torch.from_numpy(np.arange(Cl)[None, :] < counts[:, None]).to(sq.device)

    def pieces(r0, r1):
        ll = log_lik[r0:r1].to(sq.device).to(torch.float32).contiguous()
        wrong = torch.isnan(ll) | (ll == float("inf"))
        if read is not None:
            wrong &= read
        return ll, wrong.flatten(1).any(dim=1)

    return B, int(counts.max()), pieces


def soft_evidence_log_prob(sq, log_lik, x=None, *, soft_vars=None, integrate_vars=None, normalized=True, rows_per_chunk=None,
                           form: int = 0) -> torch.Tensor:
    soft, integrate = _sets(sq, soft_vars, integrate_vars, "soft evidence")
    B, _, weights = soft_weights(sq, log_lik, soft)
    xw, bad = _rows(sq, x, B, soft, integrate)
    mp = soft_plan(sq, integrate, soft)

    def pieces(r0, r1):
        ll, wrong = weights(r0, r1)
        return ll, None, None, wrong

    return _evaluate(sq, mp, xw, bad, B, pieces, normalized, rows_per_chunk, form)


def interval_log_prob(sq, lo, hi, x=None, *, box_vars=None, integrate_vars=None, normalized=True, rows_per_chunk=None,
                      form: int = 0) -> torch.Tensor:
    D = sq.plan.num_variables
    box, integrate = _sets(sq, box_vars, integrate_vars, "interval evidence")
    for name, t in (("lo", lo), ("hi", hi)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != D or t.is_floating_point() or t.dtype == torch.bool:
            raise ValueError(f"{name} should be an integer tensor of shape (B, {D}): rows, variables")
    if lo.shape != hi.shape:
        raise ValueError(f"lo has {int(lo.shape[0])} rows and hi {int(hi.shape[0])}")
    B = int(lo.shape[0])
    if B <= 0:
        raise ValueError("empty batch")
    xw, bad = _rows(sq, x, B, box, integrate)
    mp = soft_plan(sq, integrate, box)
    lo, hi = (t.to(sq.device).to(torch.int64) for t in (lo, hi))

    def pieces(r0, r1):
        return None, lo[r0:r1].contiguous(), hi[r0:r1].contiguous(), None

    return _evaluate(sq, mp, xw, bad, B, pieces, normalized, rows_per_chunk, form)


def log_cdf(sq, x, *, integrate_vars=None, rows_per_chunk=None) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.is_floating_point():
        raise ValueError(f"x should be an integer tensor of shape (B, {sq.plan.num_variables})")
    return interval_log_prob(sq, torch.zeros_like(x), x, None, integrate_vars=integrate_vars, rows_per_chunk=rows_per_chunk)
