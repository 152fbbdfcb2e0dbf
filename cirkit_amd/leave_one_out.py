"""Leave-one-out conditionals on the GPU: `HipCircuit.leave_one_out` and `HipCircuit.conditional_log_probs` (DESIGN.md
section 11, "Leave-one-out conditionals").

``p(X_v = c | x_{O \\ {v}})`` for every variable ``v`` of every row at once: how well each observed value fits the rest of its
row (pseudo-log-likelihood, per-cell outlier scores, the full conditionals of a Gibbs sweep, cell repair).  One evidence forward
and one top-down pass give all of them -- Darwiche's differential reading of a circuit: the derivative of the output with
respect to an input unit over ``v`` is the circuit with ``v`` taken out, so ``p(X_v = c, x_{O \\ v}) = sum_k (dc/du_k) t_k[c]``
over the input units ``u_k`` of ``v``, ``t_k`` their table rows.

Downward the pass carries ``D(u) = log (dc(x_O) / du)`` in LOG space, 0 at the root unit and -inf where the derivative is 0.
The flow of `posterior_marginals`, ``f = (dc/du) u / c``, cannot be reused: it is exactly 0 wherever ``u = 0`` -- an input unit
that calls the OBSERVED state impossible, which is the very term a wrong cell needs -- and 0 / 0 for a row without mass.  The
derivative recurrence never divides by a value and never multiplies by the child's own value.

The reference has no such query.  This module reuses the circuit's `Sampler` and `PosteriorState` (structure, `prepare()`d
weights, the evidence forward with its range check, the normalised input tables) unchanged and runs the shared top-down pass
(cirkit_amd/topdown.py) in its derivative form; the log normalisers of the input units are built here once per parameter
state.  Kernels: cirkit_amd/csrc/ck_loo.hip.
"""

from __future__ import annotations

from typing import TYPE_CHECKING

import numpy as np
import torch

from . import _capi as capi
from .posterior import PosteriorState, _state, query_ids
from .sampling import check_plan
from . import topdown
from .plan import Plan
from .topdown import (DERIVATIVE, QuerySets, TopDownPass, check_query, discrete_tables, leaf_entries, run_chunks,
                      variable_kinds)  # noqa: F401

if TYPE_CHECKING:  # pragma: no cover
    from .circuit import HipCircuit


def message_lists(plan: Plan) -> list[dict | None]:
    """The consumer lists of the derivative pass: `topdown.consumer_lists` with a message per (fold, input position)."""
    return topdown.consumer_lists(plan, True)


def check_query_vars(kinds: dict[int, set[str]], ids: list[int]) -> bool:
    """`topdown.check_query` for `leave_one_out`, given `variable_kinds`.  Needs no device."""
    return check_query(kinds, ids, "leave_one_out")


class LeaveOneOutState:
    """The leave-one-out state of one `HipCircuit`, next to its `PosteriorState`."""

    def __init__(self, ps: PosteriorState) -> None:
        self.ps = ps
        s = ps.s
        self.lz_off: dict[int, int] = {}  # input layer -> element offset of its (F, K) log normalisers
        n = 0
        for j, d in enumerate(s.layers):
            if "scope" in d:
                self.lz_off[j], n = n, n + d["F"] * d["Ko"]
        self.covered = sorted(ps.var_folds)
        kind = np.zeros(s.D, dtype=np.int32)
        for v in self.covered:
            kind[v] = 2 if "gaussian" in ps.kinds[v] else 1
        self._vkind = kind
        self.down = TopDownPass(s, DERIVATIVE)
        self._queries = QuerySets(self._entries)
        self._all: dict | None = None
        self._key = None
        self._lz: torch.Tensor | None = None

    # -- refusals: nothing is prepared or launched before them -----------------------------------------------------------
    def check_query(self, ids: list[int]) -> bool:
        """Whether the query variables are Gaussian; raises for an empty, uncovered or mixed query set."""
        return check_query_vars(self.ps.kinds, ids)

    # -- once per query set ------------------------------------------------------------------------------------------
    def _entries(self, ids: list[int], gauss: bool | None) -> dict:
        """The leaf entries of the variables `ids` (gauss None: log probabilities, the table offset is not read)."""
        q, e, start = leaf_entries(self.ps.s, self.ps.var_folds, self.ps.tab_off, ids, gauss, self.lz_off)
        # the widest variable's input units: the categorical leaf kernel stages one weight per unit in LDS
        q["max_units"] = max([int(e[a:b, 1].sum()) for a, b in zip(start[:-1], start[1:])], default=0)
        return q

    def query_tables(self, ids: list[int], gauss: bool) -> dict:
        return self._queries.get(ids, gauss)

    def all_tables(self) -> dict:
        if self._all is None:
            q = self._entries(list(range(self.ps.s.D)), None)
            q["vkind"] = torch.from_numpy(self._vkind).to(self.ps.s.device)
            self._all = q
        return self._all

    # -- once per parameter state ------------------------------------------------------------------------------------
    def tables(self) -> None:
        """`PosteriorState.tables()` and, from the same `prepare()` tables, ``log Z_k = log sum_c t_k[c]`` of every input
        unit (0 for a Gaussian unit, -inf for a unit whose table row has no mass)."""
        ps, s = self.ps, self.ps.s
        ps.tables()
        if self._key == s._key:
            return
        dev = s.device
        with torch.cuda.device(dev):
            zero = torch.zeros((), device=dev)
            ninf = torch.full((), float("-inf"), device=dev)
            lz = {j: torch.where(tot > 0, torch.log(torch.where(tot > 0, tot, zero + 1)) + shift, ninf)
                  for j, _, shift, tot in discrete_tables(s)}
            self._lz = torch.cat([lz[j].to(torch.float32).contiguous().reshape(-1) if j in lz else
                                  torch.zeros(d["F"] * d["Ko"], dtype=torch.float32, device=dev)
                                  for j, d in enumerate(s.layers) if "scope" in d])
        self._key = s._key

    # -- per chunk: the phases (scripts/bench_leave_one_out.py times them one by one) ---------------------------------------
    def derivative_pass(self, bd, stream: int) -> torch.Tensor:
        """The log derivatives of every unit under the values of binding `bd`, layers last to first; returns the arena."""
        return self.down.run(bd, stream)

    def leaves(self, bd, der: torch.Tensor, q: dict, gauss: bool, bad: torch.Tensor, out: torch.Tensor, stream: int) -> None:
        """The conditionals of the chunk's rows into `out` (its first row)."""
        ps, s = self.ps, self.ps.s
        head = (q["entries"].data_ptr(), q["start"].data_ptr(), q["Q"])
        tail = (der.data_ptr(), s._val_off_table(bd).data_ptr(), bad.data_ptr(), bd.B, out.data_ptr(), stream)
        if gauss:
            capi.call("ck_loo_leaf_gaussian", *head, ps._mean.data_ptr(), ps._stddev.data_ptr(), *tail)
        else:
            capi.call("ck_loo_leaf_categorical", *head, q["C"], q["max_units"], ps._ntab.data_ptr(), self._lz.data_ptr(), *tail)

    def log_probs(self, bd, der: torch.Tensor, xc: torch.Tensor, bad: torch.Tensor, out: torch.Tensor, stream: int) -> None:
        """log p(x_v | x_{O \\ v}) of the chunk's rows (masked evidence `xc`) into `out` (its first row)."""
        s, q = self.ps.s, self.all_tables()
        capi.call("ck_loo_log_probs", q["entries"].data_ptr(), q["start"].data_ptr(), q["vkind"].data_ptr(), s.D,
                  self._lz.data_ptr(), der.data_ptr(), bd.arena.data_ptr(), s._val_off_table(bd).data_ptr(), xc.data_ptr(),
                  1 if s.float_out else 0, bad.data_ptr(), bd.B, out.data_ptr(), stream)

    # -- once per call ------------------------------------------------------------------------------------------------
    def leave_one_out(self, x: torch.Tensor, query_vars, missing_vars, rows_per_chunk: int | None) -> torch.Tensor:
        s = self.ps.s
        ids = self.covered if query_vars is None else query_ids(query_vars, s.D)
        gauss = self.check_query(ids)  # (refusals first: nothing has been copied, prepared or launched)

        def start(B: int):
            q = self.query_tables(ids, gauss)
            out = torch.empty((B, q["Q"], q["C"]), dtype=torch.float32, device=s.device)

            def tail(r0, xc, bd, der, bad, stream):
                self.leaves(bd, der, q, gauss, bad, out[r0], stream)

            return out, tail

        return run_chunks(self.ps, self.down, x, [] if missing_vars is None else missing_vars, rows_per_chunk, self.tables, start)

    def conditional_log_probs(self, x: torch.Tensor, missing_vars, rows_per_chunk: int | None) -> torch.Tensor:
        s = self.ps.s

        def start(B: int):
            out = torch.empty((B, s.D), dtype=torch.float32, device=s.device)

            def tail(r0, xc, bd, der, bad, stream):
                self.log_probs(bd, der, xc, bad, out[r0], stream)

            return out, tail

        return run_chunks(self.ps, self.down, x, [] if missing_vars is None else missing_vars, rows_per_chunk, self.tables, start)


def _loo(hc: "HipCircuit") -> LeaveOneOutState:
    ps = _state(hc)
    st = getattr(ps, "_leave_one_out", None)
    if st is None:
        st = ps._leave_one_out = LeaveOneOutState(ps)
    return st


def leave_one_out(hc: "HipCircuit", x: torch.Tensor, query_vars=None, missing_vars=None, *, rows_per_chunk: int | None = None):
    """`HipCircuit.leave_one_out`: see its docstring."""
    return _loo(hc).leave_one_out(x, query_vars, missing_vars, rows_per_chunk)


def conditional_log_probs(hc: "HipCircuit", x: torch.Tensor, missing_vars=None, *, rows_per_chunk: int | None = None):
    """`HipCircuit.conditional_log_probs`: see its docstring."""
    return _loo(hc).conditional_log_probs(x, missing_vars, rows_per_chunk)


class LeaveOneOutQuery:
    """Reference-shaped wrapper, next to `PosteriorMarginalQuery`: ``LeaveOneOutQuery(circuit)(x, query_vars=...)`` returns
    the ``(B, Q, C)`` conditionals of `HipCircuit.leave_one_out`."""

    def __init__(self, circuit: "HipCircuit") -> None:
        check_plan(circuit.user_plan)
        self._circuit = circuit

    def __call__(self, x: torch.Tensor, *, query_vars, missing_vars=None):
        return leave_one_out(self._circuit, x, query_vars, missing_vars)
