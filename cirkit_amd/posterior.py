"""Posterior marginals on the GPU: `HipCircuit.posterior_marginals` ("Posterior marginals").

All single-variable posteriors ``p(X_v = c | x_O)`` of every row of a batch, exactly, in one evidence forward and one
top-down pass.  Upward: the layer-wise marginal forward the conditional sampler runs, ``v`` the per-row log value of every
unit.  Downward: the FLOW ``f(u) = d log c(x_O) / d log u`` of every unit, in linear space, 1 at the root; an entry ``i`` of a
sum-type unit ``k`` receives ``f_k w[k, i] exp(e_i - v_k)`` (``e_i`` the entry's child value), a product unit hands its
flow to its inputs, and the posterior of ``v`` is the flow that reaches the input units over ``v`` spread over their own
normalised distributions.  Flows lie in [0, 1] and sum to 1 over the input units of one variable; that is checked by the
tests, the output is not renormalised.

The reference has no such query.  This module reuses the circuit's `Sampler` (structure, `prepare()`d weights and input
tables, the private layer-wise circuit and its ``val_off`` addressing); the consumer lists are built here once per circuit,
the normalised input tables once per parameter state.  Kernels: cirkit_amd/csrc/ck_flow.hip.
"""

from __future__ import annotations

from typing import TYPE_CHECKING

import numpy as np
import torch

from . import _capi as capi
from . import topdown
from .plan import Plan
from .sampling import Sampler, check_plan, sampler
from .topdown import (FLOW, QuerySets, TopDownPass, check_query, discrete_tables, leaf_entries, num_consumers,  # noqa: F401
                      run_chunks, variable_kinds)

if TYPE_CHECKING:  # pragma: no cover
    from .circuit import HipCircuit


def consumer_lists(plan: Plan) -> list[dict | None]:
    """The consumer lists of the flow pass: `topdown.consumer_lists` with one CP-T message per fold."""
    return topdown.consumer_lists(plan, False)


def query_ids(query_vars, D: int) -> list[int]:
    """The query variables in ascending order, from an iterable of ids or a (D,) / (1, D) bool mask."""
    if isinstance(query_vars, torch.Tensor):
        if query_vars.dim() == 2 and query_vars.shape[0] > 1:
            raise ValueError("posterior_marginals takes one query set for the whole batch: a (D,) or (1, D) mask "
                             f"(a {tuple(query_vars.shape)} mask would make the output ragged)")
        if query_vars.dtype != torch.bool:
            raise ValueError(f"Expected dtype of tensor to be torch.bool, got {query_vars.dtype}")
        if query_vars.dim() not in (1, 2) or query_vars.shape[-1] != D:
            raise ValueError(f"Circuit scope has {D} variables but query_vars was defined over "
                             f"{query_vars.shape[-1] if query_vars.dim() else 0} != {D} variables")
        return [int(v) for v in np.nonzero(query_vars.reshape(-1).cpu().numpy())[0]]
    ids = sorted({int(v) for v in query_vars})
    if ids and (ids[0] < 0 or ids[-1] >= D):
        raise ValueError("The variables to marginalize must be a subset of the circuit scope")
    return ids


class PosteriorState:
    """The posterior-marginal state of one `HipCircuit`, next to its `Sampler`."""

    def __init__(self, s: Sampler) -> None:
        self.s = s
        self.var_folds: dict[int, list[tuple[int, int]]] = {}  # variable -> [(input layer, fold)]
        self.tab_off: dict[int, int] = {}  # input layer -> element offset of its block in the per-state flat tables
        n_cat = n_gauss = 0
        for j, d in enumerate(s.layers):
            if "scope" not in d:
                continue
            for f, v in enumerate(np.asarray(d["spec"].scope_idx[:, 0], dtype=np.int64)):
                self.var_folds.setdefault(int(v), []).append((j, f))
            if d["kind"] == capi.CK_SAMPLE_GAUSSIAN:
                self.tab_off[j], n_gauss = n_gauss, n_gauss + d["F"] * d["Ko"]
            else:
                self.tab_off[j], n_cat = n_cat, n_cat + d["F"] * d["Ko"] * d["M"]
        self.kinds = variable_kinds(s.plan)
        self.down = TopDownPass(s, FLOW)
        self._queries = QuerySets(self._entries)
        self._key = None
        self._ntab: torch.Tensor | None = None
        self._mean: torch.Tensor | None = None
        self._stddev: torch.Tensor | None = None

    # -- refusals: nothing is prepared or launched before them -----------------------------------------------------------
    def check_query(self, ids: list[int]) -> bool:
        """Whether the query variables are Gaussian; raises for an empty, uncovered or mixed query set."""
        return check_query(self.kinds, ids, "posterior_marginals")

    # -- once per query set ------------------------------------------------------------------------------------------
    def _entries(self, ids: list[int], gauss: bool) -> dict:
        q, e, _ = leaf_entries(self.s, self.var_folds, self.tab_off, ids, gauss)
        ks = set(e[:, 1].tolist())  # (the matrix-core leaf kernel wants every entry with the same 32 or 64 units)
        q["K_uniform"] = ks.pop() if len(ks) == 1 and next(iter(ks)) in (32, 64) else 0
        return q

    def query_tables(self, ids: list[int], gauss: bool) -> dict:
        return self._queries.get(ids, gauss)

    # -- once per parameter state ------------------------------------------------------------------------------------
    def tables(self) -> None:
        """The normalised table rows of the Categorical / Binomial layers ((F, K, C) blocks of one flat buffer) and the
        Gaussian layers' means and standard deviations, for the store's current values."""
        s = self.s
        s.prepare()
        if self._key == s._key:
            return
        dev = s.device
        with torch.cuda.device(dev):
            zero = torch.zeros((), device=dev)
            cats = [torch.where(tot > 0, t / tot, zero).contiguous().reshape(-1) for _, t, _, tot in discrete_tables(s)]
            gauss = [d for d in s.layers if "scope" in d and d["kind"] == capi.CK_SAMPLE_GAUSSIAN]
            self._ntab = torch.cat(cats) if cats else None
            self._mean = torch.cat([d["mean_v"].reshape(-1) for d in gauss]) if gauss else None
            self._stddev = torch.cat([d["stddev_v"].reshape(-1) for d in gauss]) if gauss else None
        self._key = s._key

    # -- per chunk: the three phases (scripts/bench_posterior.py times them one by one) ------------------------------------
    def evidence_forward(self, xc: torch.Tensor, bad: torch.Tensor, stream: int):
        """The layer-wise marginal forward of a chunk of masked evidence, after its range check: an out-of-range observed
        category sets bad[n] and the flag `hc.check_inputs()` reports, and is replaced by 0 for the forward, so that the
        other rows of the chunk keep their values (`mpe`'s behaviour; the circuit's own check would turn the whole launch
        into NaN)."""
        s = self.s
        hc, zc = s.hc, s._z_circuit()
        nb = int(xc.shape[0])
        clean = torch.empty_like(xc)
        flag = hc._bad_input.data_ptr() if hc.validate_inputs else None
        capi.call("ck_flow_check_evidence", xc.data_ptr(), 1 if s.float_out else 0, hc._num_states_dev().data_ptr(), nb, s.D,
                  clean.data_ptr(), bad.data_ptr(), flag, stream)
        bd = zc._run(clean)
        zc._bad_input.zero_()  # (nothing can have set it; kept clean for `prepare()`'s forwards all the same)
        return bd

    def flow_pass(self, bd, stream: int) -> torch.Tensor:
        """The flows of every unit under the values of binding `bd`, layers last to first; returns the flow arena."""
        return self.down.run(bd, stream)

    def leaves(self, bd, flow: torch.Tensor, q: dict, gauss: bool, bad: torch.Tensor, out: torch.Tensor,
               logev: torch.Tensor | None, stream: int) -> None:
        """The posteriors of the chunk's rows into `out` (its first row), and their log evidence."""
        s = self.s
        root_ko = s.layers[s.root_layer]["Ko"]
        vals, fl, vo = bd.arena.data_ptr(), flow.data_ptr(), s._val_off_table(bd).data_ptr()
        leaf = (q["entries"].data_ptr(), q["start"].data_ptr(), q["Q"])
        tail = (fl, vals, vo, s.root_fold, root_ko, bad.data_ptr(), bd.B, out.data_ptr(),
                None if logev is None else logev.data_ptr(), stream)
        if gauss:
            capi.call("ck_flow_leaf_gaussian", *leaf, self._mean.data_ptr(), self._stddev.data_ptr(), *tail)
        else:
            capi.call("ck_flow_leaf_categorical", *leaf, q["C"], q["K_uniform"], self._ntab.data_ptr(), *tail)

    # -- once per call ------------------------------------------------------------------------------------------------
    def posterior_marginals(self, x: torch.Tensor, query_vars, return_log_evidence: bool = False,
                            rows_per_chunk: int | None = None):
        s = self.s
        ids = query_ids(query_vars, s.D)
        gauss = self.check_query(ids)  # (refusals first: nothing has been copied, prepared or launched)

        def start(B: int):
            q = self.query_tables(ids, gauss)
            out = torch.empty((B, q["Q"], q["C"]), dtype=torch.float32, device=s.device)
            logev = torch.empty(B, dtype=torch.float32, device=s.device)

            def tail(r0, xc, bd, flow, bad, stream):
                self.leaves(bd, flow, q, gauss, bad, out[r0], logev[r0:], stream)

            return (out, logev), tail

        out, logev = run_chunks(self, self.down, x, ids, rows_per_chunk, self.tables, start)
        return (out, logev) if return_log_evidence else out


def _state(hc: "HipCircuit") -> PosteriorState:
    s = sampler(hc)
    st = getattr(s, "_posterior", None)
    if st is None:
        st = s._posterior = PosteriorState(s)
    return st


def posterior_marginals(hc: "HipCircuit", x: torch.Tensor, query_vars, *, return_log_evidence: bool = False,
                        rows_per_chunk: int | None = None):
    """`HipCircuit.posterior_marginals`: see its docstring."""
    return _state(hc).posterior_marginals(x, query_vars, return_log_evidence, rows_per_chunk)


class PosteriorMarginalQuery:
    """Reference-shaped wrapper, next to `SamplingQuery`: ``PosteriorMarginalQuery(circuit)(x, query_vars=...)`` returns the
    ``(B, Q, C)`` posteriors of `HipCircuit.posterior_marginals`."""

    def __init__(self, circuit: "HipCircuit") -> None:
        check_plan(circuit.user_plan)
        self._circuit = circuit

    def __call__(self, x: torch.Tensor, *, query_vars):
        return posterior_marginals(self._circuit, x, query_vars)
