"""Batch-summed expected statistics on the GPU: `HipCircuit.expected_statistics` ("Expected
statistics").

The E-step of EM as a query: the expected sufficient statistics of every parameter under ``p(. | x_O)``, summed over the rows
of a batch, missing values integrated out.  It is the flow pass of `posterior_marginals` (cirkit_amd/posterior.py) reduced
over the batch: with ``v`` the unit values of the evidence forward, ``f`` the flows and ``e_i`` the child value of entry ``i``,

* a sum-type unit ``k`` gives entry ``i`` the expected edge flow ``N[k, i] = sum_n f_k w[k, i] exp(e_i - v_k)``;
* an input unit gives its flow to the state the row observes, or spreads it over its own distribution where the row misses
  the variable (Gaussian units: the flow-weighted moments);
* every unit gives ``sum_n f_k``.

Only LIVE rows count: evidence in range and a finite root value.  Nothing is written into the parameter store; `normalised`
turns the sums into the closed-form M-step targets, and applying those through a plan's parameter graphs (softmax and other
re-parameterisations) is the caller's business.  The reference has no such query.  This module reuses the circuit's `Sampler`
and `PosteriorState` (evidence forward, flow pass, normalised tables) unchanged.  Kernels: cirkit_amd/csrc/ck_stats.hip.
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import TYPE_CHECKING

import numpy as np
import torch

from . import _capi as capi
from .posterior import PosteriorState, _state, query_ids
from .sampling import _is_mixing, check_plan
from .topdown import SUM_KINDS, run_chunks

if TYPE_CHECKING:  # pragma: no cover
    from .circuit import HipCircuit

SCRATCH_FLOATS = 1 << 21  # ck_stats_edge_sum's bound on its partial tiles: fewer than 2048 tiles of 1024 floats, 8 MiB


@dataclass
class ExpectedStatistics:
    """The result of `HipCircuit.expected_statistics`: fp32 on the circuit's device, indexed by the USER plan's layer index.

    ``edge[j]`` (F, Ko, M) for every sum-type layer, ``leaf[j]`` (F, K, C) for every Categorical / Binomial layer and
    (F, K, 3) = (sum f, sum f m1, sum f m2) for every Gaussian layer, ``unit[j]`` (F, Ko) for every layer, ``log_evidence``
    (B,) (NaN for out-of-range rows), ``rows`` the number of live rows (0-d int64).  ``support[j]``: where the weight (the
    normalised table) behind ``edge[j]`` (a discrete ``leaf[j]``) is positive; ``kinds[j]`` the layer type."""

    edge: dict[int, torch.Tensor]
    leaf: dict[int, torch.Tensor]
    unit: list[torch.Tensor]
    log_evidence: torch.Tensor
    rows: torch.Tensor
    support: dict[int, torch.Tensor] = field(default_factory=dict)
    kinds: list[str] = field(default_factory=list)
    total_count: dict[int, int] = field(default_factory=dict)

    def normalised(self, pseudocount: float = 0.0) -> dict[int, torch.Tensor | tuple[torch.Tensor, torch.Tensor]]:
        """The closed-form M-step targets per layer, nothing written anywhere.  Sum-type layers: ``(edge + pseudocount
        [w > 0])`` divided by its sum over the entries -- weight rows that sum to 1, 0 where a row has no mass.  Categorical
        layers: the same over the states.  Binomial layers: the success probability ``sum_c c N_c / (T sum_c N_c)`` (F, K).
        Gaussian layers: ``(mean, variance)`` from the three sums, 0 where a unit has no flow.  Putting these back through a
        plan's parameter graphs (a softmax wants their logarithm, a mixing weight its diagonal) is the caller's business."""
        a = float(pseudocount)
        out: dict = {}

        def rows_to_one(n: torch.Tensor, sup: torch.Tensor) -> torch.Tensor:
            n = n + a * sup.to(n.dtype)
            den = n.sum(dim=-1, keepdim=True)
            return torch.where(den > 0, n / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(n))

        for j, n in self.edge.items():
            out[j] = rows_to_one(n, self.support[j])
        for j, n in self.leaf.items():
            if self.kinds[j] == "gaussian":
                s0, s1, s2 = n[..., 0], n[..., 1], n[..., 2]
                ok = s0 > 0
                den = torch.where(ok, s0, torch.ones_like(s0))
                mean = torch.where(ok, s1 / den, torch.zeros_like(s0))
                out[j] = (mean, torch.where(ok, s2 / den - mean * mean, torch.zeros_like(s0)))
            elif self.kinds[j] == "binomial":
                T = self.total_count[j]
                c = torch.arange(n.shape[-1], dtype=n.dtype, device=n.device)
                tot = n.sum(dim=-1)
                out[j] = torch.where(tot > 0, (n * c).sum(dim=-1) / (T * torch.where(tot > 0, tot, torch.ones_like(tot))),
                                     torch.zeros_like(tot))
            else:
                out[j] = rows_to_one(n, self.support[j])
        return out


def _entry_columns(spec, user_spec) -> np.ndarray | None:
    """The entries of a padded (F, Ko, M) weight that the user's plan has, in its order; None when nothing was padded."""
    kp, ku = spec.num_input_units, user_spec.num_input_units
    if kp == ku:
        return None
    if spec.type == "cpt":
        return np.arange(ku)
    if spec.type == "tucker":
        return (np.arange(ku)[:, None] * kp + np.arange(ku)[None, :]).reshape(-1)
    return (np.arange(spec.arity)[:, None] * kp + np.arange(ku)[None, :]).reshape(-1)


class ExpectedState:
    """The expected-statistics state of one `HipCircuit`, next to its `PosteriorState`."""

    def __init__(self, ps: PosteriorState) -> None:
        self.ps = ps
        s = ps.s
        dev = s.device
        folds = [d["F"] for d in s.layers]
        units = [d["Ko"] for d in s.layers]
        self.unit_at = np.concatenate([[0], np.cumsum([f * k for f, k in zip(folds, units)])]).astype(np.int64)
        self.fold_ko = torch.from_numpy(np.repeat(np.array(units, dtype=np.int32), folds)).to(dev)
        self.unit_off = torch.from_numpy(np.concatenate(
            [self.unit_at[j] + np.arange(f, dtype=np.int64) * k for j, (f, k) in enumerate(zip(folds, units))])).to(dev)
        user = s.hc.user_plan.layers
        self.cols = [None if "child" not in d or d["kind"] not in SUM_KINDS else _entry_columns(d["spec"], us)
                     for d, us in zip(s.layers, user)]
        self.cols_d = [None if c is None else torch.from_numpy(c).to(dev) for c in self.cols]
        self._scratch: torch.Tensor | None = None

    # -- per chunk: the three phases behind the flow pass (scripts/bench_expected_statistics.py times them one by one) ------
    def unit_sums(self, bd, flow: torch.Tensor, live: torch.Tensor, unit: torch.Tensor, stream: int) -> None:
        s = self.ps.s
        capi.call("ck_stats_unit_sum", flow.data_ptr(), s._val_off_table(bd).data_ptr(), self.fold_ko.data_ptr(),
                  self.unit_off.data_ptr(), s.total_folds, live.data_ptr(), bd.B, unit.data_ptr(), stream)

    def edge_sums(self, bd, flow: torch.Tensor, live: torch.Tensor, edge: dict, stream: int) -> None:
        s = self.ps.s
        if self._scratch is None:
            self._scratch = torch.empty(SCRATCH_FLOATS, dtype=torch.float32, device=s.device)
        vals, fl, vo = bd.arena.data_ptr(), flow.data_ptr(), s._val_off_table(bd).data_ptr()
        for j, d in enumerate(s.layers):
            if d["kind"] in SUM_KINDS:
                capi.call("ck_stats_edge_sum", d["kind"], 1 if _is_mixing(d["spec"]) else 0, d["child"].data_ptr(),
                          d["w"].data_ptr(), d["F"], d["H"], d["Ki"], d["Ko"], d["M"], vals, fl, vo, int(s.fold_off[j]),
                          live.data_ptr(), bd.B, edge[j].data_ptr(), self._scratch.data_ptr(), SCRATCH_FLOATS, stream)

    def leaf_sums(self, bd, flow: torch.Tensor, xc: torch.Tensor, live: torch.Tensor, leaf: dict, stream: int) -> None:
        ps, s = self.ps, self.ps.s
        fl, vo, lv = flow.data_ptr(), s._val_off_table(bd).data_ptr(), live.data_ptr()
        for j, d in enumerate(s.layers):
            if "scope" not in d:
                continue
            g0 = int(s.fold_off[j])
            if d["kind"] == capi.CK_SAMPLE_GAUSSIAN:
                capi.call("ck_stats_leaf_gaussian", d["scope"].data_ptr(), d["mean_v"].data_ptr(), d["stddev_v"].data_ptr(),
                          d["F"], d["Ko"], xc.data_ptr(), s.D, fl, vo, g0, lv, bd.B, leaf[j].data_ptr(), stream)
            else:
                nt = ps._ntab[ps.tab_off[j] :]
                capi.call("ck_stats_leaf_categorical", d["scope"].data_ptr(), nt.data_ptr(), d["F"], d["Ko"], d["M"],
                          xc.data_ptr(), 1 if s.float_out else 0, s.D, fl, vo, g0, lv, bd.B, leaf[j].data_ptr(), stream)

    def accumulators(self) -> tuple[dict, dict, torch.Tensor]:
        """Zeroed (edge, leaf, unit) accumulators in the DEVICE plan's shapes, after `PosteriorState.tables()`."""
        s = self.ps.s
        dev = s.device
        edge = {j: torch.zeros_like(d["w"]) for j, d in enumerate(s.layers) if d["kind"] in SUM_KINDS}
        leaf = {j: torch.zeros((d["F"], d["Ko"], 3 if d["kind"] == capi.CK_SAMPLE_GAUSSIAN else d["M"]), dtype=torch.float32,
                               device=dev) for j, d in enumerate(s.layers) if "scope" in d}
        return edge, leaf, torch.zeros(int(self.unit_at[-1]), dtype=torch.float32, device=dev)

    def device_statistics(self, x: torch.Tensor, missing_vars, rows_per_chunk: int | None, into: tuple | None = None):
        """The sums of a batch in the DEVICE plan's shapes, nothing sliced: ``(edge, leaf, unit, log_evidence, rows)``.  With
        `into` = an earlier (edge, leaf, unit) the batch is ADDED to those accumulators, in call order (`HipEMTrainer`'s
        running sums over several batches); otherwise they start at zero."""
        ps, s = self.ps, self.ps.s
        ids = [] if missing_vars is None else query_ids(missing_vars, s.D)  # (refusals first: nothing copied or launched)

        def start(B: int):
            dev = s.device
            edge, leaf, unit = self.accumulators() if into is None else into
            logev = torch.empty(B, dtype=torch.float32, device=dev)
            rows = torch.zeros((), dtype=torch.int64, device=dev)
            nan = torch.full((), float("nan"), device=dev)

            def tail(r0, xc, bd, flow, bad, stream):
                root = bd.views[s.root_layer][s.root_f, :, 0]
                ok = bad[: bd.B] == 0
                live = (ok & torch.isfinite(root)).to(torch.int32)
                logev[r0 : r0 + bd.B] = torch.where(ok, root, nan)
                rows.add_(live.sum())
                self.unit_sums(bd, flow, live, unit, stream)
                self.edge_sums(bd, flow, live, edge, stream)
                self.leaf_sums(bd, flow, xc, live, leaf, stream)

            return (edge, leaf, unit, logev, rows), tail

        return run_chunks(ps, ps.down, x, ids, rows_per_chunk, ps.tables, start)

    def expected_statistics(self, x: torch.Tensor, missing_vars, rows_per_chunk: int | None) -> ExpectedStatistics:
        ps, s = self.ps, self.ps.s
        edge, leaf, unit, logev, rows = self.device_statistics(x, missing_vars, rows_per_chunk)
        user = s.hc.user_plan.layers
        with torch.cuda.device(s.device):
            # back to the user plan's unit counts (a padded unit carries no flow, a padded entry has weight 0)
            res = ExpectedStatistics({}, {}, [], logev, rows, kinds=[l.type for l in user])
            for j, (d, us) in enumerate(zip(s.layers, user)):
                ko = us.num_output_units
                res.unit.append(unit[int(self.unit_at[j]) : int(self.unit_at[j + 1])].view(d["F"], d["Ko"])[:, :ko])
                if j in edge:
                    e, w = edge[j][:, :ko], d["w"][:, :ko]
                    if self.cols_d[j] is not None:
                        e, w = e[:, :, self.cols_d[j]], w[:, :, self.cols_d[j]]
                    res.edge[j], res.support[j] = e, w > 0
                elif j in leaf:
                    res.leaf[j] = leaf[j][:, :ko]
                    if d["kind"] != capi.CK_SAMPLE_GAUSSIAN:
                        nt = ps._ntab[ps.tab_off[j] : ps.tab_off[j] + d["F"] * d["Ko"] * d["M"]].view(d["F"], d["Ko"], d["M"])
                        res.support[j] = nt[:, :ko] > 0
                        if us.type == "binomial":
                            res.total_count[j] = int(us.config["total_count"])
        return res


def _expected(hc: "HipCircuit") -> ExpectedState:
    ps = _state(hc)
    st = getattr(ps, "_expected", None)
    if st is None:
        st = ps._expected = ExpectedState(ps)
    return st


def expected_statistics(hc: "HipCircuit", x: torch.Tensor, missing_vars=None, *, rows_per_chunk: int | None = None):
    """`HipCircuit.expected_statistics`: see its docstring."""
    return _expected(hc).expected_statistics(x, missing_vars, rows_per_chunk)


class ExpectedStatisticsQuery:
    """Reference-shaped wrapper, next to `PosteriorMarginalQuery`: ``ExpectedStatisticsQuery(circuit)(x, missing_vars=...)``
    returns the `ExpectedStatistics` of `HipCircuit.expected_statistics`."""

    def __init__(self, circuit: "HipCircuit") -> None:
        check_plan(circuit.user_plan)
        self._circuit = circuit

    def __call__(self, x: torch.Tensor, *, missing_vars=None):
        return expected_statistics(self._circuit, x, missing_vars)
