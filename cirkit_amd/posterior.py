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
from .plan import Plan, resolve_fold_index
from .sampling import Sampler, _is_mixing, check_plan, chunk_rows, sampler

if TYPE_CHECKING:  # pragma: no cover
    from .circuit import HipCircuit

_SUM_KINDS = (capi.CK_SAMPLE_SUM, capi.CK_SAMPLE_CPT, capi.CK_SAMPLE_TUCKER)


def consumer_lists(plan: Plan) -> list[dict | None]:
    """Per layer (None for input layers) the consumer lists of the folds it reads, for the flow pass: ``children`` the
    global folds it feeds, ascending; ``start`` the CSR offsets into ``items``; ``items`` what each child adds, in (fold,
    input position) order -- a message slot for sum-type layers (sum / mixing ``f H + h``, CP-T ``f``, Tucker ``2 f + h``),
    the consumer's global fold for Hadamard, the pair (consumer's global fold, input position) for Kronecker; ``first``
    whether no LATER layer feeds the child (the pass walks the layers last to first: the first writer stores)."""
    folds = [l.num_folds for l in plan.layers]
    fold_off = np.concatenate([[0], np.cumsum(folds)]).astype(np.int64)
    out: list[dict | None] = [None] * len(plan.layers)
    seen: set[int] = set()
    for j in range(len(plan.layers) - 1, -1, -1):
        l = plan.layers[j]
        if l.inputs is None:
            continue
        ch = resolve_fold_index(l.inputs, folds)  # (F, H, 2)
        g = fold_off[ch[..., 0]] + ch[..., 1]  # (F, H) global folds
        lists: dict[int, list] = {}
        for f in range(l.num_folds):
            for h in range(l.arity):
                if l.type == "sum":
                    item = f * l.arity + h
                elif l.type == "cpt":
                    item = f
                elif l.type == "tucker":
                    item = 2 * f + h
                elif l.type == "hadamard":
                    item = int(fold_off[j]) + f
                else:  # kronecker
                    item = (int(fold_off[j]) + f, h)
                lists.setdefault(int(g[f, h]), []).append(item)
        children = sorted(lists)
        start = np.concatenate([[0], np.cumsum([len(lists[c]) for c in children])]).astype(np.int32)
        items = np.array([it for c in children for it in lists[c]], dtype=np.int32).reshape(-1)
        first = np.array([c not in seen for c in children], dtype=np.int32)
        seen.update(children)
        slots = {"sum": l.num_folds * l.arity, "cpt": l.num_folds, "tucker": 2 * l.num_folds}.get(l.type, 0)
        out[j] = {"children": np.array(children, dtype=np.int32), "start": start, "items": items, "first": first,
                  "slots": slots}
    return out


def num_consumers(plan: Plan) -> np.ndarray:
    """(total folds) how many (fold, input position) pairs read each global fold."""
    n = np.zeros(int(sum(l.num_folds for l in plan.layers)), dtype=np.int64)
    for c in consumer_lists(plan):
        if c is not None:
            n[c["children"]] += np.diff(c["start"])
    return n


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
        plan = s.plan
        self.var_folds: dict[int, list[tuple[int, int]]] = {}  # variable -> [(input layer, fold)]
        self.gauss_var: dict[int, bool] = {}
        self.tab_off: dict[int, int] = {}  # input layer -> element offset of its block in the per-state flat tables
        n_cat = n_gauss = 0
        for j, d in enumerate(s.layers):
            if "scope" not in d:
                continue
            gauss = d["kind"] == capi.CK_SAMPLE_GAUSSIAN
            for f, v in enumerate(np.asarray(d["spec"].scope_idx[:, 0], dtype=np.int64)):
                self.var_folds.setdefault(int(v), []).append((j, f))
                self.gauss_var[int(v)] = gauss or self.gauss_var.get(int(v), False)
            if gauss:
                self.tab_off[j], n_gauss = n_gauss, n_gauss + d["F"] * d["Ko"]
            else:
                self.tab_off[j], n_cat = n_cat, n_cat + d["F"] * d["Ko"] * d["M"]
        self.mixed_var = {v for v, fl in self.var_folds.items()
                          if len({s.layers[j]["kind"] == capi.CK_SAMPLE_GAUSSIAN for j, _ in fl}) > 1}
        self._lists: list[dict | None] | None = None
        self.msg_per_row = 0
        self._queries: dict[tuple, dict] = {}
        self._key = None
        self._ntab: torch.Tensor | None = None
        self._mean: torch.Tensor | None = None
        self._stddev: torch.Tensor | None = None
        self._buffers: dict[int, tuple[torch.Tensor, torch.Tensor | None]] = {}  # chunk rows -> (flow arena, messages)
        self.bytes_per_row = 2 * s.hc.arena_bytes(1)

    # -- refusals: nothing is prepared or launched before them -----------------------------------------------------------
    def check_query(self, ids: list[int]) -> bool:
        """Whether the query variables are Gaussian; raises for an empty, uncovered or mixed query set."""
        if not ids:
            raise ValueError("posterior_marginals needs at least one query variable")
        missing = [v for v in ids if v not in self.var_folds]
        if missing:
            raise ValueError(f"query variables {missing[:8]} are outside the scope of every input layer")
        kinds = {self.gauss_var[v] for v in ids}
        if len(kinds) > 1 or any(v in self.mixed_var for v in ids):
            raise NotImplementedError("a query set that mixes discrete and Gaussian variables")
        return kinds.pop()

    # -- once per circuit --------------------------------------------------------------------------------------------
    def structure(self) -> list[dict | None]:
        if self._lists is None:
            dev = self.s.device
            lists = consumer_lists(self.s.plan)
            for j, c in enumerate(lists):
                if c is None:
                    continue
                for n in ("children", "start", "items", "first"):
                    c[n + "_d"] = torch.from_numpy(c[n]).to(dev)
                self.msg_per_row = max(self.msg_per_row, c["slots"] * self.s.layers[j]["Ki"])
            self._lists = lists
            self.bytes_per_row += 4 * self.msg_per_row
        return self._lists

    def query_tables(self, ids: list[int], gauss: bool) -> dict:
        key = tuple(ids)
        q = self._queries.get(key)
        if q is None:
            s = self.s
            ent, start = [], [0]
            for v in ids:
                for j, f in self.var_folds[v]:
                    d = s.layers[j]
                    K, C = d["Ko"], 1 if gauss else d["M"]
                    ent.append((int(s.fold_off[j]) + f, K, C, self.tab_off[j] + f * K * C))
                start.append(len(ent))
            e = np.array(ent, dtype=np.int64)
            ks = set(e[:, 1].tolist())
            if len(self._queries) >= 8:  # (a handful of query sets per circuit; the tables are small but not free)
                self._queries.pop(next(iter(self._queries)))
            q = self._queries[key] = {
                "entries": torch.from_numpy(e).to(s.device), "start": torch.from_numpy(np.array(start, dtype=np.int32)).to(s.device),
                "Q": len(ids), "C": 2 if gauss else int(e[:, 2].max()),
                "K_uniform": ks.pop() if len(ks) == 1 and next(iter(ks)) in (32, 64) else 0}
        return q

    # -- once per parameter state ------------------------------------------------------------------------------------
    def tables(self) -> None:
        """The normalised table rows of the Categorical / Binomial layers ((F, K, C) blocks of one flat buffer) and the
        Gaussian layers' means and standard deviations, for the store's current values."""
        s = self.s
        s.prepare()
        if self._key == s._key:
            return
        dev = s.device
        cats, means, sds = [], [], []
        with torch.cuda.device(dev):
            zero = torch.zeros((), device=dev)
            for d in s.layers:
                if "scope" not in d:
                    continue
                if d["kind"] == capi.CK_SAMPLE_GAUSSIAN:
                    means.append(d["mean_v"].reshape(-1))
                    sds.append(d["stddev_v"].reshape(-1))
                    continue
                M = d["M"]
                if d["spec"].type == "binomial":  # prepare()'s (F, T + 2, K) log-pmf table, last row the integral
                    t, is_log = d["tab"][:, :M, :].permute(0, 2, 1), True
                else:  # prepare()'s (F, K, C) probabilities or logits
                    t, is_log = d["tab"], bool(d["is_logits"])
                if is_log:
                    mx = t.amax(dim=2, keepdim=True)
                    t = torch.exp(t - torch.where(torch.isfinite(mx), mx, zero))
                tot = t.sum(dim=2, keepdim=True)
                cats.append(torch.where(tot > 0, t / tot, zero).contiguous().reshape(-1))
            self._ntab = torch.cat(cats) if cats else None
            self._mean = torch.cat(means) if means else None
            self._stddev = torch.cat(sds) if sds else None
        self._key = s._key

    # -- per chunk: the three phases (scripts/bench_posterior.py times them one by one) ------------------------------------
    def chunks_of(self, B: int, rows_per_chunk: int | None) -> list[tuple[int, int]]:
        """The (first row, rows) chunks of a batch, with the bindings and buffers of other sizes released (two sizes stay
        bound: the chunk and the tail)."""
        s = self.s
        self.structure()
        chunks = chunk_rows(B, rows_per_chunk, self.bytes_per_row)
        sizes = {nb for _, nb in chunks}
        zc = s._z_circuit()
        for b in [b for b in zc._bindings if b != 1 and b not in sizes]:
            zc._bindings.pop(b).destroy()
            s._val_off.pop(b, None)
        for b in [b for b in self._buffers if b not in sizes]:
            del self._buffers[b]
        return chunks

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
        s, lists = self.s, self.structure()
        nb, dev = bd.B, s.device
        root_ko = s.layers[s.root_layer]["Ko"]
        buf = self._buffers.get(nb)
        if buf is None or buf[0].numel() != bd.arena.numel():
            msg = torch.empty(max(1, self.msg_per_row * nb), dtype=torch.float32, device=dev)
            # zeros: a fold nothing consumes is never written and carries no flow
            buf = self._buffers[nb] = (torch.zeros(bd.arena.numel(), dtype=torch.float32, device=dev), msg)
        flow, msg = buf
        vals, fl, vo = bd.arena.data_ptr(), flow.data_ptr(), s._val_off_table(bd).data_ptr()
        r_at = (bd.views[s.root_layer].data_ptr() - vals) // 4 + s.root_f * nb * root_ko
        root = flow[r_at : r_at + nb * root_ko].view(nb, root_ko)
        root.zero_()
        root[:, 0] = 1.0
        for j in range(len(s.layers) - 1, -1, -1):
            c, d = lists[j], s.layers[j]
            if c is None:
                continue
            F, H, Ki, Ko, kind = d["F"], d["H"], d["Ki"], d["Ko"], d["kind"]
            csr = (c["start_d"].data_ptr(), c["children_d"].data_ptr(), c["first_d"].data_ptr(), c["items_d"].data_ptr())
            if kind in _SUM_KINDS:
                capi.call("ck_flow_down_sum", kind, 1 if _is_mixing(d["spec"]) else 0, d["child"].data_ptr(),
                          d["w"].data_ptr(), F, H, Ki, Ko, d["M"], vals, fl, vo, int(s.fold_off[j]), nb, msg.data_ptr(), stream)
                capi.call("ck_flow_segment_add", msg.data_ptr(), *csr, fl, vo, len(c["children"]), Ki, nb, stream)
            else:
                capi.call("ck_flow_down_product", kind, *csr, fl, vo, len(c["children"]), H, Ki, Ko, nb, stream)
        return flow

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
        xm = s.evidence_batch(x, ids)
        B = int(xm.shape[0])
        chunks = self.chunks_of(B, rows_per_chunk)
        self.tables()
        q = self.query_tables(ids, gauss)
        dev = s.device
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            out = torch.empty((B, q["Q"], q["C"]), dtype=torch.float32, device=dev)
            logev = torch.empty(B, dtype=torch.float32, device=dev)
            bad = torch.zeros(B, dtype=torch.int32, device=dev)
            for r0, nb in chunks:
                bd = self.evidence_forward(xm[r0 : r0 + nb], bad[r0:], stream)
                flow = self.flow_pass(bd, stream)
                self.leaves(bd, flow, q, gauss, bad[r0:], out[r0], logev[r0:], stream)
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
