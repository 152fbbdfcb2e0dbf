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
weights, the evidence forward with its range check, the normalised input tables) unchanged; the message lists are built here
once per circuit, the log normalisers of the input units once per parameter state.  Kernels: cirkit_amd/csrc/ck_loo.hip.
"""

from __future__ import annotations

from typing import TYPE_CHECKING

import numpy as np
import torch

from . import _capi as capi
from .plan import Plan, resolve_fold_index
from .posterior import _SUM_KINDS, PosteriorState, _state, query_ids
from .sampling import _is_mixing, check_plan, chunk_rows

if TYPE_CHECKING:  # pragma: no cover
    from .circuit import HipCircuit


def message_lists(plan: Plan) -> list[dict | None]:
    """`posterior.consumer_lists` for the derivative pass: the same children, CSR offsets, list order and ``first`` marks, but
    every (fold, input position) pair has a message of its own, because an input receives the values of its SIBLINGS: sum /
    mixing and CP-T slot ``f H + h``, Tucker ``2 f + h``, and for Hadamard and Kronecker the pair (consumer's global fold,
    input position)."""
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
                if l.type in ("sum", "cpt"):
                    item = f * l.arity + h
                elif l.type == "tucker":
                    item = 2 * f + h
                else:  # hadamard, kronecker
                    item = (int(fold_off[j]) + f, h)
                lists.setdefault(int(g[f, h]), []).append(item)
        children = sorted(lists)
        start = np.concatenate([[0], np.cumsum([len(lists[c]) for c in children])]).astype(np.int32)
        items = np.array([it for c in children for it in lists[c]], dtype=np.int32).reshape(-1)
        first = np.array([c not in seen for c in children], dtype=np.int32)
        seen.update(children)
        slots = {"sum": l.num_folds * l.arity, "cpt": l.num_folds * l.arity, "tucker": 2 * l.num_folds}.get(l.type, 0)
        out[j] = {"children": np.array(children, dtype=np.int32), "start": start, "items": items, "first": first,
                  "slots": slots}
    return out


def variable_kinds(plan: Plan) -> dict[int, set[str]]:
    """Per variable in the scope of an input layer the kinds of the layers over it: "gaussian" and / or "discrete"."""
    kinds: dict[int, set[str]] = {}
    for l in plan.layers:
        if l.inputs is None and l.scope_idx is not None:
            for v in np.asarray(l.scope_idx[:, 0], dtype=np.int64):
                kinds.setdefault(int(v), set()).add("gaussian" if l.type == "gaussian" else "discrete")
    return kinds


def check_query_vars(kinds: dict[int, set[str]], ids: list[int]) -> bool:
    """Whether the query variables `ids` are Gaussian, given `variable_kinds`; raises for an empty, uncovered or mixed query
    set (the messages of `PosteriorState.check_query`).  Needs no device."""
    if not ids:
        raise ValueError("leave_one_out needs at least one query variable")
    missing = [v for v in ids if v not in kinds]
    if missing:
        raise ValueError(f"query variables {missing[:8]} are outside the scope of every input layer")
    seen = set().union(*(kinds[v] for v in ids))
    if len(seen) > 1:
        raise NotImplementedError("a query set that mixes discrete and Gaussian variables")
    return seen.pop() == "gaussian"


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
        self.kinds = variable_kinds(s.plan)
        self.covered = sorted(ps.var_folds)
        kind = np.zeros(s.D, dtype=np.int32)
        for v in self.covered:
            kind[v] = 2 if ps.gauss_var[v] else 1
        self._vkind = kind
        self._lists: list[dict | None] | None = None
        self.msg_per_row = 0
        self._queries: dict[tuple, dict] = {}
        self._all: dict | None = None
        self._key = None
        self._lz: torch.Tensor | None = None
        self._buffers: dict[int, tuple[torch.Tensor, torch.Tensor]] = {}  # chunk rows -> (derivative arena, messages)
        self.bytes_per_row = 2 * s.hc.arena_bytes(1)

    # -- refusals: nothing is prepared or launched before them -----------------------------------------------------------
    def check_query(self, ids: list[int]) -> bool:
        """Whether the query variables are Gaussian; raises for an empty, uncovered or mixed query set."""
        return check_query_vars(self.kinds, ids)

    # -- once per circuit --------------------------------------------------------------------------------------------
    def structure(self) -> list[dict | None]:
        if self._lists is None:
            dev = self.ps.s.device
            lists = message_lists(self.ps.s.plan)
            for j, c in enumerate(lists):
                if c is None:
                    continue
                for n in ("children", "start", "items", "first"):
                    c[n + "_d"] = torch.from_numpy(c[n]).to(dev)
                self.msg_per_row = max(self.msg_per_row, c["slots"] * self.ps.s.layers[j]["Ki"])
            self._lists = lists
            self.bytes_per_row += 4 * self.msg_per_row
        return self._lists

    def _entries(self, ids: list[int], gauss: bool | None) -> dict:
        """The leaf entries of the variables `ids` (gauss None: log probabilities, the table offset is not read)."""
        ps, s = self.ps, self.ps.s
        ent, start = [], [0]
        for v in ids:
            for j, f in ps.var_folds.get(v, []):
                d = s.layers[j]
                K, C = d["Ko"], 1 if (gauss or d["kind"] == capi.CK_SAMPLE_GAUSSIAN) else d["M"]
                ent.append((int(s.fold_off[j]) + f, K, C, ps.tab_off[j] + f * K * C, self.lz_off[j] + f * K))
            start.append(len(ent))
        e = np.array(ent, dtype=np.int64).reshape(-1, 5)
        units = np.add.reduceat(e[:, 1], np.array(start[:-1])[np.diff(start) > 0]) if len(ent) else np.zeros(1, dtype=np.int64)
        return {"entries": torch.from_numpy(e).to(s.device),
                "start": torch.from_numpy(np.array(start, dtype=np.int32)).to(s.device), "Q": len(ids),
                "C": 2 if gauss else int(e[:, 2].max()) if len(ent) else 1, "max_units": int(units.max())}

    def query_tables(self, ids: list[int], gauss: bool) -> dict:
        key = tuple(ids)
        q = self._queries.get(key)
        if q is None:
            if len(self._queries) >= 8:  # (a handful of query sets per circuit)
                self._queries.pop(next(iter(self._queries)))
            q = self._queries[key] = self._entries(ids, gauss)
        return q

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
        parts = []
        with torch.cuda.device(dev):
            zero = torch.zeros((), device=dev)
            ninf = torch.full((), float("-inf"), device=dev)
            for d in s.layers:
                if "scope" not in d:
                    continue
                if d["kind"] == capi.CK_SAMPLE_GAUSSIAN:
                    parts.append(torch.zeros(d["F"] * d["Ko"], dtype=torch.float32, device=dev))
                    continue
                M = d["M"]
                if d["spec"].type == "binomial":
                    t, is_log = d["tab"][:, :M, :].permute(0, 2, 1), True
                else:
                    t, is_log = d["tab"], bool(d["is_logits"])
                shift = zero
                if is_log:
                    mx = t.amax(dim=2, keepdim=True)
                    shift = torch.where(torch.isfinite(mx), mx, zero)
                    t = torch.exp(t - shift)
                tot = t.sum(dim=2, keepdim=True)
                lz = torch.where(tot > 0, torch.log(torch.where(tot > 0, tot, zero + 1)) + shift, ninf)
                parts.append(lz.to(torch.float32).contiguous().reshape(-1))
            self._lz = torch.cat(parts)
        self._key = s._key

    # -- per chunk: the phases (scripts/bench_leave_one_out.py times them one by one) ---------------------------------------
    def chunks_of(self, B: int, rows_per_chunk: int | None) -> list[tuple[int, int]]:
        """`PosteriorState.chunks_of` with this pass's bytes per row: the value arena, the derivative arena and the messages
        stay <= 2 GiB."""
        s = self.ps.s
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

    def derivative_pass(self, bd, stream: int) -> torch.Tensor:
        """The log derivatives of every unit under the values of binding `bd`, layers last to first; returns the arena."""
        s, lists = self.ps.s, self.structure()
        nb, dev = bd.B, s.device
        root_ko = s.layers[s.root_layer]["Ko"]
        buf = self._buffers.get(nb)
        if buf is None or buf[0].numel() != bd.arena.numel():
            msg = torch.empty(max(1, self.msg_per_row * nb), dtype=torch.float32, device=dev)
            # -inf: a fold nothing consumes is never written and has no derivative
            buf = self._buffers[nb] = (torch.full((bd.arena.numel(),), float("-inf"), dtype=torch.float32, device=dev), msg)
        der, msg = buf
        vals, dr, vo = bd.arena.data_ptr(), der.data_ptr(), s._val_off_table(bd).data_ptr()
        r_at = (bd.views[s.root_layer].data_ptr() - vals) // 4 + s.root_f * nb * root_ko
        root = der[r_at : r_at + nb * root_ko].view(nb, root_ko)
        root.fill_(float("-inf"))
        root[:, 0] = 0.0
        for j in range(len(s.layers) - 1, -1, -1):
            c, d = lists[j], s.layers[j]
            if c is None:
                continue
            F, H, Ki, Ko, kind = d["F"], d["H"], d["Ki"], d["Ko"], d["kind"]
            csr = (c["start_d"].data_ptr(), c["children_d"].data_ptr(), c["first_d"].data_ptr(), c["items_d"].data_ptr())
            if kind in _SUM_KINDS:
                capi.call("ck_loo_down_sum", kind, 1 if _is_mixing(d["spec"]) else 0, d["child"].data_ptr(),
                          d["w"].data_ptr(), F, H, Ki, Ko, d["M"], vals, dr, vo, int(s.fold_off[j]), nb, msg.data_ptr(), stream)
                capi.call("ck_loo_segment_lse", msg.data_ptr(), *csr, dr, vo, len(c["children"]), Ki, nb, stream)
            else:
                capi.call("ck_loo_down_product", kind, *csr, d["child"].data_ptr(), int(s.fold_off[j]), vals, dr, vo,
                          len(c["children"]), H, Ki, Ko, nb, stream)
        return der

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
        ps, s = self.ps, self.ps.s
        ids = self.covered if query_vars is None else query_ids(query_vars, s.D)
        gauss = self.check_query(ids)  # (refusals first: nothing has been copied, prepared or launched)
        xm = s.evidence_batch(x, [] if missing_vars is None else missing_vars)
        B = int(xm.shape[0])
        chunks = self.chunks_of(B, rows_per_chunk)
        self.tables()
        q = self.query_tables(ids, gauss)
        dev = s.device
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            out = torch.empty((B, q["Q"], q["C"]), dtype=torch.float32, device=dev)
            bad = torch.zeros(B, dtype=torch.int32, device=dev)
            for r0, nb in chunks:
                bd = ps.evidence_forward(xm[r0 : r0 + nb], bad[r0:], stream)
                der = self.derivative_pass(bd, stream)
                self.leaves(bd, der, q, gauss, bad[r0:], out[r0], stream)
        return out

    def conditional_log_probs(self, x: torch.Tensor, missing_vars, rows_per_chunk: int | None) -> torch.Tensor:
        ps, s = self.ps, self.ps.s
        xm = s.evidence_batch(x, [] if missing_vars is None else missing_vars)
        B = int(xm.shape[0])
        chunks = self.chunks_of(B, rows_per_chunk)
        self.tables()
        dev = s.device
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            out = torch.empty((B, s.D), dtype=torch.float32, device=dev)
            bad = torch.zeros(B, dtype=torch.int32, device=dev)
            for r0, nb in chunks:
                xc = xm[r0 : r0 + nb]
                bd = ps.evidence_forward(xc, bad[r0:], stream)
                der = self.derivative_pass(bd, stream)
                self.log_probs(bd, der, xc, bad[r0:], out[r0], stream)
        return out


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
