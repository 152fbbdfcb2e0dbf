"""The top-down message pass behind the flow and derivative queries ("The top-down message pass").

`posterior_marginals`, `expected_statistics` and `HipEMTrainer` walk the FLOW of every unit down the circuit, `leave_one_out`
and `conditional_log_probs` the log DERIVATIVE.  Both passes are one layer loop over the evidence forward's values: a sum-type
layer writes its messages and every child fold combines those of its consumers, a product layer hands its own arena values
on.  What they share lives here: the consumer lists, the pass with its buffers and chunking, the leaf-entry tables of a query
set, the normalisation of the discrete input tables, the query-set check and the per-chunk driver.  Kernels:
cirkit_amd/csrc/ck_down.h, instantiated by ck_flow.hip and ck_loo.hip.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _capi as capi
from .plan import Plan, resolve_fold_index
from .sampling import Sampler, _is_mixing, chunk_rows

SUM_KINDS = (capi.CK_SAMPLE_SUM, capi.CK_SAMPLE_CPT, capi.CK_SAMPLE_TUCKER)


def consumer_lists(plan: Plan, per_input: bool) -> list[dict | None]:
    """Per layer (None for input layers) the consumer lists of the folds it reads: ``children`` the global folds it feeds,
    ascending; ``start`` the CSR offsets into ``items``; ``items`` what each child combines, in (fold, input position) order;
    ``first`` whether no LATER layer feeds the child (the pass walks the layers last to first: the first writer stores);
    ``slots`` the number of message slots of a sum-type layer.

    An item of a sum-type layer is a message slot: sum / mixing ``f H + h``, Tucker ``2 f + h``, CP-T ``f`` -- or, with
    `per_input`, ``f H + h``: every (fold, input position) pair has a message of its own, because an input receives the
    values of its SIBLINGS.  An item of a product layer is read from the arena itself: the pair (consumer's global fold, input
    position) for Kronecker and, with `per_input`, for Hadamard; otherwise Hadamard's item is the consumer's global fold."""
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
        shared = l.type == "cpt" and not per_input  # (one message per fold, read by all its inputs)
        lists: dict[int, list] = {}
        for f in range(l.num_folds):
            for h in range(l.arity):
                if shared:
                    item = f
                elif l.type in ("sum", "cpt", "tucker"):
                    item = f * l.arity + h
                elif l.type == "hadamard" and not per_input:
                    item = int(fold_off[j]) + f
                else:  # kronecker, hadamard per input
                    item = (int(fold_off[j]) + f, h)
                lists.setdefault(int(g[f, h]), []).append(item)
        children = sorted(lists)
        start = np.concatenate([[0], np.cumsum([len(lists[c]) for c in children])]).astype(np.int32)
        items = np.array([it for c in children for it in lists[c]], dtype=np.int32).reshape(-1)
        first = np.array([c not in seen for c in children], dtype=np.int32)
        seen.update(children)
        slots = 0 if l.type not in ("sum", "cpt", "tucker") else l.num_folds * (1 if shared else l.arity)
        out[j] = {"children": np.array(children, dtype=np.int32), "start": start, "items": items, "first": first,
                  "slots": slots}
    return out


def num_consumers(plan: Plan) -> np.ndarray:
    """(total folds) how many (fold, input position) pairs read each global fold."""
    n = np.zeros(int(sum(l.num_folds for l in plan.layers)), dtype=np.int64)
    for c in consumer_lists(plan, False):
        if c is not None:
            n[c["children"]] += np.diff(c["start"])
    return n


def variable_kinds(plan: Plan) -> dict[int, set[str]]:
    """Per variable in the scope of an input layer the kinds of the layers over it: "gaussian" and / or "discrete"."""
    kinds: dict[int, set[str]] = {}
    for l in plan.layers:
        if l.inputs is None and l.scope_idx is not None:
            for v in np.asarray(l.scope_idx[:, 0], dtype=np.int64):
                kinds.setdefault(int(v), set()).add("gaussian" if l.type == "gaussian" else "discrete")
    return kinds


def check_query(kinds: dict[int, set[str]], ids: list[int], what: str) -> bool:
    """Whether the query variables `ids` of query `what` are Gaussian, given `variable_kinds`; raises for an empty, uncovered
    or mixed query set.  Needs no device."""
    if not ids:
        raise ValueError(f"{what} needs at least one query variable")
    missing = [v for v in ids if v not in kinds]
    if missing:
        raise ValueError(f"query variables {missing[:8]} are outside the scope of every input layer")
    seen = set().union(*(kinds[v] for v in ids))
    if len(seen) > 1:
        raise NotImplementedError("a query set that mixes discrete and Gaussian variables")
    return seen.pop() == "gaussian"


@dataclass(frozen=True)
class PassKind:
    """What tells the two passes apart on the host: the list mode, the arena value of a fold nothing consumes (it is never
    written), the root unit's value and the entry points.  The product call of a `per_input` pass also reads the siblings'
    values: it carries the layer's child folds, its first global fold and the value arena."""

    per_input: bool
    fill: float
    root: float
    down_sum: str
    segment: str
    down_product: str


FLOW = PassKind(False, 0.0, 1.0, "ck_flow_down_sum", "ck_flow_segment_add", "ck_flow_down_product")
DERIVATIVE = PassKind(True, float("-inf"), 0.0, "ck_loo_down_sum", "ck_loo_segment_lse", "ck_loo_down_product")


class TopDownPass:
    """One pass of a `Sampler`'s circuit: its consumer lists on the device, its arena and message buffers per chunk size."""

    def __init__(self, s: Sampler, kind: PassKind) -> None:
        self.s, self.kind = s, kind
        self._lists: list[dict | None] | None = None
        self.msg_per_row = 0
        self._buffers: dict[int, tuple[torch.Tensor, torch.Tensor]] = {}  # chunk rows -> (arena, messages)
        self.bytes_per_row = 2 * s.hc.arena_bytes(1)

    def structure(self) -> list[dict | None]:
        """Once per circuit: the lists, with device copies under ``<name>_d``."""
        if self._lists is None:
            dev = self.s.device
            lists = consumer_lists(self.s.plan, self.kind.per_input)
            for j, c in enumerate(lists):
                if c is None:
                    continue
                for n in ("children", "start", "items", "first"):
                    c[n + "_d"] = torch.from_numpy(c[n]).to(dev)
                self.msg_per_row = max(self.msg_per_row, c["slots"] * self.s.layers[j]["Ki"])
            self._lists = lists
            self.bytes_per_row += 4 * self.msg_per_row
        return self._lists

    def chunks_of(self, B: int, rows_per_chunk: int | None) -> list[tuple[int, int]]:
        """The (first row, rows) chunks of a batch -- the value arena, this pass's arena and its messages stay <= 2 GiB --
        with the bindings and buffers of other sizes released (two sizes stay bound: the chunk and the tail)."""
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

    def run(self, bd, stream: int) -> torch.Tensor:
        """The pass under the values of binding `bd`, layers last to first; returns the arena."""
        s, kind, lists = self.s, self.kind, self.structure()
        nb, dev = bd.B, s.device
        root_ko = s.layers[s.root_layer]["Ko"]
        buf = self._buffers.get(nb)
        if buf is None or buf[0].numel() != bd.arena.numel():
            msg = torch.empty(max(1, self.msg_per_row * nb), dtype=torch.float32, device=dev)
            buf = self._buffers[nb] = (torch.full((bd.arena.numel(),), kind.fill, dtype=torch.float32, device=dev), msg)
        arena, msg = buf
        vals, ar, vo = bd.arena.data_ptr(), arena.data_ptr(), s._val_off_table(bd).data_ptr()
        r_at = (bd.views[s.root_layer].data_ptr() - vals) // 4 + s.root_f * nb * root_ko
        root = arena[r_at : r_at + nb * root_ko].view(nb, root_ko)
        root.fill_(kind.fill)
        root[:, 0] = kind.root
        for j in range(len(s.layers) - 1, -1, -1):
            c, d = lists[j], s.layers[j]
            if c is None:
                continue
            F, H, Ki, Ko = d["F"], d["H"], d["Ki"], d["Ko"]
            csr = (c["start_d"].data_ptr(), c["children_d"].data_ptr(), c["first_d"].data_ptr(), c["items_d"].data_ptr())
            if d["kind"] in SUM_KINDS:
                capi.call(kind.down_sum, d["kind"], 1 if _is_mixing(d["spec"]) else 0, d["child"].data_ptr(), d["w"].data_ptr(),
                          F, H, Ki, Ko, d["M"], vals, ar, vo, int(s.fold_off[j]), nb, msg.data_ptr(), stream)
                capi.call(kind.segment, msg.data_ptr(), *csr, ar, vo, len(c["children"]), Ki, nb, stream)
            else:
                siblings = (d["child"].data_ptr(), int(s.fold_off[j]), vals) if kind.per_input else ()
                capi.call(kind.down_product, d["kind"], *csr, *siblings, ar, vo, len(c["children"]), H, Ki, Ko, nb, stream)
        return arena


def leaf_entries(s: Sampler, var_folds: dict, tab_off: dict, ids: list[int], gauss: bool | None,
                 lz_off: dict | None = None) -> tuple[dict, np.ndarray, list[int]]:
    """The leaf-entry table of the variables `ids`, one row per input fold over a variable: (global fold, units K, states C
    of the fold's table, element offset of its (K, C) block in the flat normalised tables -- or of its K means / standard
    deviations) and, with `lz_off`, a fifth column: the element offset of its K log normalisers.  C is 1 for a Gaussian
    fold (gauss None: the folds of both kinds are listed).  Returns the device tables ``entries``, ``start`` (CSR over the
    variables), ``Q`` and the output width ``C``, and the host copies of the rows and of ``start``."""
    ent, start = [], [0]
    for v in ids:
        for j, f in var_folds.get(v, []):
            d = s.layers[j]
            K, C = d["Ko"], 1 if (gauss or d["kind"] == capi.CK_SAMPLE_GAUSSIAN) else d["M"]
            row = (int(s.fold_off[j]) + f, K, C, tab_off[j] + f * K * C)
            ent.append(row if lz_off is None else row + (lz_off[j] + f * K,))
        start.append(len(ent))
    e = np.array(ent, dtype=np.int64).reshape(-1, 4 if lz_off is None else 5)
    q = {"entries": torch.from_numpy(e).to(s.device), "start": torch.from_numpy(np.array(start, dtype=np.int32)).to(s.device),
         "Q": len(ids), "C": 2 if gauss else int(e[:, 2].max()) if len(ent) else 1}
    return q, e, start


class QuerySets:
    """The tables of the last few query sets of a circuit (the tables are small but not free): `build(ids, gauss)` once each."""

    def __init__(self, build, keep: int = 8) -> None:
        self._build, self._keep, self._sets = build, keep, {}

    def get(self, ids: list[int], gauss: bool) -> dict:
        key = tuple(ids)
        q = self._sets.get(key)
        if q is None:
            q = self._build(ids, gauss)
            if len(self._sets) >= self._keep:
                self._sets.pop(next(iter(self._sets)))
            self._sets[key] = q
        return q


def discrete_tables(s: Sampler):
    """Per Categorical / Binomial layer of the `prepare()`d sampler, in layer order: ``(layer index, t, shift, tot)`` with
    ``t`` (F, K, C) the table in linear space, shifted by ``shift`` (the row maximum where the table was logarithmic, else 0)
    and ``tot`` its sum over the states: ``t / tot`` is the normalised row, ``log tot + shift`` the log normaliser."""
    zero = torch.zeros((), device=s.device)
    for j, d in enumerate(s.layers):
        if "scope" not in d or d["kind"] == capi.CK_SAMPLE_GAUSSIAN:
            continue
        if d["spec"].type == "binomial":  # prepare()'s (F, T + 2, K) log-pmf table, last row the integral
            t, is_log = d["tab"][:, : d["M"], :].permute(0, 2, 1), True
        else:  # prepare()'s (F, K, C) probabilities or logits
            t, is_log = d["tab"], bool(d["is_logits"])
        shift = zero
        if is_log:
            mx = t.amax(dim=2, keepdim=True)
            shift = torch.where(torch.isfinite(mx), mx, zero)
            t = torch.exp(t - shift)
        yield j, t, shift, t.sum(dim=2, keepdim=True)


def run_chunks(ps, down: TopDownPass, x: torch.Tensor, vars_, rows_per_chunk: int | None, tables, start):
    """The driver of every query on a pass: the masked evidence batch (the variables `vars_` marks missing), its chunks, the
    per-parameter-state `tables()`, and per chunk the evidence forward of `ps` (a `PosteriorState`), the pass `down` and the
    caller's tail.  `start(B)` allocates the outputs and returns ``(result, tail)``; ``tail(r0, xc, bd, arena, bad, stream)``
    gets the chunk's first row, evidence, binding and pass arena, and the (B,) bad-row marks from row r0 on.  Returns
    `result`.  Refusals come first: nothing is copied, prepared or launched before them."""
    s = ps.s
    if rows_per_chunk is not None and int(rows_per_chunk) <= 0:
        raise ValueError("rows_per_chunk must be positive")
    xm = s.evidence_batch(x, vars_)
    B = int(xm.shape[0])
    chunks = down.chunks_of(B, rows_per_chunk)
    tables()
    dev = s.device
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        result, tail = start(B)
        bad = torch.zeros(B, dtype=torch.int32, device=dev)
        for r0, nb in chunks:
            xc = xm[r0 : r0 + nb]
            bd = ps.evidence_forward(xc, bad[r0:], stream)
            tail(r0, xc, bd, down.run(bd, stream), bad[r0:], stream)
    return result
