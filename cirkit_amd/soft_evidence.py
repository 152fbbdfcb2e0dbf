"""Soft (likelihood) evidence on the GPU: `HipCircuit.soft_evidence_log_prob` and `HipCircuit.soft_posterior_marginals`
("Soft evidence").

Every soft variable of a row carries a non-negative weight per state, ``log_lik[n, s, c] = log lambda`` (Pearl's virtual
evidence); the query is ``Z(lambda)[n] = sum_x c(x) prod_v lambda[n, v, x_v]``, the other variables observed or summed out.
A smooth, decomposable circuit computes it exactly in one bottom-up pass: an input unit over a soft variable emits
``log sum_c lambda(c) t_k(c)`` and the inner layers do not change.  Point evidence, missing values, intervals and arbitrary
per-variable sets are the 0/1 special cases.  The posteriors ``p(X_v = c | lambda, x) = d log Z / d log_lik[n, s, c]`` come from
one top-down flow pass (`topdown.TopDownPass`, the pass of `posterior_marginals`) over the same values.

The pass runs on the layer-wise circuit the other queries use (`Sampler._z_circuit()`).  Per chunk of rows: the hard
evidence, range-checked and with the soft variables marked missing, is staged and the input layers launched as the forward
launches them; the soft leaf overwrites the arena blocks of the folds over a soft variable; every other layer is launched
once (`_enqueue_layers(inputs=False)`).  The reference has no such query.  Kernels: cirkit_amd/csrc/ck_soft.hip.
"""

from __future__ import annotations

from typing import TYPE_CHECKING

import numpy as np
import torch

from . import _capi as capi
from .layers import HipBinomialLayer, HipCategoricalLayer, HipConstantValueLayer, HipInputLayer
from .plan import Plan
from .posterior import query_ids
from .sampling import _REFUSED, Sampler, chunk_rows, sampler
from .topdown import FLOW, QuerySets, TopDownPass, variable_kinds

if TYPE_CHECKING:  # pragma: no cover
    from .circuit import HipCircuit


def check_plan(plan: Plan) -> None:
    """Refuse, before anything is launched, what has no soft evidence: a plan that is not a real lse-sum circuit
    (``ValueError``, checked first), a layer without an integral over weighted states (``TypeError`` naming it)."""
    if plan.semiring != "lse-sum":
        raise ValueError(f"soft evidence needs a real circuit in the lse-sum semiring, this plan is {plan.semiring!r}")
    for i, l in enumerate(plan.layers):
        if l.type in _REFUSED:
            raise TypeError(f"Soft evidence is not supported for layers of type {_REFUSED[l.type]} (layer {i})")


def soft_ids(plan: Plan, soft_vars) -> list[int]:
    """The soft variables in ascending order (None: every variable a Categorical / Binomial layer reads), checked: a
    variable a Gaussian layer reads is a ``NotImplementedError``, one outside every input layer's scope a ``ValueError``."""
    kinds = variable_kinds(plan)
    if soft_vars is None:
        ids = sorted(v for v, k in kinds.items() if "discrete" in k)
    else:
        ids = query_ids(soft_vars, int(plan.num_variables))
    if not ids:
        raise ValueError("soft evidence needs at least one soft variable")
    missing = [v for v in ids if v not in kinds]
    if missing:
        raise ValueError(f"soft variables {missing[:8]} are outside the scope of every input layer")
    gauss = [v for v in ids if "gaussian" in kinds[v]]
    if gauss:
        raise NotImplementedError(f"soft evidence on variables {gauss[:8]} read by a Gaussian layer: pass them as hard "
                                  "evidence through x")
    return ids


def num_states(plan: Plan, ids: list[int]) -> int:
    """The largest state count among the discrete input layers over the variables `ids`."""
    soft, C = set(ids), 0
    for l in plan.layers:
        if l.inputs is None and l.type in ("categorical", "binomial") and soft & {int(v) for v in l.scope_idx[:, 0]}:
            C = max(C, int(l.config["num_categories"]) if l.type == "categorical" else int(l.config["total_count"]) + 1)
    return C


def check_arguments(plan: Plan, log_lik, x, ids: list[int]) -> None:
    D = int(plan.num_variables)
    if not isinstance(log_lik, torch.Tensor) or log_lik.dim() != 3 or not log_lik.is_floating_point():
        raise ValueError("log_lik should be a floating-point tensor of shape (B, S, C): rows, soft variables, states")
    B, S, C = (int(n) for n in log_lik.shape)
    if B <= 0:
        raise ValueError("empty batch")
    if S != len(ids):
        raise ValueError(f"log_lik has {S} soft variables, soft_vars names {len(ids)}")
    if C < num_states(plan, ids):
        raise ValueError(f"log_lik has {C} states, the soft variables have up to {num_states(plan, ids)}")
    if x is not None:
        if not isinstance(x, torch.Tensor) or x.dim() != 2:
            raise ValueError("The input to the circuit should have shape (B, D), where B is the batch size and D "
                             "is the number of variables the circuit is defined on")
        if x.shape[1] < D:
            raise ValueError(f"expected at least {D} variables, found {x.shape[1]}")
        if int(x.shape[0]) != B:
            raise ValueError(f"log_lik has {B} rows and x {int(x.shape[0])}")


class SoftEvidenceState:
    """The soft-evidence state of one `HipCircuit`, next to its `Sampler`: the linear side tables of the last parameter
    state, the tables of the last few soft-variable sets and the flow pass."""

    def __init__(self, s: Sampler) -> None:
        self.s = s
        self._key = None
        self._side: dict[int, tuple] = {}  # discrete input layer -> (lin (F, C, K), linT view, mt view)
        self._linT: torch.Tensor | None = None  # the layers' (F, K, C) blocks, flat
        self._mt: torch.Tensor | None = None  # the layers' (F, K) maxima, flat
        self._off: dict[int, tuple[int, int]] = {}  # discrete input layer -> element offsets of its blocks in the two
        self._sets = QuerySets(self._build_set)
        self.down = TopDownPass(s, FLOW)

    # -- once per parameter state ----------------------------------------------------------------------------------------
    def tables(self, stream: int, flows: bool) -> None:
        """The layer-wise circuit's derived parameters and the side tables of every discrete input layer, for the store's
        current values (`flows`: and the sum weights the flow pass reads, `Sampler.prepare`); a no-op when nothing changed
        since the last call."""
        st, s = self.s.store, self.s
        if flows:
            s.prepare()
        key = (st.version, st.state(), st.raw_writes)
        if key == self._key:
            return
        zc = s._z_circuit()
        zc._enqueue_params(stream)
        cats = [(j, l) for j, l in enumerate(zc.layers) if isinstance(l, HipCategoricalLayer)]
        if self._linT is None:
            n_lin = n_mt = 0
            for j, l in cats:
                self._off[j] = (n_lin, n_mt)
                n_lin += l.num_folds * l.num_output_units * l.num_categories
                n_mt += l.num_folds * l.num_output_units
            self._linT = torch.empty(max(1, n_lin), dtype=torch.float32, device=s.device)
            self._mt = torch.empty(max(1, n_mt), dtype=torch.float32, device=s.device)
            for j, l in cats:
                F, K, C = l.num_folds, l.num_output_units, l.num_categories
                lo, mo = self._off[j]
                self._side[j] = (torch.empty((F, C, K), dtype=torch.float32, device=s.device),
                                 self._linT[lo : lo + F * K * C], self._mt[mo : mo + F * K])
        for j, l in cats:
            lin, linT, mt = self._side[j]
            capi.call("ck_soft_tables", l._table.data_ptr(), lin.data_ptr(), linT.data_ptr(), mt.data_ptr(), l.num_folds,
                      l.num_categories, l.num_output_units, stream)
        self._sets = QuerySets(self._build_set)  # (the entries hold the tables' addresses)
        self._key = key

    # -- once per soft-variable set ----------------------------------------------------------------------------------
    def _build_set(self, ids: list[int], _unused) -> dict:
        """Per discrete input layer with a soft fold ``spos`` (F,) int32, the position of each fold's variable among the soft
        variables (-1: hard); the posterior leaf's entries (six int64 per input fold over a soft variable) and their CSR."""
        s, zc = self.s, self.s._z_circuit()
        pos = {v: i for i, v in enumerate(ids)}
        spos: dict[int, torch.Tensor] = {}
        per_var: list[list[tuple]] = [[] for _ in ids]
        for j, l in enumerate(zc.layers):
            if not isinstance(l, HipCategoricalLayer):
                continue
            F, K, C = l.num_folds, l.num_output_units, l.num_categories
            sp = np.array([pos.get(int(v), -1) for v in np.asarray(l.scope_idx[:, 0])], dtype=np.int32)
            if (sp < 0).all():
                continue
            spos[j] = torch.from_numpy(sp).to(s.device)
            lo, mo = self._off[j]
            for f in np.nonzero(sp >= 0)[0]:
                per_var[sp[f]].append((int(s.fold_off[j]) + int(f), K, C, l._table.data_ptr() + int(f) * (C + 1) * K * 4,
                                       lo + int(f) * K * C, mo + int(f) * K))
        ent = np.array([e for es in per_var for e in es], dtype=np.int64).reshape(-1, 6)
        start = np.concatenate([[0], np.cumsum([len(es) for es in per_var])]).astype(np.int32)
        ks, cs = set(ent[:, 1].tolist()), set(ent[:, 2].tolist())
        uniform = len(ks) == 1 and len(cs) == 1 and next(iter(ks)) in (32, 64)
        return {"spos": spos, "entries": torch.from_numpy(ent).to(s.device), "start": torch.from_numpy(start).to(s.device),
                "K_uniform": next(iter(ks)) if uniform else 0, "C_uniform": next(iter(cs)) if uniform else 0,
                "entries_host": ent}

    # -- per chunk -------------------------------------------------------------------------------------------------------
    def hard_inputs(self, bd, xc: torch.Tensor, bad: torch.Tensor, stream: int) -> None:
        """The input layers of binding `bd` on a chunk of hard evidence (the soft variables marked missing), after its range
        check: an out-of-range observed category sets bad[n] and the flag `hc.check_inputs()` reports and is replaced by 0,
        so that the other rows keep their values (`PosteriorState.evidence_forward`'s rule)."""
        s = self.s
        hc, zc = s.hc, s._z_circuit()
        clean = torch.empty_like(xc)
        flag = hc._bad_input.data_ptr() if hc.validate_inputs else None
        capi.call("ck_flow_check_evidence", xc.data_ptr(), 1 if s.float_out else 0, hc._num_states_dev().data_ptr(), bd.B, s.D,
                  clean.data_ptr(), bad.data_ptr(), flag, stream)
        xf, xi = zc._prepare_input(clean)
        zc._stage_input(bd, xf, xi, stream)
        for i, role in enumerate(zc._roles):
            if role == "input":
                zc._launch_layer(i, bd, stream)
        zc._bad_input.zero_()  # (nothing can have set it; kept clean for `prepare()`'s forwards all the same)

    def soft_leaf(self, bd, q: dict, ll: torch.Tensor, bad: torch.Tensor, stream: int) -> int:
        """The soft leaf of every discrete input layer with a soft fold, into its arena view of binding `bd`; marks the rows
        with a NaN / +inf in a read entry in `bad`; returns the number of launches."""
        zc = self.s._z_circuit()
        S, Cl = int(ll.shape[1]), int(ll.shape[2])
        for j, sp in q["spos"].items():
            l = zc.layers[j]
            lin, _, mt = self._side[j]
            # (a Binomial log-pmf table spans hundreds of nats: most of its entries would take the matrix-core kernel's
            #  exact fix-up anyway -- DESIGN.md section 11, "Soft evidence")
            exact = 1 if isinstance(l, HipBinomialLayer) else 0
            capi.call("ck_soft_leaf_fwd", l._table.data_ptr(), lin.data_ptr(), mt.data_ptr(), ll.data_ptr(), sp.data_ptr(),
                      bd.views[j].data_ptr(), bad.data_ptr(), l.num_folds, bd.B, l.num_output_units, l.num_categories, S, Cl,
                      exact, stream)
        return len(q["spos"])

    def evidence_forward(self, nb: int, q: dict, xc: torch.Tensor, ll: torch.Tensor, bad: torch.Tensor, stream: int):
        """One chunk's bottom-up pass: hard inputs, soft leaf, every inner layer once; returns the binding."""
        zc = self.s._z_circuit()
        bd = zc._bind(nb)
        self.hard_inputs(bd, xc, bad, stream)
        self.soft_leaf(bd, q, ll, bad, stream)
        zc._enqueue_layers(bd, stream, inputs=False)
        return bd

    def posterior_leaf(self, bd, flow: torch.Tensor, q: dict, ll: torch.Tensor, bad: torch.Tensor, out: torch.Tensor,
                       logev: torch.Tensor | None, stream: int) -> None:
        s = self.s
        capi.call("ck_soft_posterior", q["entries"].data_ptr(), q["start"].data_ptr(), int(ll.shape[1]), int(ll.shape[2]),
                  q["K_uniform"], q["C_uniform"], ll.data_ptr(), self._linT.data_ptr(), self._mt.data_ptr(), flow.data_ptr(),
                  bd.arena.data_ptr(), s._val_off_table(bd).data_ptr(), s.root_fold, s.layers[s.root_layer]["Ko"],
                  bad.data_ptr(), bd.B, out.data_ptr(), None if logev is None else logev.data_ptr(), stream)

    # -- once per call ---------------------------------------------------------------------------------------------------
    def _evidence(self, log_lik: torch.Tensor, x: torch.Tensor | None, ids: list[int]) -> tuple[torch.Tensor, torch.Tensor]:
        """The (B, D) hard evidence with the soft variables marked missing (`x` None: every variable) and the (B, S, C)
        fp32 log-likelihoods, both on the device."""
        s = self.s
        B = int(log_lik.shape[0])
        if x is None:
            sentinel = float("nan") if s.float_out else -1
            xm = torch.full((B, s.D), sentinel, dtype=s.dtype, device=s.device)
        else:
            xm = s.evidence_batch(x, ids)
        return xm, log_lik.to(s.device).to(torch.float32).contiguous()

    def _release(self, sizes: set[int]) -> None:
        zc = self.s._z_circuit()
        for b in [b for b in zc._bindings if b != 1 and b not in sizes]:  # two batch sizes bound: the chunk and the tail
            zc._bindings.pop(b).destroy()
            self.s._val_off.pop(b, None)

    def soft_evidence_log_prob(self, log_lik, x, ids: list[int], rows_per_chunk: int | None):
        s = self.s
        hc = s.hc
        xm, ll = self._evidence(log_lik, x, ids)
        B = int(ll.shape[0])
        chunks = chunk_rows(B, rows_per_chunk, hc.arena_bytes(1))
        zc = s._z_circuit()
        self._release({nb for _, nb in chunks})
        pairs = zc._out_pairs
        K = zc.layers[int(pairs[0, 0])].num_output_units
        if hc._pad_info is not None:
            K = min(K, hc._pad_info.out_units)
        dev = s.device
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            out = torch.empty((B, len(pairs), K), dtype=torch.float32, device=dev)
            bad = torch.zeros(B, dtype=torch.int32, device=dev)
            self.tables(stream, flows=False)
            q = self._sets.get(ids, False)
            for r0, nb in chunks:
                bd = self.evidence_forward(nb, q, xm[r0 : r0 + nb], ll[r0 : r0 + nb], bad[r0:], stream)
                for o, (p, f) in enumerate(pairs):
                    out[r0 : r0 + nb, o].copy_(bd.views[int(p)][int(f)][:, :K])
            out.masked_fill_((bad != 0)[:, None, None], float("nan"))
        return out

    def soft_posterior_marginals(self, log_lik, x, ids: list[int], return_log_evidence: bool, rows_per_chunk: int | None):
        s = self.s
        xm, ll = self._evidence(log_lik, x, ids)
        B = int(ll.shape[0])
        chunks = self.down.chunks_of(B, rows_per_chunk)
        zc = s._z_circuit()
        dev = s.device
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            self.tables(stream, flows=True)
            q = self._sets.get(ids, False)
            out = torch.empty(tuple(ll.shape), dtype=torch.float32, device=dev)
            logev = torch.empty(B, dtype=torch.float32, device=dev)
            bad = torch.zeros(B, dtype=torch.int32, device=dev)
            for r0, nb in chunks:
                lc = ll[r0 : r0 + nb]
                bd = self.evidence_forward(nb, q, xm[r0 : r0 + nb], lc, bad[r0:], stream)
                flow = self.down.run(bd, stream)
                self.posterior_leaf(bd, flow, q, lc, bad[r0:], out[r0], logev[r0:], stream)
        return (out, logev) if return_log_evidence else out


def check_call(hc: "HipCircuit", log_lik, x, soft_vars) -> list[int]:
    """Every refusal and argument error of a soft-evidence query, in order; returns the soft variable ids."""
    check_plan(hc.user_plan)
    ids = soft_ids(hc.user_plan, soft_vars)
    check_arguments(hc.user_plan, log_lik, x, ids)
    for l in hc.layers:
        if isinstance(l, HipInputLayer) and not isinstance(l, HipConstantValueLayer) and not l.can_integrate:
            raise NotImplementedError(f"soft evidence through {type(l).__name__}: it cannot integrate")
    return ids


def _state(hc: "HipCircuit", log_lik, x, soft_vars) -> tuple[SoftEvidenceState, list[int]]:
    """Every refusal and argument error, then the circuit's state: nothing is allocated or launched before them."""
    ids = check_call(hc, log_lik, x, soft_vars)
    s = sampler(hc)
    if s._soft is None:
        s._soft = SoftEvidenceState(s)
    return s._soft, ids


def _rows(rows_per_chunk) -> int | None:
    if rows_per_chunk is not None and int(rows_per_chunk) <= 0:
        raise ValueError("rows_per_chunk must be positive")
    return rows_per_chunk


def soft_evidence_log_prob(hc: "HipCircuit", log_lik: torch.Tensor, x: torch.Tensor | None = None, *, soft_vars=None,
                           rows_per_chunk: int | None = None):
    """`HipCircuit.soft_evidence_log_prob`: see its docstring."""
    rows_per_chunk = _rows(rows_per_chunk)
    st, ids = _state(hc, log_lik, x, soft_vars)
    return st.soft_evidence_log_prob(log_lik, x, ids, rows_per_chunk)


def soft_posterior_marginals(hc: "HipCircuit", log_lik: torch.Tensor, x: torch.Tensor | None = None, *, soft_vars=None,
                             return_log_evidence: bool = False, rows_per_chunk: int | None = None):
    """`HipCircuit.soft_posterior_marginals`: see its docstring."""
    rows_per_chunk = _rows(rows_per_chunk)
    st, ids = _state(hc, log_lik, x, soft_vars)
    return st.soft_posterior_marginals(log_lik, x, ids, return_log_evidence, rows_per_chunk)
