"""Hidden Markov models on the GPU: the forward algorithm of a chain plan in ONE launch ("Hidden Markov
models").

`templates.hmm` -- the reference's ``cirkit.templates.pgms.hmm`` compiled with ``fold=True, optimize=True`` -- is one input
layer with a fold per position, a dense sum and T - 1 CP-T layers of ONE fold each: T dependent layers.  `HipCircuit` evaluates
them with one launch per layer, each writing a (B, K) block that the next one reads back; `HipHMM.log_prob` recognises the chain
(`chain_of`) and hands it to `ck_hmm_forward` (cirkit_amd/csrc/ck_hmm.hip), where a workgroup keeps the state of its 32 rows on
chip from the first position to the last.

A Categorical input layer is read as its (F, C + 1, K) table of logarithms, gathered by the kernel itself: one launch per call.
Any other input layer (Binomial, Gaussian) is evaluated by its own launch into a (F, B, K) block first, `rows_per_chunk` rows at a
time.  Missing entries -- a variable in `integrate_vars`, or per entry ``x[b, v] == -1`` (NaN for Gaussian inputs): what padding
sequences of different lengths needs -- are summed out.

`HipHMM.log_prob(segments=P)` is the same value for SMALL batches, parallel in time: the one launch costs a single row what it
costs 4096, so the steps are cut into `P` segments, `ck_hmm_scan_segments` evaluates the ``K x K`` log transfer matrix of every
segment of every row at once (virtual rows started from one-hot vectors) and `ck_hmm_scan_combine` chains them in the log domain
(cirkit_amd/csrc/ck_hmm_scan.hip) -- two launches per chunk of rows, Categorical inputs, up to 512 units; ``segments="auto"`` takes
it where it measured faster (`HipHMM.auto_segments`).

`HipHMM.state_posteriors` is forward-backward smoothing, ``p(z_v = k | evidence)`` for every position: the forward launch
instantiated to leave its hand-off in the ``(B, D, K)`` result, and `ck_hmm_backward`, which walks the chain back with the weights
transposed and turns that buffer into posteriors in place -- two launches where `log_prob` takes one.

`HipHMM.viterbi` is the most probable state sequence, ``argmax_z p(z, evidence)``, and its log-probability: a max-product forward
pass on the vector ALU that keeps the same hand-off (`ck_hmm_viterbi_forward`) and a walk back over it, one wave a row
(`ck_hmm_viterbi_backtrack`; cirkit_amd/csrc/ck_hmm_viterbi.hip) -- two launches again.

`HipHMM.expected_statistics` is the Baum-Welch E-step, the `ExpectedStatistics` of `HipCircuit.expected_statistics` for a chain
with a Categorical input layer: the keeping forward, a variant of the backward pass that also leaves the two operand rows of every
pairwise posterior (`ck_hmm_backward_stats`), their product reduced over the rows of the batch on the matrix pipe
(`ck_hmm_pair_sum`) and the emission histogram (`ck_hmm_leaf_sum`; both cirkit_amd/csrc/ck_hmm_stats.hip) -- four launches per chunk
of rows where the layer-wise path takes several per layer.  `HipEMTrainer.apply` turns the result into an M-step.

`HipHMM.sample_posterior` draws state paths from ``p(z | evidence)`` and completes the missing entries of each row from the
emissions of the drawn states -- forward-filter-backward-sample: the keeping forward and a walk back that draws where Viterbi's
takes a maximum, a (row, sample) pair to a group of lanes sized to K (`ck_hmm_sample_paths`; cirkit_amd/csrc/ck_hmm_sample.hip) --
two launches per chunk of rows whatever T, B, K and the number of samples.  `HipHMM.sample` is the same walk on one row without
evidence.

`HipHMM.autoregressive_log_probs`, `autoregressive_conditionals` and `coding_tables` are the chain-rule decomposition
``p(x_{o_j} = c | x_{o_0 .. o_{j-1}})`` along `generative_order`: the chain generates from its last step down, so the backward
recursion is the predictive filter of that order and ONE walk down the chain (`ck_hmm_predict`;
cirkit_amd/csrc/ck_hmm_predict.hip) gives every position -- one launch, ``O(T)`` steps a row where the owned `HipCircuit` expands
every row into ``T`` rows of ``T`` layers each.  The conditionals contract the predictive state with a cached linear emission
table on the matrix pipe (`ck_hmm_emission_table`, once per parameter state); the coding tables pass them through the
quantiser `HipCircuit.coding_tables` uses.

`HipHMM.soft_evidence_log_prob`, `soft_state_posteriors`, `soft_posterior_marginals` and `soft_viterbi` take soft (likelihood)
evidence, a ``(B, S, C)`` block of log weights per soft variable, with `HipCircuit`'s argument conventions: a soft emission is the
contraction ``log sum_c lambda_c p(c | k)``, so `ck_hmm_soft_rows` writes the ``(F, rows, K)`` block of log emissions of a chunk
on the matrix pipe (cirkit_amd/csrc/ck_hmm_soft.hip) and the chain kernels above take it as their row source unchanged;
`ck_hmm_soft_flag` makes the rows with a NaN or ``+inf`` weight NaN and `ck_hmm_soft_leaf` contracts ``gamma / y`` with the same
emission table into the posteriors of the soft variables -- 3, 4, 5 and 4 launches per chunk.

Out of scope: an M-step of `HipHMM`'s own; expected statistics, sampling and autoregressive conditionals of inputs other than
Categorical; soft evidence in `expected_statistics`, `sample_posterior`, the time-parallel forward and the autoregressive queries,
on Binomial or Gaussian chains, fused into the chain kernels' step, or with a set of soft variables per row; autoregressive conditionals of a subset of positions, along any order but the generative one, or parallel in
time; a decoder-side table provider for cirkit_amd/codec.py; k-best
paths; homogeneous chains (the kernel's table of weight pointers already allows shared transitions; their statistics would be
summed over the steps); bf16-piece variants; training beyond what `HipTrainer` and `HipEMTrainer` do with a chain plan layer by
layer; routing `HipCircuit.forward` or `HipCircuit.mpe` to these kernels.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Mapping

import numpy as np
import torch

from . import _capi as capi
from .expected import ExpectedStatistics
from .plan import Plan, resolve_fold_index

_INPUTS = ("categorical", "binomial", "gaussian")
_CHUNK_BYTES = 1 << 30  # the (F, rows, K) block of emissions of one chunk (inputs other than Categorical)


@dataclass
class ChainStep:
    """One position of the chain: the layer whose ``weight`` is its transition, the input fold it multiplies in and that fold's
    variable."""

    layer: int
    fold: int
    var: int


def chain_of(plan: Plan) -> list[ChainStep]:
    """The steps of a chain plan in plan order, or ``NotImplementedError`` naming the layer that breaks the pattern: one input
    layer with one variable per fold; a dense sum over one of its folds; then per step a CP-T layer of arity 2 -- or the Hadamard
    layer and the dense sum it was fused from -- over the previous step and one more input fold; one fold per layer, no input
    fold read twice, the last step the output.  Needs no device."""
    if plan.semiring != "lse-sum":
        raise NotImplementedError(f"HipHMM: semiring {plan.semiring!r} (chains are evaluated under lse-sum)")
    inputs = [i for i, l in enumerate(plan.layers) if l.inputs is None]
    if len(inputs) != 1:
        raise NotImplementedError(f"HipHMM: {len(inputs)} input layers (layers {inputs[:4]}); a chain has one, a fold per position")
    (inp,) = inputs
    src = plan.layers[inp]
    if src.type not in _INPUTS or src.scope_idx is None or src.scope_idx.shape[1] != 1:
        raise NotImplementedError(f"HipHMM: layer {inp} is not a {' / '.join(_INPUTS)} input layer of one variable per fold")
    K = src.num_output_units
    folds = [l.num_folds for l in plan.layers]
    steps: list[ChainStep] = []
    prev, product, seen = None, None, set()

    def refuse(i: int, why: str):
        raise NotImplementedError(f"HipHMM: layer {i} ({plan.layers[i].type}) breaks the chain: {why}")

    def take(i: int, f: int) -> None:
        if f in seen:
            refuse(i, f"input fold {f} is read twice")
        seen.add(f)

    for i, l in enumerate(plan.layers):
        if i == inp:
            continue
        if l.num_folds != 1:
            refuse(i, f"{l.num_folds} folds")
        ch = [(int(p), int(f)) for p, f in resolve_fold_index(l.inputs, folds)[0]]
        if l.type in ("sum", "cpt") and l.num_input_units != K:
            refuse(i, f"{l.num_input_units} input units, the input layer has {K}")
        if l.type == "sum" and l.arity != 1:
            refuse(i, f"a sum of arity {l.arity} (a mixing layer)")
        if l.type in ("cpt", "hadamard") and l.arity != 2:
            refuse(i, f"arity {l.arity}")
        if l.type == "sum" and prev is None and product is None:  # the first position
            if ch[0][0] != inp:
                refuse(i, "the first sum does not read the input layer")
            take(i, ch[0][1])
            steps.append(ChainStep(i, ch[0][1], int(src.scope_idx[ch[0][1], 0])))
        elif l.type == "sum" and product is not None and ch == [(product[0], 0)]:
            steps.append(ChainStep(i, product[1], int(src.scope_idx[product[1], 0])))
            product = None
        elif l.type in ("cpt", "hadamard") and prev is not None and product is None:
            leaf = [f for p, f in ch if p == inp]
            if len(leaf) != 1 or sorted(ch, key=lambda c: c[0] == inp)[0] != (prev, 0):
                refuse(i, "it does not multiply the previous step with one input fold")
            take(i, leaf[0])
            if l.type == "hadamard":
                product, prev = (i, leaf[0]), None
                continue
            steps.append(ChainStep(i, leaf[0], int(src.scope_idx[leaf[0], 0])))
        else:
            refuse(i, "not a dense sum, a CP-T layer or a Hadamard layer in chain position")
        if l.num_output_units != K and i != len(plan.layers) - 1:
            refuse(i, f"{l.num_output_units} output units inside the chain")
        prev = i
    out = [(int(p), int(f)) for p, f in resolve_fold_index(plan.output, folds).reshape(-1, 2)]
    if not steps or product is not None or out != [(steps[-1].layer, 0)]:
        raise NotImplementedError("HipHMM: the output of the plan is not the last step of a chain")
    return steps


class HipHMM:
    """``log p(x)`` of a chain plan (`templates.hmm`, or the same layers compiled by the reference) with the whole chain in one
    launch.  It owns a layer-wise `HipCircuit` of the plan for the parameter store, the evaluated parameter graphs and the input
    layer (unit counts padded to 32 where `HipCircuit` pads them); the prepared tables follow the store's state.  Refused
    (``NotImplementedError``, before anything is allocated): whatever `chain_of` refuses, complex parameter tensors, more than
    1024 units."""

    def __init__(self, plan: Plan, tensors: Mapping[str, object], *, device: str | torch.device = "cuda:0") -> None:
        from .circuit import HipCircuit

        chain_of(plan)
        self.num_states = next(l for l in plan.layers if l.inputs is None).num_output_units  # (before any padding)
        for n in plan.tensors:
            v = tensors[n]
            if np.iscomplexobj(v) or (hasattr(v, "is_complex") and v.is_complex()):
                raise NotImplementedError("HipHMM: complex parameter tensors")
        if max(l.num_output_units for l in plan.layers) > 1024:
            raise NotImplementedError("HipHMM: more than 1024 latent states")
        self.device = torch.device(device)
        # (row-major weights: the chain kernel lays a step's rows out itself while it stages them)
        self.hc = HipCircuit(plan, tensors, device=self.device, fuse=False, tiled_weights=False)
        self.store = self.hc.store
        self.plan = self.hc.plan  # (padded where HipCircuit pads)
        self.steps = chain_of(self.plan)
        self.input_layer = next(i for i, l in enumerate(self.plan.layers) if l.inputs is None)
        self.K = self.plan.layers[self.input_layer].num_output_units
        self.categorical = self.plan.layers[self.input_layer].type == "categorical"
        self.last_launches = 0  # launches of the last call of a query
        self._key = None
        self._tab: dict | None = None

    @property
    def num_variables(self) -> int:
        return self.plan.num_variables

    def tables(self) -> dict:
        """The parameter graphs evaluated for the current state of the store, and the device tables of the steps."""
        key = (self.store.version, self.store.state())
        if self._tab is not None and self._key == key:
            return self._tab
        hc = self.hc
        with torch.cuda.device(self.device):
            hc._enqueue_params(torch.cuda.current_stream(self.device).cuda_stream)
        ws = [hc.layers[s.layer]._w for s in self.steps]
        for s, w in zip(self.steps, ws):
            l = self.plan.layers[s.layer]
            if w is None or w.dtype != torch.float32 or not w.is_contiguous() or tuple(w.shape) != (1, l.num_output_units, self.K):
                raise NotImplementedError(f"HipHMM: the weight of layer {s.layer} is not a real (1, Ko, K) block")
        tab = {
            "w": torch.tensor([w.data_ptr() for w in ws], dtype=torch.int64).to(self.device),
            "keep": ws,
            "fold": torch.tensor([s.fold for s in self.steps], dtype=torch.int32).to(self.device),
            "var": torch.tensor([s.var for s in self.steps], dtype=torch.int32).to(self.device),
        }
        if self.categorical:
            t = hc.layers[self.input_layer]._table  # (F, C + 1, K) logarithms, a (fold, category) row contiguous
            if t is None or t.dtype != torch.float32 or not t.is_contiguous():
                raise NotImplementedError("HipHMM: the Categorical layer has no real table of logarithms")
            tab["rows"] = t
        self._tab, self._key = tab, key
        return tab

    def _mask(self, integrate_vars) -> torch.Tensor | None:
        if integrate_vars is None:
            return None
        from .squared import _mask_of

        m = _mask_of(integrate_vars, self.plan.num_variables)
        return torch.from_numpy(m.astype(np.int32)).to(self.device) if m.any() else None

    def rows_per_chunk(self) -> int:
        """Rows of a chunk by default for inputs other than Categorical: the block of emissions at or below 1 GiB."""
        return max(1, _CHUNK_BYTES // (len(self.steps) * self.K * 4))

    def log_prob(self, x: torch.Tensor, integrate_vars=None, *, rows_per_chunk: int | None = None,
                 segments: int | str | None = None) -> torch.Tensor:
        """``(B,)`` fp32: ``log p(x)`` with the variables of `integrate_vars` (ids, or a ``(D,)`` bool mask), and every entry
        ``x[b, v] == -1`` (NaN for Gaussian inputs), summed out.  `x`: ``(B, T)``, int64 for discrete inputs, fp32 for Gaussian
        ones.  A category outside its layer's range makes the row NaN (inputs other than Categorical: the batch, with
        `HipCircuit.check_inputs` of the owned circuit raising).  A row's value does not depend on `rows_per_chunk`.

        `segments` = ``P``, an int with ``2 <= P <= T``, takes the time-parallel path for small batches (DESIGN.md section 11,
        "Time-parallel forward"): the steps are cut at ``floor(p T / P)``, `ck_hmm_scan_segments` evaluates the ``K x K`` log
        transfer matrix of every segment of every row at the same time and `ck_hmm_scan_combine` chains them -- two launches per
        chunk of `rows_per_chunk` rows whatever ``T``, ``K``, ``B`` and ``P``, ``K`` times the arithmetic of the sequential walk
        on a dependent chain of about ``T / P + P`` steps instead of ``T``.  Same semantics (missing entries summed out, a row
        without mass -inf and never NaN, a category >= C NaN); a row's value depends on ``P`` to rounding only, not on
        `rows_per_chunk` or on the other rows, and the same ``(x, P)`` gives the same bits.  By default a chunk keeps the
        scratch -- per row ``(P - 2)`` matrices of ``num_states`` rounded up to 32 by ``K`` floats, two vectors and ``P`` flag
        words -- at or below 1 GiB.  Any other int, or ``T = 1``, raises ``ValueError``; an input layer other than Categorical, or
        more than 512 units after padding (the path multiplies the arithmetic by ``K``), raises ``NotImplementedError`` before
        anything is allocated.  ``segments="auto"`` takes what `auto_segments` picks for the batch."""
        if segments is None:
            return self._chain(x, integrate_vars, rows_per_chunk, "log_prob")[0]
        return self._scan(x, integrate_vars, rows_per_chunk, segments)

    _SCAN_MAX_UNITS = 512

    def auto_segments(self, B: int) -> int | None:
        """What ``log_prob(segments="auto")`` takes for a batch of `B` rows: ``None`` (the sequential walk) or a number of
        segments.  Fitted to the table of DESIGN.md section 11, "Time-parallel forward": ``None`` wherever the sequential walk
        measured faster than the scan or within 10 % of it, and wherever the scan does not apply."""
        T, K = len(self.steps), self.K
        if not self.categorical or K > self._SCAN_MAX_UNITS or T < 64:  # (chains shorter than 64 steps: not measured)
            return None
        # workgroups of launch 1 that the device holds at once: LDS of one (activation tile, row maxima, weight rings) in the
        # 160 KiB of a CU.  The scan measured faster than the sequential walk by more than 10 % wherever the (row, tile of start
        # states) pairs of ONE segment fill at most half of them, and level with it or slower where they fill all.
        lds = 4 * (32 * K + 128 + min(K // 32, 4) * 8 * 512)
        held = torch.cuda.get_device_properties(self.device).multi_processor_count * max(1, (160 << 10) // lds)
        pairs = B * -(-self.num_states // 32)
        if 2 * pairs > held:
            return None
        # sqrt(T) segments balance the two chains where a boundary of launch 2 costs about a step (K = 32) and all segments run at
        # once; half as many where a boundary costs more than a step (K >= 256) or the segments queue for the device
        full = max(2, round(T ** 0.5))
        return full if K < 256 and pairs * (full - 1) <= held else max(2, round(T ** 0.5 / 2))

    def _scan(self, x: torch.Tensor, integrate_vars, rows_per_chunk: int | None, segments) -> torch.Tensor:
        """`log_prob` by the time-parallel path: per chunk of rows `ck_hmm_scan_segments` and `ck_hmm_scan_combine`."""
        D, T, K = self.plan.num_variables, len(self.steps), self.K
        auto = isinstance(segments, str) and segments == "auto"
        if auto and self.auto_segments(1) is None:  # (no batch is small enough, or the path does not apply)
            return self._chain(x, integrate_vars, rows_per_chunk, "log_prob")[0]
        self._need_categorical("log_prob(segments=)")
        if K > self._SCAN_MAX_UNITS:
            raise NotImplementedError(f"HipHMM.log_prob(segments=): {K} units after padding, the time-parallel path serves up to "
                                      f"{self._SCAN_MAX_UNITS}")
        if x.dim() != 2 or x.shape[1] != D:
            raise ValueError(f"expected x of shape (B, {D}), found {tuple(x.shape)}")
        if rows_per_chunk is not None and int(rows_per_chunk) <= 0:
            raise ValueError("rows_per_chunk must be positive")
        B = int(x.shape[0])
        if B <= 0:
            raise ValueError("empty batch")
        if auto:
            segments = self.auto_segments(B)
            if segments is None:
                return self._chain(x, integrate_vars, None, "log_prob")[0]
        if isinstance(segments, bool) or not isinstance(segments, (int, np.integer)) or not 2 <= int(segments) <= T:
            raise ValueError(f"segments must be None, 'auto' or an int in 2 .. T = {T}, found {segments!r}")
        P = int(segments)
        tab = self.tables()
        C = self.plan.layers[self.input_layer].config["num_categories"]
        ns32 = -(-self.num_states // 32) * 32
        per_row = 4 * ((P - 2) * ns32 * K + 2 * K + P)
        n = min(B, int(rows_per_chunk) if rows_per_chunk is not None else max(1, _CHUNK_BYTES // per_row))
        self.last_launches = 0
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            mask = self._mask(integrate_vars)
            mp = None if mask is None else mask.data_ptr()
            x = x.to(self.device).to(torch.int64).contiguous()
            out = torch.empty(B, dtype=torch.float32, device=self.device)
            lg = torch.empty((n, P - 2, ns32, K), dtype=torch.float32, device=self.device) if P > 2 else None
            first, last = (torch.empty((n, K), dtype=torch.float32, device=self.device) for _ in range(2))
            flags = torch.empty((n, P), dtype=torch.int32, device=self.device)
            scratch = (first.data_ptr(), None if lg is None else lg.data_ptr(), last.data_ptr(), flags.data_ptr())
            for r0 in range(0, B, n):
                nb = min(n, B - r0)
                capi.call("ck_hmm_scan_segments", tab["w"].data_ptr(), tab["fold"].data_ptr(), tab["var"].data_ptr(), T, K,
                          self.num_states, tab["rows"].data_ptr(), x[r0:].data_ptr(), D, C, mp, nb, P, *scratch, stream)
                capi.call("ck_hmm_scan_combine", T, K, self.num_states, nb, P, *scratch, out[r0:].data_ptr(), stream)
                self.last_launches += 2
        return out

    def state_posteriors(self, x: torch.Tensor, integrate_vars=None, *, rows_per_chunk: int | None = None,
                         return_log_prob: bool = False):
        """``(B, D, K)`` fp32 smoothing posteriors ``[b, v, k] = p(z_v = k | evidence of row b)``, indexed by variable id, `K` the
        number of latent states (a view of the buffer padded to 32 units; padded units carry 0); with `return_log_prob` also the
        ``(B,)`` log-likelihood of the same pass.  `x`, `integrate_vars` and `rows_per_chunk` as for `log_prob`.  Forward-backward
        in two launches (`ck_hmm_forward_keep`, `ck_hmm_backward`) where `log_prob` takes one: the forward leaves its hand-off in
        the result buffer and the backward pass turns it into posteriors in place, each (row, position) normalised by its own
        sum -- no ``(T, B, K)`` scratch besides the result.  A row without mass (``log p = -inf``) is NaN in every entry, and so is
        whatever `log_prob` makes NaN (a category outside its layer's range).  A row's values do not depend on
        `rows_per_chunk`."""
        out, post, _ = self._chain(x, integrate_vars, rows_per_chunk, "posteriors")
        post = post[:, :, :self.num_states]
        return (post, out) if return_log_prob else post

    def viterbi(self, x: torch.Tensor, integrate_vars=None, *, rows_per_chunk: int | None = None):
        """``(states, score)``: the most probable state sequence given the observed entries of each row, and its log-probability
        ``max_z log p(z, observed entries)`` -- ``(B,)`` fp32.  ``states`` is ``(B, D)`` int64 indexed by variable id:
        ``states[b, var_s]`` is the state of step ``s``, the unit index that is the last axis of `state_posteriors`, always
        ``< num_states``; -1 for a variable that no step reads.  `x`, `integrate_vars` and `rows_per_chunk` as for `log_prob`:
        missing entries are summed out (their emission row is zeros).  Between paths of equal score the choice is free.  A row
        without a path of positive mass has score -inf, a row that `log_prob` makes NaN has score NaN; both have -1 in every
        state.  Two launches: the max-product forward (`ck_hmm_viterbi_forward`) keeps its hand-off in a ``(B, D, K)`` scratch,
        the walk back (`ck_hmm_viterbi_backtrack`) recomputes each decision from it and one weight row.  A row's result does
        not depend on `rows_per_chunk`."""
        out, _, states = self._chain(x, integrate_vars, rows_per_chunk, "viterbi")
        return states, out

    def expected_statistics(self, x: torch.Tensor, integrate_vars=None, *, rows_per_chunk: int | None = None) -> ExpectedStatistics:
        """The Baum-Welch E-step: the expected sufficient statistics of every parameter under ``p(z | evidence)``, summed over the
        LIVE rows of the batch (evidence in range, finite ``log p``; a dead row contributes exactly nothing) -- the
        `ExpectedStatistics` of `HipCircuit.expected_statistics`, in the user plan's shapes and indexed by its layer index, so that
        `HipEMTrainer.apply` takes it.  ``edge[j]`` ``(1, Ko, K)`` of step ``s``'s layer: ``sum_b p(z_s = i, z_{s+1} = o | evidence of
        b)`` in entry ``[o, i]`` (the last step: ``Ko = 1``, ``sum_b gamma_{T-1}[b, i]``).  ``leaf[input layer]`` ``(F, K, C)``: fold
        ``f`` of step ``s`` gets ``gamma_s[b, k]`` in entry ``[k, x[b, var_s]]``; a live row that misses the variable (-1, or
        `integrate_vars`) spreads it over the layer's own ``p(c | k)``.  ``unit[j]`` the edge sums over the entries (step layers) or
        over the outputs (input folds), ``log_evidence`` ``(B,)`` what `log_prob` returns, ``rows`` the number of live rows.
        Categorical input layers only: any other raises ``NotImplementedError`` naming the layer before anything is allocated or
        launched.  Nothing is written into the parameter store.  Four launches per chunk of `rows_per_chunk` rows
        (`ck_hmm_forward_keep`, `ck_hmm_backward_stats`, `ck_hmm_pair_sum`, `ck_hmm_leaf_sum`) whatever ``T``, ``B`` and ``K``; by
        default a chunk holds each of its three ``(rows, D, K)`` buffers at or below 1 GiB.  Chunks add to the same sums in call
        order and no sum uses float atomics: the same `x` and `rows_per_chunk` give the same bits; different `rows_per_chunk`
        agree to rounding."""
        src = self.hc.user_plan.layers[self.input_layer]
        if not self.categorical:
            raise NotImplementedError(f"HipHMM.expected_statistics: layer {self.input_layer} ({src.type}) is not a Categorical "
                                      "input layer")
        D, T, K = self.plan.num_variables, len(self.steps), self.K
        if x.dim() != 2 or x.shape[1] != D:
            raise ValueError(f"expected x of shape (B, {D}), found {tuple(x.shape)}")
        if rows_per_chunk is not None and int(rows_per_chunk) <= 0:
            raise ValueError("rows_per_chunk must be positive")
        B = int(x.shape[0])
        if B <= 0:
            raise ValueError("empty batch")
        tab = self.tables()
        user = self.hc.user_plan.layers
        C, F = self.plan.layers[self.input_layer].config["num_categories"], int(tab["rows"].shape[0])
        n = min(B, int(rows_per_chunk) if rows_per_chunk is not None else max(1, _CHUNK_BYTES // (D * K * 4)))
        self.last_launches = 0
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            mask = self._mask(integrate_vars)
            x = x.to(self.device).to(torch.int64).contiguous()
            new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.device)  # noqa: E731
            out, gamma, pa, pr = new(B), new(n, D, K), new(n, D, K), new(n, D, K)
            edge = torch.zeros((T - 1) * K * K + K, dtype=torch.float32, device=self.device)
            leaf = torch.zeros((F, K, C), dtype=torch.float32, device=self.device)
            units = max(capi.load().ck_hmm_stats_scratch(T, K, C, nb) for nb in {n, B % n or n})
            capi.check(min(units, 0), "ck_hmm_stats_scratch")
            scratch = new(units * 1024) if units else None
            sp, sn = (None, 0) if scratch is None else (scratch.data_ptr(), scratch.numel())
            head = (tab["w"].data_ptr(), tab["fold"].data_ptr(), tab["var"].data_ptr(), T, K)
            mp = None if mask is None else mask.data_ptr()
            for r0 in range(0, B, n):
                nb = min(n, B - r0)
                source = (tab["rows"].data_ptr(), x[r0:].data_ptr(), D, C, mp, nb, out[r0:].data_ptr(), gamma.data_ptr())
                capi.call("ck_hmm_forward_keep", *head, *source, stream)
                capi.call("ck_hmm_backward_stats", *head, *source, pa.data_ptr(), pr.data_ptr(), stream)
                capi.call("ck_hmm_pair_sum", tab["w"].data_ptr(), tab["var"].data_ptr(), T, K, D, nb, pa.data_ptr(), pr.data_ptr(),
                          gamma.data_ptr(), edge.data_ptr(), sp, sn, stream)
                capi.call("ck_hmm_leaf_sum", tab["fold"].data_ptr(), tab["var"].data_ptr(), T, K, tab["rows"].data_ptr(),
                          x[r0:].data_ptr(), D, C, mp, nb, gamma.data_ptr(), leaf.data_ptr(), sp, sn, stream)
                self.last_launches += 4
            # back to the user plan's shapes (a padded unit carries no flow, a padded entry has weight 0)
            ku = self.num_states
            res = ExpectedStatistics({}, {}, [None] * len(user), out, torch.isfinite(out).sum(), kinds=[l.type for l in user])
            inner = edge[:(T - 1) * K * K].view(T - 1, K, K)[:, :ku, :ku]
            last = edge[-K:].view(1, K)[:, :ku]
            by_out, by_in = torch.cat([inner.sum(-1), last.sum(-1, keepdim=True).expand(1, ku)]), torch.cat([inner.sum(-2), last])
            into = torch.zeros((F, ku), dtype=torch.float32, device=self.device)  # flow into each input fold
            into.index_copy_(0, tab["fold"].long(), by_in)
            folds = [l.num_folds for l in self.plan.layers]
            for s, (st, w) in enumerate(zip(self.steps, tab["keep"])):
                ko = user[st.layer].num_output_units
                e = inner[s:s + 1] if s + 1 < T else last[None]
                res.edge[st.layer], res.support[st.layer] = e, w[:, :ko, :ku] > 0
                res.unit[st.layer] = by_out[s:s + 1, :ko]
                if s and user[st.layer].type == "sum":  # (unfused: the Hadamard layer below passes the same flow on)
                    res.unit[int(resolve_fold_index(self.plan.layers[st.layer].inputs, folds)[0][0][0])] = by_in[s:s + 1]
            res.unit[self.input_layer] = into
            res.leaf[self.input_layer] = leaf[:, :ku]
            res.support[self.input_layer] = (tab["rows"][:, :C, :ku] > -float("inf")).transpose(1, 2)
        return res

    def _need_categorical(self, query: str) -> None:
        if not self.categorical:
            src = self.hc.user_plan.layers[self.input_layer]
            raise NotImplementedError(f"HipHMM.{query}: layer {self.input_layer} ({src.type}) is not a Categorical input layer")

    def _emission_cdf(self, tab: dict, stream) -> int:
        """Leaves the ``(F, K, C)`` table of `sample_posterior` in ``tab["cdf"]``; the number of launches that took."""
        if "cdf" in tab:
            return 0
        rows = tab["rows"]
        F, C = int(rows.shape[0]), int(rows.shape[1]) - 1
        cdf = torch.empty((F, self.K, C), dtype=torch.float32, device=self.device)
        capi.call("ck_hmm_emission_cdf", rows.data_ptr(), F, self.K, C, cdf.data_ptr(), stream)
        tab["cdf"] = cdf
        return 1

    def sample_posterior(self, x: torch.Tensor, integrate_vars=None, *, num_samples: int = 1, seed: int = 0,
                         rows_per_chunk: int | None = None, return_log_prob: bool = False):
        """``(states, completed)``, both ``(B, S, D)`` int64 with ``S = num_samples``: `S` state paths per row drawn from
        ``p(z | evidence of the row)``, and the row completed along each.  ``states[b, j, var_s]`` is the state of step ``s`` in
        sample ``j`` of row ``b``, the unit index of `viterbi` and `state_posteriors`, always ``< num_states``; -1 for a variable
        that no step reads.  ``completed[b, j, v]`` is ``x[b, v]`` where that entry is observed and, where it is missing (-1, or
        `integrate_vars`), a draw from the emission ``p(c | z_s)`` of its step's fold given the sampled state.  With
        `return_log_prob` also the ``(B,)`` log-likelihood of the same forward pass.  `x` and `integrate_vars` as for `log_prob`.
        A row whose `log_prob` is -inf or NaN (no mass; a category outside the layer's range) has -1 in every state and at every
        missing entry; its observed entries are still copied.

        Forward-filter-backward-sample in two launches per chunk of `rows_per_chunk` rows (`ck_hmm_forward_keep`,
        `ck_hmm_sample_paths`) whatever ``T``, ``B``, ``K`` and ``S``; by default a chunk keeps the ``(rows, D, K)`` hand-off, which
        is scratch, at or below 1 GiB.  The first call after the parameters changed takes one launch more
        (`ck_hmm_emission_cdf`): the ``(F, K, C)`` fp32 table of cumulative emission probabilities, a contiguous row per (fold,
        state), kept with the other tables until the parameters change -- 67 MB at ``T, K, C = 256, 256, 256`` and at ``64, 1024,
        256``; the other queries never build it.  Draws follow the samplers' contract ("Sampling paths"):
        Philox4x32-10 keyed by `seed`, counter ``(b S + j, s, 0, 0)`` with ``b`` the row's index in `x`, one call per (sample,
        step), word 0 for the state and word 1 for the emission -- a sample depends on ``(seed, b, j)`` only, not on
        `rows_per_chunk` or on the other rows of the batch.  Categorical input layers only: any other raises
        ``NotImplementedError`` naming the layer before anything is allocated or launched.  Nothing is written into the
        parameter store."""
        self._need_categorical("sample_posterior")
        D, T, K = self.plan.num_variables, len(self.steps), self.K
        if x.dim() != 2 or x.shape[1] != D:
            raise ValueError(f"expected x of shape (B, {D}), found {tuple(x.shape)}")
        if rows_per_chunk is not None and int(rows_per_chunk) <= 0:
            raise ValueError("rows_per_chunk must be positive")
        B, S = int(x.shape[0]), int(num_samples)
        if B <= 0:
            raise ValueError("empty batch")
        if S <= 0:
            raise ValueError("num_samples must be positive")
        if B * S >= 2**32:
            raise ValueError(f"B * num_samples = {B * S} does not fit the 32-bit sample index of the draw's counter")
        tab = self.tables()
        C = self.plan.layers[self.input_layer].config["num_categories"]
        n = min(B, int(rows_per_chunk) if rows_per_chunk is not None else max(1, _CHUNK_BYTES // (D * K * 4)))
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            self.last_launches = self._emission_cdf(tab, stream)
            mask = self._mask(integrate_vars)
            mp = None if mask is None else mask.data_ptr()
            x = x.to(self.device).to(torch.int64).contiguous()
            out = torch.empty(B, dtype=torch.float32, device=self.device)
            keep = torch.empty((n, D, K), dtype=torch.float32, device=self.device)
            if D == T:
                states, completed = (torch.empty((B, S, D), dtype=torch.int64, device=self.device) for _ in range(2))
            else:  # (a variable that no step reads: no state, and its entry as it came)
                states = torch.full((B, S, D), -1, dtype=torch.int64, device=self.device)
                completed = x[:, None, :].expand(B, S, D).contiguous()
            head = (tab["w"].data_ptr(), tab["fold"].data_ptr(), tab["var"].data_ptr(), T, K)
            for r0 in range(0, B, n):
                nb = min(n, B - r0)
                capi.call("ck_hmm_forward_keep", *head, tab["rows"].data_ptr(), x[r0:].data_ptr(), D, C, mp, nb, out[r0:].data_ptr(),
                          keep.data_ptr(), stream)
                capi.call("ck_hmm_sample_paths", *head, self.num_states, tab["cdf"].data_ptr(), x[r0:].data_ptr(), D, C, mp, nb, S, r0,
                          int(seed) & (2**64 - 1), out[r0:].data_ptr(), keep.data_ptr(), states[r0:].data_ptr(),
                          completed[r0:].data_ptr(), stream)
                self.last_launches += 2
        return (states, completed, out) if return_log_prob else (states, completed)

    def sample(self, num_samples: int, *, seed: int = 0):
        """``(x, states)``, both ``(N, D)`` int64: `N` sequences from the model with the state paths that emitted them --
        `sample_posterior` of ONE row without evidence with ``num_samples = N``: the forward runs for one row, and the samples
        of that row carry the parallelism of the walk back."""
        self._need_categorical("sample")
        x = torch.full((1, self.plan.num_variables), -1, dtype=torch.int64, device=self.device)
        states, completed = self.sample_posterior(x, num_samples=num_samples, seed=seed)
        return completed[0], states[0]

    @property
    def generative_order(self) -> list[int]:
        """The variables in the order the chain generates them: the plan's last step holds the prior, so position ``j`` is the
        variable of step ``T - 1 - j`` -- for `templates.hmm(ordering)`, ``ordering`` itself."""
        return [s.var for s in reversed(self.steps)]

    def _emission_table(self, tab: dict, stream) -> int:
        """Leaves the ``(F, Cp, K)`` linear emission table of `autoregressive_conditionals` in ``tab["emission"]``; the number of
        launches that took."""
        if "emission" in tab:
            return 0
        rows = tab["rows"]
        F, C = int(rows.shape[0]), int(rows.shape[1]) - 1
        em = torch.empty((F, -(-C // 32) * 32, self.K), dtype=torch.float32, device=self.device)
        capi.call("ck_hmm_emission_table", rows.data_ptr(), F, self.K, C, em.data_ptr(), stream)
        tab["emission"] = em
        return 1

    def _predict_checks(self, x: torch.Tensor, query: str) -> int:
        self._need_categorical(query)
        D = self.plan.num_variables
        if x.dim() != 2 or x.shape[1] != D:
            raise ValueError(f"expected x of shape (B, {D}), found {tuple(x.shape)}")
        if int(x.shape[0]) <= 0:
            raise ValueError("empty batch")
        return int(x.shape[0])

    def _predict(self, tab: dict, x: torch.Tensor, mask, nb: int, lp: torch.Tensor, cond: torch.Tensor | None, stream) -> None:
        """One `ck_hmm_predict` launch on the first `nb` rows of `x` (a device tensor, int64, contiguous)."""
        C = self.plan.layers[self.input_layer].config["num_categories"]
        capi.call("ck_hmm_predict", tab["w"].data_ptr(), tab["fold"].data_ptr(), tab["var"].data_ptr(), len(self.steps), self.K,
                  tab["rows"].data_ptr(), x.data_ptr(), self.plan.num_variables, C, None if mask is None else mask.data_ptr(), nb,
                  lp.data_ptr(), None if cond is None else tab["emission"].data_ptr(), None if cond is None else cond.data_ptr(),
                  stream)

    def autoregressive_log_probs(self, x: torch.Tensor, integrate_vars=None) -> torch.Tensor:
        """``(B, T)`` fp32: entry ``[b, j]`` is ``log p(x[b, order[j]] | observed entries of row b among order[:j])`` with ``order =
        generative_order`` -- the chain-rule decomposition of `log_prob`, whose value a row sums to.  Exactly 0 where the row
        misses ``order[j]`` (-1, or `integrate_vars`).  Entries of `x` at ``order[j + 1:]`` do not influence position ``j``.  Where
        only the observed value has no mass the entry is -inf and every later one NaN (the prefix has no mass); a category
        ``>= C`` makes its own position and every later one NaN; no row affects another.  ONE launch (`ck_hmm_predict`,
        cirkit_amd/csrc/ck_hmm_predict.hip) whatever ``T``, ``B`` and ``K``: one walk down the chain, ``O(T)`` steps a row where
        `HipCircuit.autoregressive_log_probs` takes ``O(T^2)``; no forward pass, no ``(B, D, K)`` buffer, no host
        synchronisation, nothing written into the parameter store.  Categorical input layers only: any other raises
        ``NotImplementedError`` naming the layer before anything is allocated or launched."""
        B = self._predict_checks(x, "autoregressive_log_probs")
        tab = self.tables()
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            mask = self._mask(integrate_vars)
            x = x.to(self.device).to(torch.int64).contiguous()
            lp = torch.empty((B, len(self.steps)), dtype=torch.float32, device=self.device)
            self._predict(tab, x, mask, B, lp, None, stream)
            self.last_launches = 1
        return lp

    def autoregressive_conditionals(self, x: torch.Tensor, integrate_vars=None, *, return_log_probs: bool = False):
        """``(B, T, C)`` fp32 linear probabilities, as `HipCircuit.autoregressive_conditionals` returns them: entry ``[b, j, c]``
        is ``p(X_{order[j]} = c | observed entries of row b among order[:j])`` with ``order = generative_order`` -- also where the
        row misses ``order[j]``: that is the forecast.  A view of a buffer padded to 32 categories.  With `return_log_probs` also
        what `autoregressive_log_probs` returns, from the same launch.  Entries of `x` at ``order[j:]`` do not influence position
        ``j``; after a position whose observed value has no mass, and from a category ``>= C`` on, the row is NaN.  ONE launch
        (`ck_hmm_predict` with the predictive state contracted against the step's emission matrix on the matrix pipe); the first
        call after the parameters changed takes one more (`ck_hmm_emission_table`): the ``(F, Cp, K)`` fp32 table of linear
        emission probabilities, a contiguous row per (fold, category), kept with the other tables until the parameters change.
        Refusals, synchronisation and the parameter store as for `autoregressive_log_probs`."""
        B = self._predict_checks(x, "autoregressive_conditionals")
        tab = self.tables()
        C = self.plan.layers[self.input_layer].config["num_categories"]
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            launches = self._emission_table(tab, stream)
            mask = self._mask(integrate_vars)
            x = x.to(self.device).to(torch.int64).contiguous()
            lp = torch.empty((B, len(self.steps)), dtype=torch.float32, device=self.device)
            cond = torch.empty((B, len(self.steps), int(tab["emission"].shape[1])), dtype=torch.float32, device=self.device)
            self._predict(tab, x, mask, B, lp, cond, stream)
            self.last_launches = launches + 1
        return (cond[:, :, :C], lp) if return_log_probs else cond[:, :, :C]

    def coding_tables(self, x: torch.Tensor, integrate_vars=None, *, precision: int = 16,
                      rows_per_chunk: int | None = None) -> torch.Tensor:
        """``(B, T, C + 1)`` int32: the cumulative frequency table at ``2**precision`` of every conditional of
        `autoregressive_conditionals`, by the quantiser of `HipCircuit.coding_tables` (`ck_ar_quantise`) -- what the encoder of
        cirkit_amd/codec.py reads.  `precision` is checked as `autoregressive.check_precision` checks it, before anything is
        allocated or launched.  Two launches per chunk of `rows_per_chunk` rows (by default the chunk's conditionals at or below
        1 GiB), and the emission table's on the first call; a row's tables do not depend on `rows_per_chunk`."""
        from .autoregressive import check_precision

        B = self._predict_checks(x, "coding_tables")
        C, T = self.plan.layers[self.input_layer].config["num_categories"], len(self.steps)
        precision = check_precision(precision, C)
        if rows_per_chunk is not None and int(rows_per_chunk) <= 0:
            raise ValueError("rows_per_chunk must be positive")
        tab = self.tables()
        Cp = -(-C // 32) * 32
        n = min(B, int(rows_per_chunk) if rows_per_chunk is not None else max(1, _CHUNK_BYTES // (T * Cp * 4)))
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            self.last_launches = self._emission_table(tab, stream)
            mask = self._mask(integrate_vars)
            x = x.to(self.device).to(torch.int64).contiguous()
            lp = torch.empty((n, T), dtype=torch.float32, device=self.device)
            cond = torch.empty((n, T, Cp), dtype=torch.float32, device=self.device)
            # the quantiser sees Cp states of which the first C are live: the padded ones get no count, and entry C is the total
            out = torch.empty((B, T, C + 1), dtype=torch.int32, device=self.device)
            wide = out if Cp == C else torch.empty((n, T, Cp + 1), dtype=torch.int32, device=self.device)
            rowvar = torch.zeros(n * T, dtype=torch.int32, device=self.device)
            states = torch.full((1,), C, dtype=torch.int32, device=self.device)
            for r0 in range(0, B, n):
                nb = min(n, B - r0)
                self._predict(tab, x[r0:], mask, nb, lp, cond, stream)
                dst = out[r0:] if Cp == C else wide
                capi.call("ck_ar_quantise", cond.data_ptr(), rowvar.data_ptr(), states.data_ptr(), nb * T, Cp, precision,
                          dst.data_ptr(), stream)
                if Cp != C:
                    out[r0:r0 + nb] = wide[:nb, :, :C + 1]
                self.last_launches += 2
        return out

    def soft_evidence_log_prob(self, log_lik: torch.Tensor, x: torch.Tensor | None = None, *, soft_vars=None, integrate_vars=None,
                               rows_per_chunk: int | None = None) -> torch.Tensor:
        """``(B,)`` fp32: ``log Z(lambda) = log sum_x p(x) prod_s lambda[b, s, x_{v_s}]`` under soft (likelihood, Pearl's virtual)
        evidence, with `HipCircuit.soft_evidence_log_prob`'s argument conventions (`soft_evidence.soft_ids` and
        `check_arguments` on the user plan: the same forms, checks and error types).  `log_lik`: ``(B, S, C')`` floating point,
        ``C' >= C``, the logarithms of the weights of the soft variables in ascending order of variable id; entries at
        ``c >= C`` are never read.  `soft_vars`: one set for the batch, ``None`` for every variable.  `x`: ``(B, D)`` int64 hard
        evidence for the other variables, -1 missing, ``None`` all missing; its entries at soft variables are ignored.
        `integrate_vars` sums hard variables out as in `log_prob`; naming a soft variable there is a ``ValueError``.  Point
        evidence, missing entries and a set of allowed values per position are the 0 / 1 special cases of `log_lik`.

        Three launches per chunk of `rows_per_chunk` rows ("Soft evidence on chains"): `ck_hmm_soft_rows`
        writes the ``(F, rows, K)`` block of log emissions -- a soft one is ``log sum_c lambda_c p(c | k)``, contracted with the
        cached linear emission table on the matrix pipe -- `ck_hmm_forward` takes it as its row source and `ck_hmm_soft_flag`
        makes the flagged rows NaN.  The first call after the parameters changed takes one more (`ck_hmm_emission_table`).  By
        default a chunk keeps the block at or below 1 GiB.  A NaN or ``+inf`` entry read, or a hard category ``>= C``, makes its
        own row NaN; a soft variable whose entries read are all -inf makes it -inf; no row affects another and a row's value
        does not depend on `rows_per_chunk`.  `log_lik` is read where it lies (staged only if it is not contiguous fp32), no host
        synchronisation, nothing written into the parameter store.  Categorical input layers only: any other raises
        ``NotImplementedError`` naming the layer before anything is allocated or launched."""
        return self._soft("soft_evidence_log_prob", log_lik, x, soft_vars, integrate_vars, rows_per_chunk)[0]

    def soft_state_posteriors(self, log_lik: torch.Tensor, x: torch.Tensor | None = None, *, soft_vars=None, integrate_vars=None,
                              rows_per_chunk: int | None = None, return_log_evidence: bool = False):
        """``(B, D, num_states)`` fp32: ``p(z_v = k | lambda, x)``, `state_posteriors` under the evidence of
        `soft_evidence_log_prob` (same arguments, same row rules: a flagged row or one without mass is NaN in every entry); with
        `return_log_evidence` also ``log Z``.  Four launches per chunk: the block of emissions, the keeping forward, the flag,
        `ck_hmm_backward`."""
        out, post, _, _ = self._soft("soft_state_posteriors", log_lik, x, soft_vars, integrate_vars, rows_per_chunk)
        post = post[:, :, :self.num_states]
        return (post, out) if return_log_evidence else post

    def soft_posterior_marginals(self, log_lik: torch.Tensor, x: torch.Tensor | None = None, *, soft_vars=None, integrate_vars=None,
                                 rows_per_chunk: int | None = None, return_log_evidence: bool = False):
        """``(B, S, C)`` fp32: the posterior of every soft variable, ``[b, s, c] = d log Z / d log_lik[b, s, c] = p(x_{v_s} = c |
        lambda, x)``, with the meaning and NaN rules of `HipCircuit.soft_posterior_marginals` (not renormalised; a flagged row
        or one without mass is NaN; 0 where the weight is 0) -- a view of a buffer padded to 32 categories; with
        `return_log_evidence` also ``log Z``.  Five launches per chunk: the block of emissions, the keeping forward, the flag, the
        backward pass into a ``(rows, D, K)`` scratch (at or below 1 GiB by default) and `ck_hmm_soft_leaf`, which contracts
        ``gamma / y`` with the same emission table on the matrix pipe."""
        out, _, marg, _ = self._soft("soft_posterior_marginals", log_lik, x, soft_vars, integrate_vars, rows_per_chunk)
        marg = marg[:, :, :self.plan.layers[self.input_layer].config["num_categories"]]
        return (marg, out) if return_log_evidence else marg

    def soft_viterbi(self, log_lik: torch.Tensor, x: torch.Tensor | None = None, *, soft_vars=None, integrate_vars=None,
                     rows_per_chunk: int | None = None):
        """``(states, score)``: ``argmax_z sum_x p(z, x) prod_s lambda_s(x_{v_s})`` and its log value, with `viterbi`'s conventions
        (``states`` ``(B, D)`` int64 by variable id; a row without a path of positive mass has score -inf, a flagged row NaN, both
        -1 in every state).  Four launches per chunk: the block of emissions, `ck_hmm_viterbi_forward`, the flag -- before the walk
        back, which reads the score -- and `ck_hmm_viterbi_backtrack`."""
        out, _, _, states = self._soft("soft_viterbi", log_lik, x, soft_vars, integrate_vars, rows_per_chunk)
        return states, out

    def _soft(self, query: str, log_lik, x, soft_vars, integrate_vars, rows_per_chunk: int | None):
        """``(log Z or score, (B, D, K) state posteriors, (B, S, Cp) soft posteriors, (B, D) states)``, ``None`` where `query` does
        not ask for it."""
        from . import soft_evidence as se
        from .squared import _mask_of

        self._need_categorical(query)
        if rows_per_chunk is not None and int(rows_per_chunk) <= 0:
            raise ValueError("rows_per_chunk must be positive")
        ids = se.soft_ids(self.hc.user_plan, soft_vars)
        se.check_arguments(self.hc.user_plan, log_lik, x, ids)
        D, T, K = self.plan.num_variables, len(self.steps), self.K
        if integrate_vars is not None:
            both = [v for v in ids if _mask_of(integrate_vars, D)[v]]
            if both:
                raise ValueError(f"variables {both[:8]} are soft and in integrate_vars")
        keep, viterbi, leaf = query != "soft_evidence_log_prob", query == "soft_viterbi", query == "soft_posterior_marginals"
        whole = query == "soft_state_posteriors"  # (the (B, D, K) buffer is the result: no scratch per chunk)
        B, S, Cl = (int(n) for n in log_lik.shape)
        tab = self.tables()
        C, F = self.plan.layers[self.input_layer].config["num_categories"], int(tab["rows"].shape[0])
        Cp = -(-C // 32) * 32
        per_row = 4 * K * max(F, D if keep and not whole else 0)
        n = min(B, int(rows_per_chunk) if rows_per_chunk is not None else max(1, _CHUNK_BYTES // per_row))
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            self.last_launches = self._emission_table(tab, stream)
            sets = tab.setdefault("soft", {})
            if tuple(ids) not in sets:  # the soft slot of every step, and the step of every soft slot
                slot_of = {v: j for j, v in enumerate(ids)}
                step_of = {s.var: t for t, s in enumerate(self.steps)}
                sets[tuple(ids)] = tuple(torch.tensor(a, dtype=torch.int32).to(self.device) for a in (
                    [slot_of.get(s.var, -1) for s in self.steps], [step_of.get(v, -1) for v in ids]))
            step_slot, soft_step = sets[tuple(ids)]
            mask = self._mask(integrate_vars) if x is not None else None
            mp = None if mask is None else mask.data_ptr()
            ll = log_lik.to(self.device).to(torch.float32).contiguous()  # (as it lies where it is contiguous fp32 on the device)
            ldx = 0
            if x is not None:
                x = x.to(self.device).to(torch.int64).contiguous()
                ldx = int(x.shape[1])
            new = lambda *shape: (torch.zeros if D != T else torch.empty)(shape, dtype=torch.float32, device=self.device)  # noqa: E731
            out = torch.empty(B, dtype=torch.float32, device=self.device)
            block = torch.empty((F, n, K), dtype=torch.float32, device=self.device)
            m = torch.empty((T, n), dtype=torch.float32, device=self.device)
            flags = torch.empty((T, n), dtype=torch.int32, device=self.device)
            post = new(B if whole else n, D, K) if keep else None
            marg = torch.empty((B, S, Cp), dtype=torch.float32, device=self.device) if leaf else None
            states = None
            if viterbi:  # (-1 where no step writes)
                states = (torch.empty((B, D), dtype=torch.int64, device=self.device) if D == T else
                          torch.full((B, D), -1, dtype=torch.int64, device=self.device))
            em = tab["emission"].data_ptr()
            steps = (tab["fold"].data_ptr(), tab["var"].data_ptr(), T, K)
            head = (tab["w"].data_ptr(), *steps)
            for r0 in range(0, B, n):
                nb = min(n, B - r0)
                lp, o = ll[r0:].data_ptr(), out[r0:].data_ptr()
                kp = None if post is None else (post[r0:] if whole else post).data_ptr()
                capi.call("ck_hmm_soft_rows", lp, S, Cl, step_slot.data_ptr(), *steps, tab["rows"].data_ptr(), em,
                          None if x is None else x[r0:].data_ptr(), ldx, C, mp, nb, block.data_ptr(), m.data_ptr(), flags.data_ptr(),
                          stream)
                source = (block.data_ptr(), None, D, 0, None, nb, o)  # (a block source: its missing entries are in the block)
                if not keep:
                    capi.call("ck_hmm_forward", *head, *source, stream)
                else:
                    capi.call("ck_hmm_viterbi_forward" if viterbi else "ck_hmm_forward_keep", *head, *source, kp, stream)
                capi.call("ck_hmm_soft_flag", flags.data_ptr(), T, nb, o, stream)
                if viterbi:
                    capi.call("ck_hmm_viterbi_backtrack", tab["w"].data_ptr(), tab["var"].data_ptr(), T, K, self.num_states, D, nb, o,
                              kp, states[r0:].data_ptr(), stream)
                elif keep:
                    capi.call("ck_hmm_backward", *head, *source, kp, stream)
                if leaf:
                    capi.call("ck_hmm_soft_leaf", lp, S, Cl, soft_step.data_ptr(), *steps, em, C, block.data_ptr(), m.data_ptr(), kp, D,
                              nb, o, marg[r0:].data_ptr(), stream)
                self.last_launches += 3 + keep + leaf
        return out, (post if whole else None), marg, states

    def _chain(self, x: torch.Tensor, integrate_vars, rows_per_chunk: int | None, query: str):
        """``(log_prob, None, None)`` by the forward launch; ``(log_prob, (B, D, K) posteriors, None)`` by the keeping forward
        and the backward pass; ``(score, (B, D, K) hand-off, (B, D) states)`` by the max-product forward and the walk back."""
        keep, viterbi = query != "log_prob", query == "viterbi"
        D = self.plan.num_variables
        if x.dim() != 2 or x.shape[1] != D:
            raise ValueError(f"expected x of shape (B, {D}), found {tuple(x.shape)}")
        if rows_per_chunk is not None and int(rows_per_chunk) <= 0:
            raise ValueError("rows_per_chunk must be positive")
        B, T = int(x.shape[0]), len(self.steps)
        if B <= 0:
            raise ValueError("empty batch")
        hc, tab = self.hc, self.tables()
        self.last_launches = 0
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            # one buffer for both results (the range check of discrete inputs poisons it in one launch): the posteriors start
            # 16-byte aligned, and are 0 for a variable that no step reads
            Bp = -(-B // 4) * 4
            flat = (torch.zeros if keep and not viterbi and D != T else torch.empty)(Bp + (B * D * self.K if keep else 0),
                                                                                     dtype=torch.float32, device=self.device)
            out, post = flat[:B], (flat[Bp:].view(B, D, self.K) if keep else None)
            states = None
            if viterbi:  # (-1 where no step writes)
                states = (torch.empty((B, D), dtype=torch.int64, device=self.device) if D == T else
                          torch.full((B, D), -1, dtype=torch.int64, device=self.device))
            head = (tab["w"].data_ptr(), tab["fold"].data_ptr(), tab["var"].data_ptr(), T, self.K)

            def backtrack(nb, r0):
                capi.call("ck_hmm_viterbi_backtrack", tab["w"].data_ptr(), tab["var"].data_ptr(), T, self.K, self.num_states, D, nb,
                          out[r0:].data_ptr(), post[r0:].data_ptr(), states[r0:].data_ptr(), stream)
                return 1

            def run(source, nb, r0):
                if not keep:
                    capi.call("ck_hmm_forward", *head, *source, nb, out[r0:].data_ptr(), stream)
                    return 1
                if viterbi:
                    capi.call("ck_hmm_viterbi_forward", *head, *source, nb, out[r0:].data_ptr(), post[r0:].data_ptr(), stream)
                    return 1 + (backtrack(nb, r0) if self.categorical else 0)
                capi.call("ck_hmm_forward_keep", *head, *source, nb, out[r0:].data_ptr(), post[r0:].data_ptr(), stream)
                capi.call("ck_hmm_backward", *head, *source, nb, out[r0:].data_ptr(), post[r0:].data_ptr(), stream)
                return 2

            if self.categorical:
                mask = self._mask(integrate_vars)
                x = x.to(self.device).to(torch.int64).contiguous()
                C = self.plan.layers[self.input_layer].config["num_categories"]
                self.last_launches = run((tab["rows"].data_ptr(), x.data_ptr(), D, C, None if mask is None else mask.data_ptr()), B, 0)
                return out, post, states
            # any other input layer: its own launch writes the (F, rows, K) emissions of a chunk, missing entries included
            if integrate_vars is not None:
                x = hc._apply_integration_mask(x.to(self.device), integrate_vars)
            layer = hc.layers[self.input_layer]
            n = min(B, int(rows_per_chunk) if rows_per_chunk is not None else self.rows_per_chunk())
            rows = torch.empty((layer.num_folds, n, self.K), dtype=torch.float32, device=self.device)
            xt = torch.empty((D, n), dtype=torch.float32 if layer.wants_float_input else torch.int32, device=self.device)
            for r0 in range(0, B, n):
                nb = min(n, B - r0)
                xf, xi = hc._prepare_input(x[r0:r0 + nb])
                if layer.wants_float_input:
                    capi.call("ck_transpose_f32", xf.data_ptr(), xt.data_ptr(), nb, D, stream)
                else:
                    capi.call("ck_stage_categories", xi.data_ptr(), xt.data_ptr(), nb, D, hc._num_states_dev().data_ptr(),
                              hc._bad_input.data_ptr(), 0, None, stream)
                layer.launch_input(xt, D, rows, nb, stream)
                self.last_launches += 2 + run((rows.data_ptr(), None, D, 0, None), nb, r0)
            if not layer.wants_float_input:
                capi.call("ck_poison_outputs", flat.data_ptr(), flat.numel(), hc._bad_input.data_ptr(), stream)
                self.last_launches += 1
            if viterbi:  # the walk back reads the score, so it follows the range check's verdict on it
                self.last_launches += sum(backtrack(min(n, B - r0), r0) for r0 in range(0, B, n))
        return out, post, states

    def __call__(self, x: torch.Tensor, *, integrate_vars=None) -> torch.Tensor:
        """``(B, 1, 1)`` like `HipCircuit.forward`."""
        return self.log_prob(x, integrate_vars).view(-1, 1, 1)
