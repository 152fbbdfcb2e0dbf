"""Exact ancestral sampling on the GPU: `HipCircuit.sample` and a reference-shaped `SamplingQuery`.

Replaces the reference's ``SamplingQuery`` (cirkit/backend/torch/queries.py:187-275) and the ``sample()`` methods of its
layers.  The reference samples bottom up -- every unit of every layer draws a full ``(N, D)`` assignment and the sum layers
gather among those draws -- and refuses circuits whose sum weights are not normalised.  This module samples TOP DOWN from
``p(x) = c(x) / Z`` for any smooth, decomposable, monotonic circuit, normalised or not:

* a unit on the induced tree of a sample draws its input entry in proportion to weight x partition function of that entry
  (the partition function of every unit: the circuit's own marginal forward at B = 1 with every variable integrated, run
  layer by layer on the same `TensorStore`);
* the conditional draws are fp32 CDF rows written once per parameter state (`ck_sample_cdf`), the walk is one launch per
  call (`ck_sample_walk`); randomness is Philox4x32-10 with counter (sample, global fold id, 0, 0) (cirkit_amd/csrc/ck_philox.h).

On a normalised circuit every partition function is 1 and the distribution is the reference's.

`HipCircuit.sample_conditional` draws the unobserved part of every row from ``p(x_S | x_O)``: the same walk, weighted by the
per-row unit values of the layer-wise marginal forward of the row's evidence instead of the partition functions, so its CDF
rows are built on the device per (fold, sample) (`ck_sample_cond_walk`, DESIGN.md section 11 "Conditional sampling").
"""

from __future__ import annotations

from typing import TYPE_CHECKING

import numpy as np
import torch

from . import _capi as capi
from .parameters import HipParameter
from .plan import Plan, resolve_fold_index

if TYPE_CHECKING:  # pragma: no cover
    from .circuit import HipCircuit

_REFUSED = {"embedding": "TorchEmbeddingLayer", "constant": "TorchConstantValueLayer", "tensordot": "TorchTensorDotLayer"}
_SUPPORTED = {"categorical", "binomial", "gaussian", "sum", "cpt", "tucker", "hadamard", "kronecker"}


def _is_mixing(spec) -> bool:
    g = spec.params["weight"]
    return spec.type == "sum" and len(g.output.ids) == 1 and g.nodes[g.output.ids[0]].op == "mixing_weight"


def check_plan(plan: Plan) -> None:
    """Refuse, before anything is launched, what cannot be sampled: a plan that is not a monotonic lse-sum circuit
    (``ValueError``, checked first), a layer without a sampler (``TypeError`` naming it, as the reference's
    layers/inner.py:66-82 do), an input layer over more than one variable (``NotImplementedError``, queries.py:266-267)."""
    if plan.semiring != "lse-sum":
        raise ValueError(f"sampling needs a monotonic circuit in the lse-sum semiring, this plan is {plan.semiring!r}")
    for i, l in enumerate(plan.layers):
        if l.type in _REFUSED:
            raise TypeError(f"Sampling is not supported for layers of type {_REFUSED[l.type]} (layer {i})")
        if l.type not in _SUPPORTED:
            raise TypeError(f"Sampling is not supported for layers of type {l.type!r} (layer {i})")
        if l.inputs is None and l.scope_idx is not None and l.scope_idx.shape[1] != 1:
            raise NotImplementedError("Sampling input layers over more than one variable is not supported")
        if l.type == "tucker" and l.arity != 2:
            raise NotImplementedError(f"sampling a Tucker layer of arity {l.arity} (layer {i}): arity 2 only")


def _choice_map(spec, user_spec) -> np.ndarray:
    """Entry i of a padded CDF row -> the choice in the user's unit numbering (-1: a padded entry, never drawn)."""
    kp, ku = spec.num_input_units, user_spec.num_input_units
    if spec.type == "cpt":
        i = np.arange(kp)
        return np.where(i < ku, i, -1).astype(np.int32)
    if spec.type == "tucker":
        a, b = np.divmod(np.arange(kp * kp), kp)
        return np.where((a < ku) & (b < ku), a * ku + b, -1).astype(np.int32)
    h, k = np.divmod(np.arange(spec.arity * kp), kp)
    if _is_mixing(spec):
        return h.astype(np.int32)
    return np.where(k < ku, h * ku + k, -1).astype(np.int32)


_CHUNK_ARENA_BYTES = 2 << 30  # default bound of the evidence forward's activation arena (`sample_conditional`)


def chunk_rows(B: int, rows_per_chunk: int | None, arena_bytes_per_row: int) -> list[tuple[int, int]]:
    """(first row, rows) of each chunk of a `sample_conditional` batch of B rows: `rows_per_chunk` rows each (None: as many as
    keep the evidence forward's arena <= 2 GiB), the last chunk the remainder.  Two sizes at most: the chunk and the tail."""
    if rows_per_chunk is None:
        R = max(1, _CHUNK_ARENA_BYTES // max(1, int(arena_bytes_per_row)))
    else:
        R = int(rows_per_chunk)
        if R <= 0:
            raise ValueError("rows_per_chunk must be positive")
    R = min(R, B)
    return [(r0, min(R, B - r0)) for r0 in range(0, B, R)]


def fold_block_offsets(bases, folds, units, B: int) -> np.ndarray:
    """(total folds) int64 `val_off` of `ck_sample_cond_walk`: the element offset, from the arena base, of global fold g's
    (B, Ko) block, for layers whose (F, B, Ko) outputs start at element offsets `bases`."""
    return np.concatenate([int(b) + np.arange(int(f), dtype=np.int64) * int(B) * int(k) for b, f, k in zip(bases, folds, units)]
                          ).astype(np.int64)


class Sampler:
    """The sampling state of one `HipCircuit`: the walk's structure (built once) and the CDF tables of the last parameter
    state (built by `prepare`)."""

    def __init__(self, hc: "HipCircuit") -> None:
        check_plan(hc.user_plan)
        plan, user = hc.plan, hc.user_plan
        self.hc, self.plan = hc, plan
        self.device = hc.device
        self.store = hc.store
        folds = [l.num_folds for l in plan.layers]
        self.fold_off = np.concatenate([[0], np.cumsum(folds)]).astype(np.int64)
        self.total_folds = int(self.fold_off[-1])
        self.D = int(plan.num_variables)
        if self.D <= 0:
            raise ValueError("sampling needs a circuit over at least one variable")
        self.S = min(64, capi.CK_SAMPLE_MAX_LDS // (2 * self.total_folds))
        if self.S < 1:
            raise NotImplementedError(f"sampling a circuit of {self.total_folds} folds (at most {capi.CK_SAMPLE_MAX_LDS // 2})")
        units = [l.num_output_units for l in plan.layers]
        if max(units) >= 32768:
            raise NotImplementedError("sampling layers of 32768 units or more")
        out = resolve_fold_index(plan.output, folds).reshape(-1, 2)
        self.root_layer, self.root_f = int(out[0, 0]), int(out[0, 1])  # (layer, fold) of the root unit
        self.root_fold = int(self.fold_off[self.root_layer] + self.root_f)
        self.float_out = any(l.type == "gaussian" for l in plan.layers)
        self.dtype = torch.float32 if self.float_out else torch.int64
        dev = self.device
        covered = np.zeros(self.D, dtype=bool)
        self.layers: list[dict] = []
        self.sum_layers: list[int] = []
        # (the log partition function of unit k of fold f of layer p sits at zoff[p] + f Ko_p + k of the flattened layer outputs)
        zoff = np.concatenate([[0], np.cumsum([f * k for f, k in zip(folds, units)])]).astype(np.int64)
        self.root_z = int(zoff[self.root_layer] + self.root_f * units[self.root_layer])
        for j, (s, us) in enumerate(zip(plan.layers, user.layers)):
            d: dict = {"spec": s, "F": s.num_folds, "H": s.arity, "Ki": s.num_input_units, "Ko": s.num_output_units}
            if s.inputs is None:
                scope = np.asarray(s.scope_idx[:, 0], dtype=np.int64)
                if scope.size and (scope.min() < 0 or scope.max() >= self.D):
                    raise ValueError(f"input layer {j} has a variable outside 0 .. {self.D - 1}")
                covered[scope] = True
                d["scope"] = torch.from_numpy(scope).to(dev)
                if s.type == "gaussian":
                    d["kind"] = capi.CK_SAMPLE_GAUSSIAN
                    d["mean"] = HipParameter(s.params["mean"], self.store)
                    d["stddev"] = HipParameter(s.params["stddev"], self.store)
                    d["M"] = 1
                else:
                    d["kind"] = capi.CK_SAMPLE_CATEGORICAL
                    pn = "probs" if "probs" in s.params else "logits"
                    d["param"], d["is_logits"] = HipParameter(s.params[pn], self.store), pn == "logits"
                    d["M"] = int(s.config["num_categories"]) if s.type == "categorical" else int(s.config["total_count"]) + 1
                self.layers.append(d)
                continue
            ch = resolve_fold_index(s.inputs, folds)  # (F, H, 2)
            if ch.shape[:2] != (s.num_folds, s.arity):
                raise ValueError(f"fold index of layer {j} has shape {ch.shape[:2]}, expected {(s.num_folds, s.arity)}")
            if any(units[int(p)] != s.num_input_units for p in np.unique(ch[..., 0])):
                raise ValueError(f"layer {j} reads inputs whose unit count is not its num_input_units")
            d["child"] = torch.from_numpy((self.fold_off[ch[..., 0]] + ch[..., 1]).astype(np.int32)).to(dev)
            Ki = s.num_input_units
            if s.type == "hadamard":
                d["kind"], d["M"] = capi.CK_SAMPLE_HADAMARD, 1
            elif s.type == "kronecker":
                if s.num_output_units != Ki ** s.arity:
                    raise ValueError(f"Kronecker layer {j}: {s.num_output_units} output units for {s.arity} inputs of {Ki}")
                d["kind"], d["M"] = capi.CK_SAMPLE_KRONECKER, 1
            else:
                d["kind"] = {"sum": capi.CK_SAMPLE_SUM, "cpt": capi.CK_SAMPLE_CPT, "tucker": capi.CK_SAMPLE_TUCKER}[s.type]
                d["M"] = {"sum": s.arity * Ki, "cpt": Ki, "tucker": Ki * Ki}[s.type]
                d["weight"] = HipParameter(s.params["weight"], self.store)
                zidx = zoff[ch[..., 0]][..., None] + ch[..., 1][..., None] * Ki + np.arange(Ki)  # (F, H, Ki)
                d["zidx"] = torch.from_numpy(zidx).to(dev)
                d["cmap"] = torch.from_numpy(_choice_map(s, us)).to(dev)
                self.sum_layers.append(j)
            self.layers.append(d)
        self.zero_fill = not covered.all()  # (variables outside every input layer's scope read 0)
        self.uncovered = torch.from_numpy(np.nonzero(~covered)[0]).to(dev)  # (copied once: a call does not wait on the host)
        self._zc = None
        self._wtab: tuple | None = None  # (parameter key, device table of the sum-type layers' linear weights)
        self._val_off: dict[int, tuple[int, torch.Tensor]] = {}  # chunk rows -> (arena address, val_off table)
        self._key = None
        self._table: torch.Tensor | None = None  # the device descriptor table without choices
        self._desc: np.ndarray | None = None
        self._mpe = None  # the `MPEState` (cirkit_amd/mpe.py), built by the first `mpe` call
        self._mmap = None  # the `MarginalMapState` (cirkit_amd/marginal_map.py), built by the first `marginal_map` call
        self._posterior = None  # the `PosteriorState` (cirkit_amd/posterior.py), built by the first `posterior_marginals` call
        self._interval = None  # the `IntervalState` (cirkit_amd/interval.py), built by the first `interval_log_prob` call
        self._soft = None  # the `SoftEvidenceState` (cirkit_amd/soft_evidence.py), built by the first soft-evidence call
        self._soft_decode = None  # the `SoftDecodeState` (cirkit_amd/soft_decode.py), built by the first soft_mpe / sample_soft

    # -- once per parameter state ------------------------------------------------------------------------------------
    def _z_circuit(self):
        if self._zc is None:
            from .circuit import HipCircuit

            # layer by layer: every layer output (= the log partition function of each unit at B = 1) is materialised
            self._zc = HipCircuit(self.plan, self.store, device=self.device, fuse=False, pad_units=False, use_graph=False)
        return self._zc

    def prepare(self) -> None:
        """The CDF tables of the store's current values; a no-op when nothing changed since the last call."""
        st = self.store
        key = (st.version, st.state(), st.raw_writes)
        if key == self._key:
            return
        zc = self._z_circuit()
        dev = self.device
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            xm = torch.full((1, self.D), float("nan"), device=dev) if zc._float_input else \
                torch.full((1, self.D), -1, dtype=torch.int64, device=dev)
            views = zc.layer_outputs(xm)  # (F, 1, Ko) log partition functions
            zflat = torch.cat([v.reshape(-1) for v in views])
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            desc = np.zeros(len(self.layers), dtype=capi.SAMPLE_LAYER_DTYPE)
            for j, d in enumerate(self.layers):
                F, Ko, M = d["F"], d["Ko"], d["M"]
                kind = d["kind"]
                e = desc[j]
                e["type"], e["F"], e["H"], e["Ki"], e["Ko"], e["M"] = kind, F, d["H"], d["Ki"], Ko, M
                e["fold_off"] = int(self.fold_off[j])
                if "child" in d:
                    e["child"] = d["child"].data_ptr()
                if "scope" in d:
                    e["scope"] = d["scope"].data_ptr()
                if kind == capi.CK_SAMPLE_GAUSSIAN:
                    d["mean_v"] = d["mean"].evaluate(stream).reshape(F, Ko).contiguous().clone()
                    d["stddev_v"] = d["stddev"].evaluate(stream).reshape(F, Ko).contiguous().clone()
                    e["mean"], e["stddev"] = d["mean_v"].data_ptr(), d["stddev_v"].data_ptr()
                    continue
                if kind in (capi.CK_SAMPLE_HADAMARD, capi.CK_SAMPLE_KRONECKER):
                    continue
                cdf = d.get("cdf")
                if cdf is None:
                    cdf = d["cdf"] = torch.empty((F, Ko, M), dtype=torch.float32, device=dev)
                if kind == capi.CK_SAMPLE_CATEGORICAL:
                    v = d["param"].evaluate(stream)
                    if v.is_complex():
                        raise ValueError("sampling an input layer with complex parameters")
                    if d["spec"].type == "binomial":  # log-pmf table (F, T + 2, K), last row the integral
                        tab = d["tab"] = torch.empty((F, M + 1, Ko), dtype=torch.float32, device=dev)
                        capi.call("ck_param_binomial_table", v.contiguous().data_ptr(), 1 if d["is_logits"] else 0,
                                  tab.data_ptr(), F, Ko, M - 1, stream)
                        w, strides, w_log = tab, ((M + 1) * Ko, 1, Ko), 1
                    else:  # (F, K, C): probabilities, or logits taken as log-likelihoods (layers/input.py:405-408)
                        w = d["tab"] = v.reshape(F, Ko, M).contiguous()
                        strides, w_log = (Ko * M, M, 1), 1 if d["is_logits"] else 0
                    capi.call("ck_sample_cdf", w.data_ptr(), *strides, w_log, None, F, Ko, M, cdf.data_ptr(), flag.data_ptr(),
                              stream)
                else:
                    w = d["w"] = d["weight"].evaluate(stream).reshape(F, Ko, M).contiguous()
                    if w.is_complex():
                        raise ValueError("sampling a sum layer with complex weights")
                    zc_ = zflat[d["zidx"]]  # (F, H, Ki) log partition functions of the entries' inputs
                    if kind == capi.CK_SAMPLE_CPT:
                        lz = zc_.sum(1)
                    elif kind == capi.CK_SAMPLE_TUCKER:
                        lz = (zc_[:, 0, :, None] + zc_[:, 1, None, :]).reshape(F, M)
                    else:
                        lz = zc_.reshape(F, M)
                    lz = d["lz"] = lz.contiguous()
                    capi.call("ck_sample_cdf", w.data_ptr(), Ko * M, M, 1, 0, lz.data_ptr(), F, Ko, M, cdf.data_ptr(),
                              flag.data_ptr(), stream)
                    e["cmap"] = d["cmap"].data_ptr()
                e["cdf"] = cdf.data_ptr()
            root = zflat[self.root_z]
            check = torch.stack([flag.to(torch.float32)[0], root]).cpu()  # one read per parameter state
        bad, logz = int(check[0]), float(check[1])
        if bad & 1:
            raise ValueError("sampling needs a monotonic circuit: a sum weight or input probability is negative")
        if bad & 2:
            raise ValueError("sampling met a NaN / infinite weight or partition function")
        if not np.isfinite(logz):
            raise ValueError(f"the partition function of the sampled unit is {np.exp(logz)} (log {logz}): nothing to sample")
        self._desc = desc
        self._table = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
        self._key = key

    # -- once per call ------------------------------------------------------------------------------------------------
    def sample(self, num_samples: int, seed: int | None = None, return_choices: bool = False):
        N = int(num_samples)
        if N <= 0:
            raise ValueError("num_samples must be positive")
        seed = _seed(seed)
        self.prepare()
        dev = self.device
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            alloc = torch.zeros if self.zero_fill else torch.empty
            x = alloc((N, self.D), dtype=self.dtype, device=dev)
            table, choices = self.choice_table(N) if return_choices else (self._table, None)
            capi.call("ck_sample_walk", table.data_ptr(), len(self.layers), self.root_fold, 0, self.total_folds, self.S, N,
                      self.D, seed, x.data_ptr(), 1 if self.float_out else 0, stream)
        return pack(x, choices, None)

    # -- shared by the evidence queries: `sample_conditional` and `mpe` (cirkit_amd/mpe.py) ----------------------------
    def evidence_batch(self, x: torch.Tensor, vars_) -> torch.Tensor:
        """The (B, D) batch `x` with the variables `vars_` marks set to the sentinel, on the device in the output dtype.
        Raises before anything is prepared or launched."""
        if not isinstance(x, torch.Tensor) or x.dim() != 2:
            raise ValueError("The input to the circuit should have shape (B, D), where B is the batch size and D "
                             "is the number of variables the circuit is defined on")
        if x.shape[1] < self.D:
            raise ValueError(f"expected at least {self.D} variables, found {x.shape[1]}")
        if x.shape[0] <= 0:
            raise ValueError("empty batch")
        return self.hc._apply_integration_mask(x[:, :self.D].to(self.device), vars_).to(self.dtype).contiguous()

    def choice_table(self, N: int) -> tuple[torch.Tensor, list[torch.Tensor]]:
        """The device descriptor table with an (F, N) int32 choices tensor for every sum-type layer, and those tensors.
        The table is kept until the next call: the walk that reads it is asynchronous."""
        desc = self._desc.copy()
        choices = []
        for j in self.sum_layers:
            c = torch.empty((self.layers[j]["F"], N), dtype=torch.int32, device=self.device)
            desc[j]["choices"] = c.data_ptr()
            choices.append(c)
        self._keep = torch.from_numpy(desc.view(np.uint8).copy()).pin_memory().to(self.device, non_blocking=True)
        return self._keep, choices

    def fill_uncovered(self, out: torch.Tensor, root_value: torch.Tensor) -> None:
        """Variables outside every input layer's scope read 0, as `sample` writes, in the rows whose root value is finite."""
        if self.zero_fill:
            u = self.uncovered
            cols = out[:, u]
            sent = torch.isnan(cols) if self.float_out else cols < 0
            zero = torch.zeros((), dtype=out.dtype, device=out.device)
            out[:, u] = torch.where(sent & torch.isfinite(root_value)[:, None], zero, cols)

    # -- conditional sampling ---------------------------------------------------------------------------------------
    def _weight_table(self) -> torch.Tensor:
        """Device array of one pointer per layer: the (F, Ko, M) linear weights `prepare` evaluated, NULL for the others."""
        if self._wtab is None or self._wtab[0] != self._key:
            self._wtab = (self._key, ptr_table([d.get("w") for d in self.layers], self.device))
        return self._wtab[1]

    def _val_off_table(self, bd) -> torch.Tensor:
        """(total_folds) int64: element offset of global fold g's (B, Ko) block from the arena base of binding `bd`."""
        hit = self._val_off.get(bd.B)
        if hit is not None and hit[0] == bd.arena.data_ptr():
            return hit[1]
        base = bd.arena.data_ptr()
        off = fold_block_offsets([(v.data_ptr() - base) // v.element_size() for v in bd.views],
                                 [l.num_folds for l in self.plan.layers], [l.num_output_units for l in self.plan.layers], bd.B)
        t = torch.from_numpy(off).to(self.device)
        self._val_off[bd.B] = (base, t)
        return t

    def sample_conditional(self, x: torch.Tensor, sample_vars, seed: int | None = None, return_choices: bool = False,
                           return_log_evidence: bool = False, rows_per_chunk: int | None = None):
        xm = self.evidence_batch(x, sample_vars)
        B = int(xm.shape[0])
        chunks = chunk_rows(B, rows_per_chunk, self.hc.arena_bytes(1))
        sizes = {nb for _, nb in chunks}
        seed = _seed(seed)
        self.prepare()
        zc = self._z_circuit()
        for b in [b for b in zc._bindings if b != 1 and b not in sizes]:  # two batch sizes bound: the chunk and the tail
            zc._bindings.pop(b).destroy()
            self._val_off.pop(b, None)
        dev = self.device
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            out = xm.clone()  # (the sentinels mark what is left to draw)
            logev = torch.empty(B, dtype=torch.float32, device=dev)
            table, choices = self.choice_table(B) if return_choices else (self._table, None)
            wtab = self._weight_table()
            for r0, nb in chunks:
                bd = zc._run(xm[r0 : r0 + nb])
                # the evidence is range-checked where it is staged, on the private circuit's flag: move a hit to the flag
                # `hc.check_inputs()` reports (that chunk's outputs are NaN, as `hc(x)`'s would be) and clear this one, so
                # that later forwards of the private circuit -- `prepare()` included -- are not poisoned by it
                if self.hc.validate_inputs:
                    self.hc._bad_input.bitwise_or_(zc._bad_input)
                zc._bad_input.zero_()
                logev[r0 : r0 + nb].copy_(bd.views[self.root_layer][self.root_f, :, 0])
                capi.call("ck_sample_cond_walk", table.data_ptr(), wtab.data_ptr(), len(self.layers), self.root_fold, 0,
                          self.total_folds, self.S, bd.arena.data_ptr(), self._val_off_table(bd).data_ptr(), r0, nb, B,
                          self.D, seed, xm[r0].data_ptr(), out[r0].data_ptr(), 1 if self.float_out else 0, stream)
            self.fill_uncovered(out, logev)
        return pack(out, choices, logev if return_log_evidence else None)


def _seed(seed: int | None) -> int:
    """The walk's 64-bit Philox key; None draws it from torch's default CPU generator (torch.manual_seed reproduces it)."""
    if seed is None:
        seed = int(torch.randint(0, 2**63 - 1, (1,), dtype=torch.int64).item())
    return int(seed) & (2**64 - 1)


def ptr_table(tensors, device) -> torch.Tensor:
    """A device array of one pointer per layer: each tensor's address, NULL for None."""
    ptrs = np.array([0 if t is None else t.data_ptr() for t in tensors], dtype=np.uint64)
    return torch.from_numpy(ptrs.view(np.int64)).to(device)


def pack(out: torch.Tensor, choices: list | None, value: torch.Tensor | None):
    """A query's result: the output, then the choices and the per-row value where they were asked for."""
    res = (out,) + ((choices,) if choices is not None else ()) + ((value,) if value is not None else ())
    return res[0] if len(res) == 1 else res


def sampler(hc: "HipCircuit") -> Sampler:
    """The circuit's `Sampler`, built on first use."""
    s = getattr(hc, "_sampler", None)
    if s is None:
        s = hc._sampler = Sampler(hc)
    return s


def sample(hc: "HipCircuit", num_samples: int, *, seed: int | None = None, return_choices: bool = False):
    """`HipCircuit.sample`: see its docstring."""
    return sampler(hc).sample(num_samples, seed, return_choices)


def sample_conditional(hc: "HipCircuit", x: torch.Tensor, sample_vars, *, seed: int | None = None,
                       return_choices: bool = False, return_log_evidence: bool = False, rows_per_chunk: int | None = None):
    """`HipCircuit.sample_conditional`: see its docstring."""
    return sampler(hc).sample_conditional(x, sample_vars, seed, return_choices, return_log_evidence, rows_per_chunk)


class SamplingQuery:
    """Reference-shaped wrapper (cirkit/backend/torch/queries.py:187-275): ``SamplingQuery(circuit)(num_samples)`` returns
    ``(samples, choices)`` -- the samples ``(N, D)`` and the latent choices of the sum-type layers (`HipCircuit.sample`).
    The reference raises on a circuit whose sum weights are not normalised; this one samples ``c(x) / Z`` exactly."""

    def __init__(self, circuit: "HipCircuit") -> None:
        check_plan(circuit.user_plan)
        self._circuit = circuit

    def __call__(self, num_samples: int = 1, *, seed: int | None = None):
        return sample(self._circuit, num_samples, seed=seed, return_choices=True)
