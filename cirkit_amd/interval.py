"""Interval (box) evidence on the GPU: `HipCircuit.interval_log_prob` and `HipCircuit.log_cdf` (DESIGN.md section 11,
"Interval evidence").

A smooth, decomposable circuit integrates exactly over any product of per-variable sets in one bottom-up pass: every input
unit emits the mass of its own set and the inner layers do not change.  Here the sets are closed intervals, one per row and
variable.  The pass runs on the layer-wise circuit the other queries use (`Sampler._z_circuit()`): per chunk of rows the two
bound tensors are staged once with the contract's clamping and sentinel rules (`ck_interval_stage`), the interval kernels
write the input layers' arena views (`ck_categorical_interval_fwd`, `ck_gaussian_interval_fwd`), and every other layer is
launched exactly as the forward launches it.  The reference's ``IntegrateQuery`` (queries.py:19-184) knows two states per
variable, observed and integrated; both are special cases here.  Kernels: cirkit_amd/csrc/ck_interval.hip.
"""

from __future__ import annotations

from typing import TYPE_CHECKING

import torch

from . import _capi as capi
from .layers import HipCategoricalLayer, HipConstantValueLayer, HipGaussianLayer, HipInputLayer
from .plan import Plan
from .sampling import _REFUSED, Sampler, chunk_rows, sampler

if TYPE_CHECKING:  # pragma: no cover
    from .circuit import HipCircuit

_BLOCK = 16  # states per block of the side tables (kBlk of ck_interval.hip)


def check_plan(plan: Plan) -> None:
    """Refuse, before anything is launched, what has no interval evidence: a plan that is not a real lse-sum circuit
    (``ValueError``, checked first), a layer without an integral over a set (``TypeError`` naming it), an input layer that
    cannot integrate (``NotImplementedError``)."""
    if plan.semiring != "lse-sum":
        raise ValueError(f"interval evidence needs a real circuit in the lse-sum semiring, this plan is {plan.semiring!r}")
    for i, l in enumerate(plan.layers):
        if l.type in _REFUSED:
            raise TypeError(f"Interval evidence is not supported for layers of type {_REFUSED[l.type]} (layer {i})")
        if l.inputs is None and l.type not in ("categorical", "binomial", "gaussian"):
            raise NotImplementedError(f"interval evidence through an input layer of type {l.type!r} (layer {i}): it cannot integrate")


class IntervalState:
    """The interval-evidence state of one `HipCircuit`, next to its `Sampler`: the block-sum side tables of the last
    parameter state and the staged bounds of the bound chunk sizes."""

    def __init__(self, s: Sampler) -> None:
        self.s = s
        self._key = None
        self._side: dict[int, torch.Tensor] = {}  # discrete input layer -> (F, ceil(C / 16), 2, K) block sums
        self._staged: dict[int, tuple] = {}  # chunk rows -> (lo_i, hi_i, lo_f, hi_f), each (D, rows) or None

    # -- refusals and argument errors: nothing is copied, prepared or launched before them -------------------------------
    def check_bounds(self, lo, hi) -> None:
        D = self.s.D
        for t in (lo, hi):
            if not isinstance(t, torch.Tensor) or t.dim() != 2:
                raise ValueError("The bounds of the circuit's variables should have shape (B, D), where B is the batch size and D "
                                 "is the number of variables the circuit is defined on")
        if lo.dtype != hi.dtype:
            raise ValueError(f"lo and hi must have the same dtype, found {lo.dtype} and {hi.dtype}")
        if lo.dtype == torch.bool or lo.is_complex():
            raise ValueError(f"the bounds must be integers or floating-point numbers, found {lo.dtype}")
        if lo.shape[0] != hi.shape[0]:
            raise ValueError(f"lo has {lo.shape[0]} rows and hi {hi.shape[0]}")
        if lo.shape[1] < D or hi.shape[1] < D:
            raise ValueError(f"expected at least {D} variables, found {min(lo.shape[1], hi.shape[1])}")
        if lo.shape[0] <= 0:
            raise ValueError("empty batch")

    def _integration_mask(self, B: int, integrate_vars) -> torch.Tensor:
        """The (B, D) / (1, D) bool mask of `forward`'s ``integrate_vars``, with its forms and errors."""
        hc, dev = self.s.hc, self.s.device
        zero = torch.zeros((B, self.s.D), dtype=torch.float32 if hc._float_input else torch.int64, device=dev)
        marked = hc._apply_integration_mask(zero, integrate_vars)
        return torch.isnan(marked) if hc._float_input else marked < 0

    # -- once per parameter state ----------------------------------------------------------------------------------------
    def tables(self, stream: int) -> None:
        """The layer-wise circuit's derived parameters and, from its log tables, the block sums of every discrete input
        layer, for the store's current values; a no-op when nothing changed since the last call."""
        st = self.s.store
        key = (st.version, st.state(), st.raw_writes)
        if key == self._key:
            return
        zc = self.s._z_circuit()
        zc._enqueue_params(stream)
        for j, l in enumerate(zc.layers):
            if not isinstance(l, HipCategoricalLayer):
                continue
            F, K, C = l.num_folds, l.num_output_units, l.num_categories
            shape = (F, (C + _BLOCK - 1) // _BLOCK, 2, K)
            side = self._side.get(j)
            if side is None or tuple(side.shape) != shape:
                side = self._side[j] = torch.empty(shape, dtype=torch.float32, device=self.s.device)
            capi.call("ck_interval_block_sums", l._table.data_ptr(), side.data_ptr(), F, C, K, stream)
        self._key = key

    # -- per chunk -----------------------------------------------------------------------------------------------------------
    def _staging(self, nb: int, want_int: bool, want_float: bool) -> tuple:
        hit = self._staged.get(nb)
        if hit is None:
            dev, D = self.s.device, self.s.D
            mk = lambda dt: (torch.empty((D, nb), dtype=dt, device=dev), torch.empty((D, nb), dtype=dt, device=dev))  # noqa: E731
            hit = self._staged[nb] = (mk(torch.int32) if want_int else (None, None)) + (mk(torch.float32) if want_float else (None, None))
        return hit

    def leaves(self, bd, lo: torch.Tensor, hi: torch.Tensor, stream: int) -> int:
        """Stage a chunk's bounds and launch the interval kernel of every input layer into its arena view of binding `bd`;
        returns the number of launches."""
        zc = self.s._z_circuit()
        nb, D = bd.B, self.s.D
        lo_i, hi_i, lo_f, hi_f = self._staging(nb, zc._int_input, zc._float_input)
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        capi.call("ck_interval_stage", lo.data_ptr(), hi.data_ptr(), 1 if lo.is_floating_point() else 0, nb, D,
                  zc._num_states_dev().data_ptr(), ptr(lo_i), ptr(hi_i), ptr(lo_f), ptr(hi_f), stream)
        n = 1
        for j, (l, view) in enumerate(zip(zc.layers, bd.views)):
            if not isinstance(l, HipInputLayer):
                continue
            scope = l._scope(self.s.device).data_ptr()
            if isinstance(l, HipGaussianLayer):
                mean, stddev, lz = l._vals
                capi.call("ck_gaussian_interval_fwd", mean.data_ptr(), stddev.data_ptr(), ptr(lz), lo_f.data_ptr(), hi_f.data_ptr(),
                          scope, view.data_ptr(), l.num_folds, nb, l.num_output_units, D, stream)
            else:
                capi.call("ck_categorical_interval_fwd", l._table.data_ptr(), self._side[j].data_ptr(), lo_i.data_ptr(),
                          hi_i.data_ptr(), scope, view.data_ptr(), l.num_folds, nb, l.num_output_units, l.num_categories, D, stream)
            n += 1
        return n

    # -- once per call -------------------------------------------------------------------------------------------------------
    def bounds(self, lo: torch.Tensor, hi: torch.Tensor, integrate_vars) -> tuple[torch.Tensor, torch.Tensor]:
        """The checked bounds on the device, cut to the circuit's variables, in the dtype the staging reads (int64, or fp32
        when the circuit has a Gaussian layer or the bounds are floating point), the variables `integrate_vars` marks set
        to the sentinel in both."""
        s = self.s
        self.check_bounds(lo, hi)
        mask = None if integrate_vars is None else self._integration_mask(int(lo.shape[0]), integrate_vars)
        as_float = s.hc._float_input or lo.is_floating_point()
        dt = torch.float32 if as_float else torch.int64
        sentinel = torch.full((), float("nan") if as_float else -1, dtype=dt, device=s.device)
        out = []
        for t in (lo, hi):
            t = t[:, : s.D].to(s.device).to(dt)
            out.append((t if mask is None else torch.where(mask, sentinel, t)).contiguous())
        return out[0], out[1]

    def interval_log_prob(self, lo: torch.Tensor, hi: torch.Tensor, integrate_vars=None, rows_per_chunk: int | None = None):
        s = self.s
        hc = s.hc
        lo, hi = self.bounds(lo, hi, integrate_vars)
        B = int(lo.shape[0])
        chunks = chunk_rows(B, rows_per_chunk, hc.arena_bytes(1))
        sizes = {nb for _, nb in chunks}
        zc = s._z_circuit()
        for b in [b for b in zc._bindings if b != 1 and b not in sizes]:  # two batch sizes bound: the chunk and the tail
            zc._bindings.pop(b).destroy()
            s._val_off.pop(b, None)
        for b in [b for b in self._staged if b not in sizes]:
            del self._staged[b]
        pairs = zc._out_pairs
        K = zc.layers[int(pairs[0, 0])].num_output_units
        if hc._pad_info is not None:
            K = min(K, hc._pad_info.out_units)
        dev = s.device
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            out = torch.empty((B, len(pairs), K), dtype=torch.float32, device=dev)
            for nb in sizes:
                zc._bind(nb)
            self.tables(stream)
            for r0, nb in chunks:
                bd = zc._bind(nb)
                self.leaves(bd, lo[r0 : r0 + nb], hi[r0 : r0 + nb], stream)
                zc._enqueue_layers(bd, stream, inputs=False)
                for o, (p, f) in enumerate(pairs):
                    out[r0 : r0 + nb, o].copy_(bd.views[int(p)][int(f)][:, :K])
        return out


def _state(hc: "HipCircuit") -> IntervalState:
    check_plan(hc.user_plan)
    for l in hc.layers:
        if isinstance(l, HipInputLayer) and not isinstance(l, HipConstantValueLayer) and not l.can_integrate:
            raise NotImplementedError(f"interval evidence through {type(l).__name__}: it cannot integrate")
    s = sampler(hc)
    if s._interval is None:
        s._interval = IntervalState(s)
    return s._interval


def interval_log_prob(hc: "HipCircuit", lo: torch.Tensor, hi: torch.Tensor, *, integrate_vars=None,
                      rows_per_chunk: int | None = None):
    """`HipCircuit.interval_log_prob`: see its docstring."""
    return _state(hc).interval_log_prob(lo, hi, integrate_vars, rows_per_chunk)


def log_cdf(hc: "HipCircuit", x: torch.Tensor, *, integrate_vars=None, rows_per_chunk: int | None = None):
    """`HipCircuit.log_cdf`: see its docstring."""
    if not isinstance(x, torch.Tensor):
        raise ValueError("The input to the circuit should have shape (B, D)")
    lo = torch.full_like(x, float("-inf")) if x.is_floating_point() else torch.zeros_like(x)
    return interval_log_prob(hc, lo, x, integrate_vars=integrate_vars, rows_per_chunk=rows_per_chunk)
