"""The LAYER-WISE reverse launch list of `HipSquaredTrainer` (cirkit_amd/training_squared.py, module docstring): one circuit under
complex-lse-sum or lse-sum -- c on the batch, or the partition function Z on no input -- differentiated layer by layer over the
activations of its last forward.

`_PlanBackward.__init__` decides the KIND of every layer once (and refuses what has no backward here); what a batch size adds --
the gradient arena, the per-layer scratch (`LayerScratch`), the pool of weight gradients -- is a `ReverseState`; scratch
allocation, the pool's layout and the backward launches dispatch on the kind through `_OF_KIND`.  `run` issues calls of the C ABI
only, so the trainer records it into a `ck_program`."""

from __future__ import annotations

import itertools
from dataclasses import dataclass
from typing import Mapping, NamedTuple

import numpy as np
import torch

from . import _capi as capi
from .circuit import HipCircuit
from .circuit_launch import launch_tensordot
from .fusion import tensordot_lists
from .layers import (HipCategoricalLayer, HipConstantValueLayer, HipCPTLayer, HipEmbeddingLayer, HipGaussianLayer, HipHadamardLayer,
                     HipSumLayer, HipTensorDotLayer, HipTuckerLayer)

# serial numbers of the per-batch-size states of c and Z (never repeated): the recorded launch lists of `HipSquaredTrainer` point at
# their buffers and are keyed on them -- a rebuilt state can get its arena back at the old address while its other buffers moved
state_serials = itertools.count(1)
MAX_BOUND = 4  # batch sizes kept per circuit, oldest evicted first

# layer type -> kind; "absorbed" replaces it where the reader's launch does the layer's part (`_PlanBackward.__init__`)
_KIND_OF_TYPE = ((HipTensorDotLayer, "tensordot"), ((HipSumLayer, HipCPTLayer, HipTuckerLayer), "sum"), (HipHadamardLayer, "hadamard"),
                 (HipCategoricalLayer, "categorical"), (HipGaussianLayer, "gaussian"), (HipEmbeddingLayer, "embedding"),
                 (HipConstantValueLayer, "const"))


class _Methods(NamedTuple):
    """The methods of `_PlanBackward` that serve one kind of layer (None: nothing to do)."""
    scratch: str | None  # (i, layer, binding, B) -> the `LayerScratch` of a batch size
    dw_shape: str | None  # (i, layer) -> the shape of the evaluated weights' gradient in the pool
    backward: str | None  # (i, layer, binding, state, B, stream): the backward launches


_OF_KIND = {
    "tensordot": _Methods(None, "_dw_shape_tensordot", "_bwd_tensordot"),
    "sum": _Methods(None, "_dw_shape_sum", "_bwd_sum"),
    "hadamard": _Methods("_scratch_hadamard", None, "_bwd_hadamard"),
    "categorical": _Methods("_scratch_categorical", None, "_bwd_categorical"),
    "gaussian": _Methods("_scratch_gaussian", None, "_bwd_gaussian"),
    "embedding": _Methods("_scratch_embedding", None, "_bwd_embedding"),
    "const": _Methods("_scratch_const", None, "_bwd_const"),
    "absorbed": _Methods(None, "_dw_shape_absorbed", None),
}


def embedding_bwd_fits_lds(num_states: int, K: int) -> bool:
    """Whether `ck_embedding_bwd` holds the (C + 1, K + 1) gradient table of a fold, its counters and its staging in the LDS."""
    words = (num_states + 1) * (K + 1) + 2 * num_states + 3 + 4096
    return words * 4 <= 160 * 1024


@dataclass(slots=True)
class LayerScratch:
    """What the backward of one layer keeps at one batch size (None: this kind has no such buffer)."""
    dw: torch.Tensor | None = None  # the gradient of the evaluated weights: a slice of the pool, or -- `direct` -- of a stored tensor's
    direct: bool | None = None  # (None: a layer without a slice of the pool)
    ro: torch.Tensor | None = None  # Hadamard: the children's offsets in floats
    dtable: torch.Tensor | None = None  # Categorical / Embedding in two launches: the scatter by category
    one_launch: bool = False  # Embedding: `ck_embedding_bwd` does scatter and division
    dm: torch.Tensor | None = None  # Gaussian: d mean, d stddev
    dsd: torch.Tensor | None = None
    gr: torch.Tensor | None = None  # the real parts of a complex gradient block
    gsum: torch.Tensor | None = None  # ConstantValue: the batch sum, the row of ones that takes it, d value
    ones: torch.Tensor | None = None
    dv: torch.Tensor | None = None


@dataclass(slots=True)
class ReverseState:
    """What one batch size adds to a `_PlanBackward`."""
    binding: int  # serial of the circuit's binding the views below point into
    serial: int  # of this state (`state_serials`)
    garena: torch.Tensor  # complex64 / fp32, the mirror of the activation arena
    gviews: list[torch.Tensor]
    scratch: list[LayerScratch]
    pool: torch.Tensor | None = None  # the weight gradients of every sum / TensorDot layer (sized at the first run)


class _PlanBackward:
    """The reverse launch list of ONE layer-wise circuit (complex-lse-sum or lse-sum) over the activations of its last forward.
    Every buffer a launch touches is allocated when a batch size is bound, `run` issues calls of the C ABI only: the list can be
    recorded into a `ck_program` (HipSquaredTrainer does) and holds no tensor-library kernel."""

    def __init__(self, circuit: HipCircuit, grads: Mapping[str, torch.Tensor]) -> None:
        self.c, self.grads = circuit, grads
        self.cplx = circuit.plan.semiring == "complex-lse-sum"
        self.e = 2 if self.cplx else 1  # floats per value
        self._bound: dict[int, ReverseState] = {}
        c = circuit
        if len(c._out_pairs) != 1:
            raise NotImplementedError("training needs a single circuit output")
        po = int(c._out_pairs[0, 0])
        if c.layers[po].num_output_units != 1:
            raise NotImplementedError("training needs a scalar output unit")
        seen: set[tuple[int, int]] = set()
        for ch in c._children:
            if ch is None:
                continue
            for p, f in ch.reshape(-1, 2):
                if (int(p), int(f)) in seen:
                    raise NotImplementedError("squared-circuit training: a fold read by several consumers (gradients are stored, not added)")
                seen.add((int(p), int(f)))
        self.kind = [self._kind_of(spec, l) for spec, l in zip(c.plan.layers, c.layers)]
        # What the TensorDot launches take over (cirkit_amd/fusion.py: Hadamard layers read as lists, the W / conj W pair of
        # TensorDot layers in one launch)
        self.had_of, self.pair_of = tensordot_lists(c.layers, c._children, {po})
        self._pair_first = set(self.pair_of.values())
        self._skip = set(self.had_of.values()) | self._pair_first
        for i in self._skip:
            self.kind[i] = "absorbed"

    def _kind_of(self, spec, l) -> str:
        """The kind of a layer by its type; raises for what the list cannot differentiate."""
        kind = next((k for types, k in _KIND_OF_TYPE if isinstance(l, types)), None)
        if kind is None:
            raise NotImplementedError(f"squared-circuit training: layer type {spec.type!r}")
        if kind == "sum" and getattr(l, "_mixing", False):
            raise NotImplementedError("squared-circuit training: mixing layers")
        if kind == "categorical" and (self.cplx or l.probs is None or l.probs.softmax_source() is None):
            raise NotImplementedError("squared-circuit training: Categorical layers need lse-sum and probs = softmax(tensor)")
        if kind == "gaussian" and (self.cplx or l.log_partition is not None):
            raise NotImplementedError("squared-circuit training: Gaussian layers need lse-sum and no log-partition parameter")
        return kind

    @staticmethod
    def _need_real(t: torch.Tensor, what: str = "complex-valued weights") -> None:
        if t.is_complex():
            raise NotImplementedError(f"squared-circuit training: {what}")

    # ---- what a batch size adds -----------------------------------------------------------------------------------------------
    def bind(self, B: int) -> ReverseState:
        bd = self.c._bind(B)
        st = self._bound.get(B)
        if st is not None and st.binding == bd.serial:
            return st
        garena = torch.zeros_like(bd.arena)
        gviews = []
        for i, l in enumerate(self.c.layers):
            off = (bd.views[i].data_ptr() - bd.arena.data_ptr()) // bd.arena.element_size()
            gviews.append(garena[off : off + l.num_folds * B * l.num_output_units].view(l.num_folds, B, l.num_output_units))
        # per layer: the scratch of its backward, by its kind (the weight gradients join it at the first run: `_weight_pool`)
        scratch = []
        for i, l in enumerate(self.c.layers):
            make = _OF_KIND[self.kind[i]].scratch
            scratch.append(LayerScratch() if make is None else getattr(self, make)(i, l, bd, B))
        st = ReverseState(binding=bd.serial, serial=next(state_serials), garena=garena, gviews=gviews, scratch=scratch)
        self._bound.pop(B, None)
        while len(self._bound) >= MAX_BOUND:
            self._bound.pop(next(iter(self._bound)))
        self._bound[B] = st
        return st

    def _f32(self, *shape) -> torch.Tensor:
        return torch.zeros(shape, dtype=torch.float32, device=self.c.device)

    def _scratch_hadamard(self, i: int, l, bd, B: int) -> LayerScratch:
        return LayerScratch(ro=(bd.row_off[i] * self.e).contiguous())

    def _scratch_categorical(self, i: int, l, bd, B: int) -> LayerScratch:
        return LayerScratch(dtable=self._f32(l.num_folds, l.num_categories + 1, l.num_output_units))

    def _scratch_gaussian(self, i: int, l, bd, B: int) -> LayerScratch:
        return LayerScratch(dm=self._f32(l.num_folds, l.num_output_units), dsd=self._f32(l.num_folds, l.num_output_units))

    def _scratch_embedding(self, i: int, l, bd, B: int) -> LayerScratch:
        F, K = l.num_folds, l.num_output_units
        sc = LayerScratch(dw=self._f32(F, K, l.num_states), one_launch=K % 32 == 0 and embedding_bwd_fits_lds(l.num_states, K))
        if not sc.one_launch:
            sc.dtable = self._f32(F, l.num_states + 1, K)
            if self.cplx:
                sc.gr = self._f32(F, B, K)
        return sc

    def _scratch_const(self, i: int, l, bd, B: int) -> LayerScratch:
        F, K = l.num_folds, l.num_output_units
        sc = LayerScratch()
        if self.cplx or B > 1:
            sc.gsum = self._f32(F, K)
        if B > 1:
            sc.ones = torch.ones((F, 1, B), dtype=torch.float32, device=self.c.device)
            if self.cplx:
                sc.gr = self._f32(F, B, K)
        if not l.log_space:
            sc.dv = self._f32(F, K)
        return sc

    # ---- the pool of weight gradients -----------------------------------------------------------------------------------------
    def _dw_shape_tensordot(self, i: int, l) -> tuple:
        return (l.num_folds, l.num_output_units // l._num_batch_units, l._num_contract_units)

    def _dw_shape_sum(self, i: int, l) -> tuple:
        return tuple(l._w.shape)

    def _dw_shape_absorbed(self, i: int, l) -> tuple | None:
        return self._dw_shape_tensordot(i, l) if i in self._pair_first else None  # (an absorbed Hadamard layer has no weights)

    def _weight_pool(self, st: ReverseState) -> torch.Tensor:
        """The gradients of the evaluated weights of every sum / TensorDot layer as slices of ONE buffer (the kernels add into
        them with atomics: one fill per step zeroes them all); sized at the first run, when the forward has evaluated the weights."""
        if st.pool is None:
            shapes, off = {}, 0
            for i, l in enumerate(self.c.layers):
                shape_of = _OF_KIND[self.kind[i]].dw_shape
                shape = None if shape_of is None else getattr(self, shape_of)(i, l)
                if shape is None:
                    continue
                sc = st.scratch[i]
                # a weight that IS a stored tensor (a pointer, through conjugates): the kernel adds into that tensor's gradient
                name = l.weight.passthrough_tensor()
                if name is not None and self.grads[name].numel() == int(np.prod(shape)) and self.grads[name].is_contiguous():
                    sc.dw, sc.direct = self.grads[name].view(shape), True
                    continue
                shapes[i] = (off, shape)
                off += (int(np.prod(shape)) + 3) // 4 * 4
            pool = torch.zeros(max(off, 4), dtype=torch.float32, device=st.garena.device)
            for i, (o, shape) in shapes.items():
                st.scratch[i].dw, st.scratch[i].direct = pool[o : o + int(np.prod(shape))].view(shape), False
            st.pool = pool
        return st.pool

    def zero_pool(self, B: int, stream: int) -> None:
        """Zero the weight-gradient pool of this binding (what `run(..., pool_zeroed=True)` then adds into)."""
        pool = self._weight_pool(self.bind(B))
        capi.call("ck_fill_f32", pool.data_ptr(), pool.numel(), 0.0, stream)

    # ---- the forward of a circuit without input ---------------------------------------------------------------------------------
    def forward(self, B: int, stream: int) -> None:
        """The layer launches of a circuit WITHOUT input variables (the partition function: `HipCircuit._enqueue_layers` with the
        Hadamard layers read as lists and the TensorDot pairs in one launch each); the parameters must have been evaluated."""
        c = self.c
        if c.plan.num_variables:
            raise NotImplementedError("_PlanBackward.forward: circuits with input variables go through HipCircuit")
        bd = c._bind(B)
        for i, l in enumerate(c.layers):
            kind = self.kind[i]
            if kind == "tensordot":
                self._need_real(l._w)
                launch_tensordot(c.layers, i, bd, self.had_of, self.pair_of, self.cplx, stream)
            elif kind == "const":
                l.launch_const(bd.views[i], B, stream)
            elif kind != "absorbed":
                l.launch(bd.arena, bd.row_off[i], bd.views[i], B, stream)

    # ---- the backward ---------------------------------------------------------------------------------------------------------
    def run(self, B: int, seed_real: float, stream: int, pool_zeroed: bool = False) -> None:
        """Gradients of ``seed_real * sum_b Re out_b`` w.r.t. the parameter tensors, ADDED into `grads`."""
        c = self.c
        bd, st = c._bind(B), self.bind(B)
        po, fo = int(c._out_pairs[0, 0]), int(c._out_pairs[0, 1])
        # the output layer's gradient: filled on every run, so a recorded list carries the seed of its own (B, global batch) key --
        # lists of several keys share this block (c at one B with two global batches; Z, whose B = 1, under any B / global batch)
        capi.call("ck_fill_f32", st.gviews[po].data_ptr(), st.gviews[po].numel() * self.e, 0.0, stream)
        capi.call("ck_fill_strided_f32", st.gviews[po][fo].data_ptr(), B, self.e, float(seed_real), stream)  # (Re = seed, Im = 0)
        pool = self._weight_pool(st)
        if not pool_zeroed:
            capi.call("ck_fill_f32", pool.data_ptr(), pool.numel(), 0.0, stream)
        for i in range(len(c.layers) - 1, -1, -1):
            bwd = _OF_KIND[self.kind[i]].backward
            if bwd is not None:  # (None: its reader's launch did its part -- an absorbed Hadamard layer, the first half of a pair)
                getattr(self, bwd)(i, c.layers[i], bd, st, B, stream)

    def _weight_backward(self, l, sc: LayerScratch, stream: int) -> None:
        if not sc.direct:
            l.weight.backward(sc.dw, self.grads, stream)

    def _real_part(self, g: torch.Tensor, sc: LayerScratch, stream: int) -> torch.Tensor:
        """(F, B, K) fp32: the real parts of a gradient block."""
        if not self.cplx:
            return g
        capi.call("ck_copy_strided_f32", g.data_ptr(), sc.gr.data_ptr(), g.numel(), 2, 1, stream)
        return sc.gr

    def _td_args(self, i: int, bd):
        """(row offsets, list length) of TensorDot layer i's input: its own block, or the children of the Hadamard layer it absorbs."""
        h = self.had_of.get(i)
        return (bd.row_off[i].data_ptr(), 1) if h is None else (bd.row_off[h].data_ptr(), self.c.layers[h].arity)

    def _bwd_tensordot(self, i: int, l, bd, st: ReverseState, B: int, stream: int) -> None:
        """(optimized.py:289-296) on its own layout: x (B, Kj, Kq) -> out (B, Kq, Kk); with the TensorDot layer beneath it where
        the forward took the pair in one launch."""
        self._need_real(l._w)
        g, sc = st.gviews[i], st.scratch[i]
        F, K = l.num_folds, l.num_output_units
        aa, ga, cv = bd.arena.data_ptr(), st.garena.data_ptr(), 1 if self.cplx else 0
        a = self.pair_of.get(i)
        if a is None:
            ro, H = self._td_args(i, bd)
            capi.call("ck_tensordot_lse_bwd", aa, ga, ro, H, l._w.data_ptr(), bd.views[i].data_ptr(), g.data_ptr(), sc.dw.data_ptr(),
                      F, B, l._num_contract_units, l._num_batch_units, K // l._num_batch_units, cv, stream)
        else:
            la, sa = self.c.layers[a], st.scratch[a]
            self._need_real(la._w)
            ro, H = self._td_args(a, bd)
            capi.call("ck_tensordot2_lse_bwd", aa, ga, ro, H, la._w.data_ptr(), bd.views[a].data_ptr(), st.gviews[a].data_ptr(),
                      l._w.data_ptr(), bd.views[i].data_ptr(), g.data_ptr(), sa.dw.data_ptr(), sc.dw.data_ptr(), F, B,
                      la._num_contract_units, la._num_batch_units, la.num_output_units // la._num_batch_units, K // l._num_batch_units,
                      cv, stream)
            self._weight_backward(la, sa, stream)
        self._weight_backward(l, sc, stream)

    def _bwd_sum(self, i: int, l, bd, st: ReverseState, B: int, stream: int) -> None:
        self._need_real(l._w)
        sc = st.scratch[i]
        head = (bd.arena.data_ptr(), st.garena.data_ptr(), bd.row_off[i].data_ptr())
        tail = (l._w.data_ptr(), bd.views[i].data_ptr(), st.gviews[i].data_ptr(), sc.dw.data_ptr(), l.num_folds, l.arity, B,
                l.num_input_units, l.num_output_units, l._mode, 0, stream)
        if self.cplx:
            capi.call("ck_sum_lse_bwd_c", *head, *tail)
        else:
            capi.call("ck_sum_lse_bwd", *head, None, *tail)
        self._weight_backward(l, sc, stream)

    def _bwd_hadamard(self, i: int, l, bd, st: ReverseState, B: int, stream: int) -> None:
        """Log space: the sum of the children -- (re, im) pairs as 2 K floats."""
        capi.call("ck_hadamard_bwd", st.garena.data_ptr(), st.scratch[i].ro.data_ptr(), st.gviews[i].data_ptr(), l.num_folds, l.arity, B,
                  self.e * l.num_output_units, 0, stream)

    def _bwd_categorical(self, i: int, l, bd, st: ReverseState, B: int, stream: int) -> None:
        """(lse-sum) the scatter-add into the log-table, then log softmax backward."""
        g, dtable = st.gviews[i], st.scratch[i].dtable
        F, K, Cn = l.num_folds, l.num_output_units, l.num_categories
        capi.call("ck_categorical_bwd", g.data_ptr(), None, bd.xt_i.data_ptr(), l._scope(g.device).data_ptr(), dtable.data_ptr(),
                  F, B, K, Cn, 0, None, stream)
        name = l.probs.graph.nodes[0].config["tensor"]
        capi.call("ck_param_log_table_bwd", l._table.data_ptr(), dtable.data_ptr(), self.grads[name].data_ptr(), F, K, Cn, 1, stream)

    def _bwd_gaussian(self, i: int, l, bd, st: ReverseState, B: int, stream: int) -> None:
        """(lse-sum) batch sums of d log N / d mean, d log N / d stddev."""
        g, sc = st.gviews[i], st.scratch[i]
        mean, stddev, _ = l._vals
        capi.call("ck_gaussian_bwd", g.data_ptr(), bd.xt.data_ptr(), l._scope(g.device).data_ptr(), mean.data_ptr(), stddev.data_ptr(),
                  sc.dm.data_ptr(), sc.dsd.data_ptr(), l.num_folds, B, l.num_output_units, stream)
        l.mean.backward(sc.dm.view(mean.shape), self.grads, stream)
        l.stddev.backward(sc.dsd.view(stddev.shape), self.grads, stream)

    def _bwd_embedding(self, i: int, l, bd, st: ReverseState, B: int, stream: int) -> None:
        """out = log(w[f, :, x]): the scatter-add of Re(gout) over the batch, divided by w."""
        self._need_real(l._table, "complex Embedding weights (the layer-level autograd of cirkit_amd.layer_ops.embedding differentiates them)")
        g, sc = st.gviews[i], st.scratch[i]
        F, K, Cn = l.num_folds, l.num_output_units, l.num_states
        if sc.one_launch:
            capi.call("ck_embedding_bwd", g.data_ptr(), self.e, None, None, bd.xt_i.data_ptr(), l._scope(g.device).data_ptr(),
                      l._table.data_ptr(), sc.dw.data_ptr(), F, B, K, Cn, stream)
        else:
            gr = self._real_part(g, sc, stream)
            capi.call("ck_categorical_bwd", gr.data_ptr(), None, bd.xt_i.data_ptr(), l._scope(gr.device).data_ptr(),
                      sc.dtable.data_ptr(), F, B, K, Cn, 0, None, stream)
            capi.call("ck_embedding_weight_bwd", l._table.data_ptr(), sc.dtable.data_ptr(), sc.dw.data_ptr(), F, Cn, K, stream)
        l.weight.backward(sc.dw, self.grads, stream)

    def _bwd_const(self, i: int, l, bd, st: ReverseState, B: int, stream: int) -> None:
        """The batch sum of the gradient block (+ d log v / dv for a value kept in linear space)."""
        v = l._val
        self._need_real(v, "complex constant values")
        g, sc = st.gviews[i], st.scratch[i]
        F, K = l.num_folds, l.num_output_units
        if B == 1:
            if self.cplx:
                capi.call("ck_copy_strided_f32", g.data_ptr(), sc.gsum.data_ptr(), F * K, 2, 1, stream)
                gsum = sc.gsum
            else:
                gsum = g.view(F, K)
        else:  # the batch sum as a product with a row of ones
            gr = self._real_part(g, sc, stream)
            gsum = sc.gsum
            capi.call("ck_param_bmm", sc.ones.data_ptr(), gr.data_ptr(), gsum.data_ptr(), F, 1, K, B, 0, 0, 0, stream)
        if l.log_space:
            dv = gsum
        else:
            dv = sc.dv
            capi.call("ck_param_unary_bwd", capi.CK_UNARY_LOG, v.data_ptr(), v.data_ptr(), gsum.data_ptr(), dv.data_ptr(), F * K, 0, stream)
        l.value.backward(dv.view(v.shape), self.grads, stream)
