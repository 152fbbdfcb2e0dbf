"""Training step on the HIP backend: forward, backward, optimiser -- SURVEY.md section 8 (f3).

The reference trains with autograd through its torch forward (notebooks/learning-a-circuit.ipynb,
cell 18: ``loss = -torch.mean(circuit(batch)); loss.backward(); optimizer.step()``).  Two forms here:

* FUSED (cirkit_amd/train_fused.py; circuits whose leaf region is one persistent launch -- Categorical -> dense -> 2 or 4 CP-T levels, BASELINE
  configs 2 / 3 -- `HipTrainer(fused=None)` picks it when it applies): the forward is the fused inference forward that also
  keeps the linear tile of every node of the leaf region (`ck_leaf_walk_fwd` keep_levels) and the outputs of the tail; the
  backward walks the tail layer by layer, then the leaf region two levels per launch on those tiles (`ck_leaf_walk_bwd`:
  no layer gradient is materialised above the leaves), scatters the leaf gradients into the (F, C + 1, 32) table by
  category, and pushes the table gradient through the dense layer and the Categorical log-softmax ON THE TABLE (C + 1
  rows per fold, like `dense_on_table` in the forward);
* LAYER-WISE (everything else, and the checker of the fused form): the forward with every layer output kept in the arena,
  then a reverse launch list of hand-written kernels (cirkit_amd/csrc/ck_backward.hip) over the plan.

Data-parallel training = one process per GPU, the batch sharded, and ONE all-reduce of a
single flat gradient buffer (all parameter gradients are views of it) over RCCL/xGMI per step.

Covered: real lse-sum circuits made of Categorical (probs = softmax) or Gaussian inputs, Sum / CP-T /
Tucker layers (softmax, raw, or any parameter graph `HipParameter.backward` handles, e.g. the MatMul weight
of a collapsed Sum -> Sum pair), mixing layers, Hadamard and Kronecker layers -- what the image / tabular
templates build with 'cp', 'cp-t' and 'tucker' (BASELINE configs 1-4, the reference's Tucker notebook).  Other layers
(TensorDot, the complex semiring) raise NotImplementedError.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import TYPE_CHECKING, Mapping

import numpy as np
import torch

from .distributed import world_size as _world_size
from . import _capi as capi
from .circuit import HipCircuit
from .layers import (HipCategoricalLayer, HipCPTLayer, HipGaussianLayer, HipHadamardLayer, HipKroneckerLayer, HipSumLayer,
                     HipTuckerLayer)
from .plan import Plan, resolve_fold_index
from .train_state import DeviceOptState, FlatBuffers, TrainerSurface

if TYPE_CHECKING:
    from .train_fused import FusedBinding


@dataclass(slots=True)
class SharedChildren:
    """A layer whose folds share children: its backward writes one block per (fold, slot) to the binding's temporary, and
    `ck_segment_add_rows` adds the blocks of every distinct child into the gradient arena."""
    row_off: torch.Tensor  # the (fold, slot) blocks of the temporary, as element offsets
    cptr: torch.Tensor  # per distinct child: where its (fold, slot) list starts in `clist`
    clist: torch.Tensor
    coff: torch.Tensor  # per distinct child: its element offset in the arena
    n_child: int
    block: int


@dataclass(slots=True)
class BackwardBinding:
    """What the backward holds for one batch size, over the circuit's forward binding `bd` of that size; rebuilt when the
    circuit's arena moves (`arena_ptr`), together with everything that points into it -- the fused form's part included."""
    arena_ptr: int
    garena: torch.Tensor  # the gradient of every materialised layer output, at the output's offset in the arena
    gviews: list  # per layer: its (F, B, K) view of `garena`, None where the output is never materialised
    flags: dict[int, int]  # `HipTrainer._accumulate_flags`
    need_zero: set[int]
    dws: dict  # linear-space weight / table gradients: views of `dw_flat`
    dw_flat: torch.Tensor
    shared: dict[int, SharedChildren]
    tmp: torch.Tensor
    fused: FusedBinding | None = None  # cirkit_amd/train_fused.py

    def target(self, i: int, bd) -> tuple[int, int, int]:
        """(gradient arena, child offsets, accumulate flag) of layer i's backward launch."""
        sh = self.shared.get(i)
        if sh is None:
            return self.garena.data_ptr(), bd.row_off[i].data_ptr(), self.flags[i]
        return self.tmp.data_ptr(), sh.row_off.data_ptr(), 0

    def gather_shared(self, i: int, stream: int) -> None:
        """After layer i's backward launch: its shared children's gradients from the temporary into the arena."""
        sh = self.shared.get(i)
        if sh is not None:
            capi.call("ck_segment_add_rows", self.tmp.data_ptr(), sh.cptr.data_ptr(), sh.clist.data_ptr(),
                      sh.coff.data_ptr(), self.garena.data_ptr(), sh.n_child, sh.block, stream)


class HipTrainer(TrainerSurface):
    """Maximum-likelihood training of a plan's parameters: ``loss = -mean_b log p(x_b)``."""

    def __init__(
        self,
        plan: Plan,
        tensors: Mapping[str, object],
        *,
        device: str | torch.device = "cuda:0",
        lr: float = 0.01,
        optimizer: str = "adam",
        betas: tuple[float, float] = (0.9, 0.999),
        eps: float = 1e-8,
        pad_units: bool = False,
        fused: bool | None = None,
        jobs: bool | None = None,
        fuse_optimizer: bool = True,
    ) -> None:
        """`pad_units`: train the plan with its unit counts padded to multiples of 32 (cirkit_amd/padding.py), so that
        the MFMA forward / backward tiles apply to any width.  The padded entries never receive a gradient (softmax
        at a -inf logit, zero weight on every padded unit), so the padded circuit stays the same function; `self.grads`
        and the parameter store then hold the PADDED tensors -- `gradients()` / `parameters()` return user shapes.
        `fused`: None takes the fused forward / backward when the plan qualifies (module docstring), True insists
        (NotImplementedError says why not), False forces the layer-wise form.
        `jobs`: circuits of 64-unit dense / CP-T / mixing / Hadamard layers (the reference's learning notebook, BASELINE config 4)
        step as level launches over jobs (cirkit_amd/train_jobs.py) when the fused form does not apply: None where the plan
        qualifies, True insists, False never.  `fuse_optimizer` (fused and job forms, one rank): `step` runs the optimizer inside the backward
        epilogues -- the workgroup that holds a weight's gradient updates its logits and moments and writes the next step's
        softmax; no gradient, no normalised weight and no optimizer launch for those tensors (`loss_and_grads` still leaves
        every gradient in `grads`)."""
        if plan.semiring != "lse-sum":
            raise NotImplementedError("HipTrainer trains circuits under the real lse-sum semiring; squared circuits compiled under "
                                      "complex-lse-sum (Embedding / CP-T for c, ConstantValue / Hadamard / TensorDot for Z) train with "
                                      "cirkit_amd.training_squared.HipSquaredTrainer")
        if optimizer not in ("adam", "sgd"):
            raise ValueError(f"unknown optimizer {optimizer!r}")
        self.user_plan, self._pad_info = plan, None
        if pad_units:
            plan, tensors = self._pad(plan, tensors)
        # parameters, gradients and moments: one flat buffer each (cirkit_amd/train_state.py); `grads` are views
        fb = FlatBuffers(plan.tensors, tensors, device, optimizer)
        self._flat_param, self._flat_grad, self._m1, self._m2, self._moments = fb.param, fb.grad, fb.m1, fb.m2, fb.moments
        self.plan, self.grads = plan, fb.grads
        self._fuse_optimizer = bool(fuse_optimizer)
        # the DEVICE ck_opt_state of the optimizer epilogues (fused form) or job epilogues (job form: the two exclude each other)
        self._opt = DeviceOptState(device)
        self._choose_circuit(fb.store, device, fused)
        self.device = self.circuit.device
        self.lr, self.optimizer, self.betas, self.eps = lr, optimizer, betas, eps
        self.step_count = 0
        self._clock: str | None = None  # which optimizer clock has advanced: "device" (fused job step) | "host" (apply_gradients)
        self._grads_current = False  # `grads` holds the gradients of the last step (false after a fused job step)
        if len(self.circuit._out_pairs) != 1:
            raise NotImplementedError("training needs a single circuit output")
        if not self.fused:
            self._check_supported()
        self._bwd: dict[int, BackwardBinding] = {}
        # input validation: the circuit's flag is raised by a batch with an out-of-range category; a step on such a batch
        # changes nothing (`step`), the flag is latched into `_bad_seen` -- what `check_inputs()` reports -- and cleared
        self._bad_seen = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._step_flag = torch.zeros(1, dtype=torch.int32, device=self.device)  # fused: the flag of the step being taken
        self._skipped = torch.zeros(1, dtype=torch.int32, device=self.device)  # Adam steps that did not count
        self._choose_jobs(jobs)

    def _pad(self, plan: Plan, tensors: Mapping[str, object]):
        """(plan, tensors) with the unit counts padded to multiples of 32 -- as they are when nothing needs padding."""
        from . import padding

        res = padding.pad_units(plan)
        if res is None:
            return plan, tensors
        plan, self._pad_info = res
        host = {n: (tensors[n].detach().cpu().numpy() if hasattr(tensors[n], "detach") else np.asarray(tensors[n]))
                for n in self.user_plan.tensors}
        return plan, padding.pad_tensors(self._pad_info, host)

    def _choose_circuit(self, store, device, fused: bool | None) -> None:
        """The fused form (cirkit_amd/train_fused.py) where it applies and is not declined, else the layer-wise circuit."""
        self.fused, self._fused_step = False, None
        why = "fused=False"
        if fused is not False:
            from .train_fused import FusedStep

            fs = FusedStep(self, store, device)
            why = fs.why
        if why is None:
            self.circuit, self.fused, self._fused_step = fs.circuit, True, fs
            return
        if fused is True:
            raise NotImplementedError(f"fused training does not apply to this plan: {why}")
        # layer-wise forward, every activation materialised, row-major linear weights
        self.circuit = HipCircuit(self.plan, store, device=device, use_graph=False, fuse=False,
                                  batch_params=True, tiled_weights=False, dense_on_table=False, pad_units=False,
                                  fused_weight_softmax=False)

    def _choose_jobs(self, jobs: bool | None) -> None:
        """The job form (cirkit_amd/train_jobs.py) where the fused form does not apply and the plan qualifies."""
        self._jobs = None
        if not self.fused and jobs is not False and self._pad_info is None:
            from .train_jobs import JobStep

            js = JobStep(self)
            if js.why is None:
                self._jobs = js
            elif jobs is True:
                raise NotImplementedError(f"the job form of the training step does not apply to this plan: {js.why}")
        elif jobs is True:
            raise NotImplementedError("the job form of the training step needs an unpadded plan outside the fused form")

    # ------------------------------------------------------------------------------------------
    _PARAM_OPS = {"tensor", "softmax", "log_softmax", "sigmoid", "exp", "log", "square", "clamp", "softplus", "scaled_sigmoid", "mixing_weight", "matmul"}

    def _check_supported(self) -> None:
        for spec, l in zip(self.plan.layers, self.circuit.layers):
            if isinstance(l, HipCategoricalLayer):
                if l.probs is None or l.probs.softmax_source() is None:
                    raise NotImplementedError("training: Categorical layers need probs = softmax(tensor)")
            elif isinstance(l, HipGaussianLayer):
                if l.log_partition is not None or (set(l.mean.ops) | set(l.stddev.ops)) - self._PARAM_OPS:
                    raise NotImplementedError("training: Gaussian layers with a log-partition or exotic parameters")
            elif isinstance(l, (HipSumLayer, HipCPTLayer)) and type(l) in (HipSumLayer, HipCPTLayer, HipTuckerLayer):
                if set(l.weight.ops) - self._PARAM_OPS:
                    raise NotImplementedError(f"training: weight parameterisation {l.weight.ops}")
            elif isinstance(l, (HipHadamardLayer, HipKroneckerLayer)):
                pass
            else:
                raise NotImplementedError(f"training: layer type {spec.type!r}")

    def _fast_softmax(self, l) -> bool:
        """tensor -> softmax weights evaluated by the batched prologue: their backward is one kernel."""
        return l.weight.ops == ["tensor", "softmax"] and l.weight.softmax_source() is not None and not l._mixing

    def _accumulate_flags(self) -> tuple[dict[int, int], set[int]]:
        """Per consumer layer: 0 store / 1 add / 2 atomic; and the producer layers whose gradient
        block must be zeroed first.  A layer whose children -- (producer, fold) pairs -- are read by nobody else (any
        tree-structured region graph) STORES their gradients: nothing to zero, nothing to add."""
        c = self.circuit
        count: dict[tuple[int, int], int] = {}
        dup_in_layer: dict[int, bool] = {}
        for j, ch in enumerate(c._children):
            if ch is None:
                continue
            pairs = ch.reshape(-1, 2)
            uniq = np.unique(pairs, axis=0)
            dup_in_layer[j] = len(uniq) != len(pairs)
            for p, f in uniq:
                count[(int(p), int(f))] = count.get((int(p), int(f)), 0) + 1
        flags: dict[int, int] = {}
        for j, ch in enumerate(c._children):
            if ch is None:
                continue
            if dup_in_layer[j]:
                flags[j] = 2
            elif any(count[(int(p), int(f))] > 1 for p, f in ch.reshape(-1, 2)):
                flags[j] = 1
            else:
                flags[j] = 0
        # a launch with flag 1/2 adds into ALL its producers: they all must start from zero
        need_zero: set[int] = set()
        for j, fl in flags.items():
            if fl:
                need_zero |= {int(p) for p in np.unique(c._children[j][..., 0])}
        # (a storing layer may share a producer LAYER with an adding one: its own (producer, fold) blocks have no other writer
        #  -- that is what flag 0 means -- and the zero fills run before every backward launch, so the store loses nothing)
        return flags, need_zero

    def _shared_children(self, B: int, bd, flags: dict[int, int]) -> tuple[dict[int, SharedChildren], torch.Tensor]:
        """Layers whose folds share children (flag 2): contributions go to a temporary (one block per (fold, slot)) and are
        added per distinct child by ck_segment_add_rows instead of through float atomics.  Returns (layer -> its tables, the
        temporary)."""
        c = self.circuit
        shared, tmp_elems = {}, 0
        for j, fl in flags.items():
            l = c.layers[j]
            if fl != 2 or bd.row_off[j] is None:
                continue
            ro = bd.row_off[j].cpu().numpy().reshape(-1)  # element offsets of the (fold, slot) children in the arena
            block = B * l.num_input_units
            uniq, inv = np.unique(ro, return_inverse=True)
            order = np.argsort(inv, kind="stable")
            cptr = np.concatenate([[0], np.cumsum(np.bincount(inv, minlength=len(uniq)))])
            dev = self.device
            shared[j] = SharedChildren(
                row_off=(torch.arange(len(ro), dtype=torch.int64) * block).to(dev),
                cptr=torch.from_numpy(cptr.astype(np.int32)).to(dev),
                clist=torch.from_numpy(order.astype(np.int32)).to(dev),
                coff=torch.from_numpy(uniq.astype(np.int64)).to(dev),
                n_child=int(len(uniq)), block=int(block),
            )
            tmp_elems = max(tmp_elems, len(ro) * block)
        return shared, torch.empty(max(tmp_elems, 1), dtype=torch.float32, device=self.device)

    def _bind_backward(self, B: int) -> BackwardBinding:
        st = self._bwd.get(B)
        bd = self.circuit._bind(B)
        if st is not None and st.arena_ptr == bd.arena.data_ptr():
            return st
        c = self.circuit
        garena = torch.zeros_like(bd.arena)
        gviews = []
        for i, l in enumerate(c.layers):
            if bd.views[i] is None:  # (fused: never materialised)
                gviews.append(None)
                continue
            n = l.num_folds * B * l.num_output_units
            off = bd.views[i].data_ptr() - bd.arena.data_ptr()
            gviews.append(garena.view(torch.uint8)[off : off + 4 * n].view(torch.float32).view(l.num_folds, B, l.num_output_units))
        flags, need_zero = self._accumulate_flags()
        # linear-space weight gradients (dW, dTable) live in ONE flat buffer: a single fill per step
        sizes = {}
        for i, l in enumerate(c.layers):
            if isinstance(l, (HipSumLayer, HipCPTLayer)) and not (l.weight.ops == ["tensor"]):
                sizes[i] = tuple(l._w.shape) if l._w is not None else (l.num_folds, l.num_output_units, l.num_input_units)  # mixing layers: the (F, K, H) coefficients
            elif isinstance(l, HipCategoricalLayer):
                sizes[i] = (l.num_folds, l.num_categories + 1, l.num_output_units)
            elif isinstance(l, HipGaussianLayer):
                sizes[(i, "mean")] = sizes[(i, "stddev")] = (l.num_folds, l.num_output_units)
        flat = torch.zeros(sum(int(np.prod(sh)) for sh in sizes.values()) or 1, dtype=torch.float32, device=self.device)
        dws, off = {}, 0
        for i, sh in sizes.items():
            n = int(np.prod(sh))
            dws[i] = flat[off : off + n].view(sh)
            off += n
        shared, tmp = self._shared_children(B, bd, flags)
        st = BackwardBinding(arena_ptr=bd.arena.data_ptr(), garena=garena, gviews=gviews, flags=flags, need_zero=need_zero,
                             dws=dws, dw_flat=flat, shared=shared, tmp=tmp)
        if self.fused:  # (its tables hold addresses of the buffers above: one owner, one life)
            st.fused = self._fused_step.bind(B, bd, st)
        while len(self._bwd) >= 4:  # like the forward bindings: a handful of batch sizes stay resident
            self._bwd.pop(next(iter(self._bwd)))
        self._bwd[B] = st
        return st

    # ------------------------------------------------------------------------------------------
    def loss_and_grads(self, x: torch.Tensor, *, global_batch: int | None = None) -> torch.Tensor:
        """Forward + backward for ``loss = -(1/global_batch) sum_b log p(x_b)``; gradients land in
        ``self.grads`` (views of one flat buffer).  Returns the device tensor [sum log p, count] of this shard -- a view
        of the circuit's own buffer, overwritten by the next step (clone it to keep it).

        ``global_batch``: see `TrainerSurface._global_batch`."""
        with torch.cuda.device(self.device):  # every launch below goes to a stream of self.device
            return self._loss_and_grads(x, global_batch)

    def _loss_and_grads(self, x: torch.Tensor, global_batch: int | None) -> torch.Tensor:
        self._grads_current = True
        B = int(x.shape[0])
        gB = self._global_batch(B, global_batch)
        if self._jobs is not None:  # one recorded launch list: parameters, forward levels, root, backward levels
            return self._jobs.loss_and_grads(x, gB)
        ll = self._forward(x)
        self._backward(B, gB, None)
        return ll

    def _forward(self, x: torch.Tensor) -> torch.Tensor:
        """The training forward: [sum log p, count] of the batch; fused: kept tiles of the leaf region + tail outputs,
        layer-wise: every activation stays in the arena."""
        return self.circuit.log_likelihood_sum(x)

    def _backward(self, B: int, gB: float, seed, with_opt: bool = False) -> None:
        """The backward launch list over the activations of the LAST forward at batch size B: gradients of
        ``sum_b seed[b] * log p(x_b)`` (seed None: of ``-(1 / gB) sum_b log p(x_b)``) into `self.grads`.  A root of K units
        (a class-conditional circuit) takes a seed of B x K values -- a tensor, or a callable ``seed(view, stream)`` that
        writes the root's (B, K) gradient view itself; layer-wise form only."""
        c = self.circuit
        bd = c._bind(B)
        st = self._bind_backward(B)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if self.fused:
            return self._fused_step.backward(B, gB, seed, bd, st, stream, with_opt)
        capi.call("ck_fill_f32", st.dw_flat.data_ptr(), st.dw_flat.numel(), 0.0, stream)
        capi.call("ck_fill_f32", self._flat_grad.data_ptr(), self._flat_grad.numel(), 0.0, stream)
        gviews = st.gviews
        for p in st.need_zero:
            capi.call("ck_fill_f32", gviews[p].data_ptr(), gviews[p].numel(), 0.0, stream)
        po, fo = int(c._out_pairs[0, 0]), int(c._out_pairs[0, 1])
        units = c.layers[po].num_output_units
        if units != 1 and seed is None:
            raise NotImplementedError("training needs a scalar output unit")
        capi.call("ck_fill_f32", gviews[po].data_ptr(), gviews[po].numel(), 0.0, stream)
        if seed is None:
            capi.call("ck_fill_f32", gviews[po][fo].data_ptr(), B, -1.0 / gB, stream)
        elif callable(seed):  # (the class head, cirkit_amd/classification.py: it writes the (B, units) seed in place)
            seed(gviews[po][fo], stream)
        else:  # (an arbitrary gradient of the outputs: `HipCircuitModule` under autograd)
            if seed.numel() != B * units:
                raise ValueError(f"the seed holds {seed.numel()} values, the root has {B} rows of {units} units")
            gviews[po][fo].reshape(-1).copy_(seed.reshape(-1))
        for i in range(len(c.layers) - 1, -1, -1):
            l = c.layers[i]
            if isinstance(l, (HipCategoricalLayer, HipGaussianLayer)):
                self._bwd_input_layer(i, bd, st, B, stream)
            elif isinstance(l, HipHadamardLayer):
                ga, ro, fl = st.target(i, bd)
                capi.call("ck_hadamard_bwd", ga, ro, gviews[i].data_ptr(), l.num_folds, l.arity, B, l.num_input_units, fl, stream)
                st.gather_shared(i, stream)
            elif isinstance(l, HipKroneckerLayer):  # inner.py:178-187
                ga, ro, fl = st.target(i, bd)
                capi.call("ck_kronecker_bwd", ga, ro, gviews[i].data_ptr(), l.num_folds, l.arity, B, l.num_input_units, fl, stream)
                st.gather_shared(i, stream)
            elif l._mixing:
                dmw = st.dws[i]
                ga, ro, fl = st.target(i, bd)
                capi.call("ck_mixing_lse_bwd", bd.arena.data_ptr(), ga, bd.row_off[i].data_ptr(), ro,
                          l._w.data_ptr(), gviews[i].data_ptr(), dmw.data_ptr(), l.num_folds, l.arity, B,
                          l.num_output_units, fl, stream)
                st.gather_shared(i, stream)
                if l._batched:  # tensor -> softmax evaluated by the batched prologue: its backward is one kernel
                    name = l.weight.graph.nodes[0].config["tensor"]
                    capi.call("ck_param_softmax_bwd", l._w.data_ptr(), dmw.data_ptr(), self.grads[name].data_ptr(),
                              l.num_folds * l.num_output_units, dmw.shape[-1], 0, stream)
                else:
                    l.weight.backward(dmw, self.grads, stream, upto=len(l.weight.graph.nodes) - 2)
            else:  # sum / cpt
                self._bwd_sum_layer(i, bd, st, B, stream)

    def _bwd_input_layer(self, i: int, bd, st: BackwardBinding, B: int, stream: int) -> None:
        """Backward launch of Categorical / Gaussian layer i, then its parameters'."""
        l = self.circuit.layers[i]
        if isinstance(l, HipCategoricalLayer):
            dT = st.dws[i]
            capi.call("ck_categorical_bwd", st.gviews[i].data_ptr(), None, bd.xt_i.data_ptr(), l._scope(self.device).data_ptr(),
                      dT.data_ptr(), l.num_folds, B, l.num_output_units, l.num_categories, 1, None, stream)
            name = l.probs.graph.nodes[0].config["tensor"]
            capi.call("ck_param_log_table_bwd", l._table.data_ptr(), dT.data_ptr(), self.grads[name].data_ptr(),
                      l.num_folds, l.num_output_units, l.num_categories, 0, stream)
        else:
            mean, stddev, _ = l._vals
            dm, ds = st.dws[(i, "mean")], st.dws[(i, "stddev")]
            capi.call("ck_gaussian_bwd", st.gviews[i].data_ptr(), bd.xt.data_ptr(), l._scope(self.device).data_ptr(),
                      mean.data_ptr(), stddev.data_ptr(), dm.data_ptr(), ds.data_ptr(), l.num_folds, B,
                      l.num_output_units, stream)
            l.mean.backward(dm, self.grads, stream)
            l.stddev.backward(ds, self.grads, stream)

    def _bwd_sum_layer(self, i: int, bd, st: BackwardBinding, B: int, stream: int) -> None:
        """Backward launch of sum / CP-T layer i over its materialised inputs and output gradient, then its weight's
        parameter graph (semiring.py:383-408 under autograd)."""
        c = self.circuit
        l, gviews = c.layers[i], st.gviews
        raw = l.weight.ops == ["tensor"]
        dW = self.grads[l.weight.graph.nodes[0].config["tensor"]] if raw else st.dws[i]
        ga, ro, fl = st.target(i, bd)
        capi.call("ck_sum_lse_bwd", bd.arena.data_ptr(), ga, bd.row_off[i].data_ptr(), ro,
                  l._w.data_ptr(), bd.views[i].data_ptr(), gviews[i].data_ptr(), dW.data_ptr(), l.num_folds,
                  l.arity, B, l.num_input_units, l.num_output_units, l._mode, fl, stream)
        st.gather_shared(i, stream)
        if self.fused:
            return  # (one batched softmax backward for all layers at the end of `FusedStep.backward`)
        if self._fast_softmax(l):
            name = l.weight.graph.nodes[0].config["tensor"]
            rows = l.num_folds * l.num_output_units
            capi.call("ck_param_softmax_bwd", l._w.data_ptr(), dW.data_ptr(), self.grads[name].data_ptr(),
                      rows, dW.shape[-1], 0, stream)
        elif not raw:
            l.weight.backward(dW, self.grads, stream)

    def gradients(self) -> dict[str, np.ndarray]:
        """The gradients of the last `loss_and_grads`, host copies in the shapes of the user's plan."""
        if not self._grads_current:
            raise RuntimeError("gradients(): the last step was a fused job step, whose gradients never reach `grads` (the optimizer runs "
                               "in the job epilogues); call loss_and_grads() to obtain them")
        out = {}
        for n in self.user_plan.tensors:
            g = self.grads[n].detach().cpu().numpy()
            out[n] = self._pad_info.unpad(n, g) if self._pad_info is not None else g
        return out

    def parameters(self) -> dict[str, np.ndarray]:
        """The current parameter values, host copies in the shapes of the user's plan."""
        return {n: self.circuit.store.export(n) if self._pad_info is None else
                self._pad_info.unpad(n, self.circuit.store[n].detach().cpu().numpy()) for n in self.user_plan.tensors}

    def apply_gradients(self, skip_flag: torch.Tensor | None = None) -> None:
        """The optimizer step on `self.grads`.  `skip_flag`: a device int32; when it is nonzero at launch time the step
        changes nothing (parameters, moments, Adam's step count)."""
        with torch.cuda.device(self.device):
            self._apply_gradients(skip_flag)

    def _fused_opt_ok(self) -> bool:
        """The fused form takes the optimizer into its backward epilogues: `fuse_optimizer`, no padded duplicates to follow,
        a Categorical table the epilogue's table job applies to (C % 4 == 0; `train_fused.why_not_fused` checked C <= 256)."""
        return (self.fused and self._fuse_optimizer and self._pad_info is None and self._jobs is None
                and self.circuit.layers[self._fused_step.tables.group.input_layer].num_categories % 4 == 0)

    @property
    def _fz(self) -> dict | None:  # (bench.py reads the fused group here: its one reader)
        return {"group": self._fused_step.tables.group} if self.fused else None

    def _use_clock(self, which: str) -> None:
        """ONE optimizer clock per trainer: the fused job step counts Adam's steps on the device (`ck_opt_state.step`, not advanced
        by dropped batches), `apply_gradients` on the host (`step_count`).  Both update the same moments, so a trainer that has
        stepped with one refuses the other rather than applying inconsistent bias corrections."""
        if self._clock is not None and self._clock != which:
            raise RuntimeError(f"this trainer's optimizer clock is on the {self._clock}: step() (fused job form, one rank) and "
                               "loss_and_grads() + apply_gradients() (or a process group initialised mid-run) cannot be mixed on "
                               "one HipTrainer; construct it with fuse_optimizer=False to use the host clock throughout")
        self._clock = which

    def _apply_gradients(self, skip_flag: torch.Tensor | None = None) -> None:
        self._use_clock("host")
        self.step_count += 1
        stream = torch.cuda.current_stream(self.device).cuda_stream
        p, g = self._flat_param, self._flat_grad
        skip = None if skip_flag is None else skip_flag.data_ptr()
        if self.optimizer == "adam":
            capi.call("ck_adam_step", p.data_ptr(), g.data_ptr(), self._m1.data_ptr(), self._m2.data_ptr(), p.numel(),
                      self.lr, self.betas[0], self.betas[1], self.eps, self.step_count, 1.0, skip, self._skipped.data_ptr(), stream)
        else:
            capi.call("ck_sgd_step", p.data_ptr(), g.data_ptr(), p.numel(), self.lr, 1.0, skip, stream)
        if self._pad_info is not None:  # padded input-layer units are copies of real ones: follow their update
            for n in self.user_plan.tensors:
                for ax, old, new in self._pad_info.duplicated_axes(n):
                    t = self.circuit.store[n]
                    idx = (torch.arange(old, new, device=t.device) % old)
                    t.narrow(ax, old, new - old).copy_(t.index_select(ax, idx))
        self.circuit.store.touch()  # values changed in place: circuits that cache derived parameters must refresh

    def step(self, x: torch.Tensor, *, global_batch: int | None = None) -> torch.Tensor:
        """One optimisation step on this rank's shard; returns the device tensor [sum log p, count]
        of the shard (before the update)."""
        c = self.circuit
        alone = _world_size() <= 1
        if self._jobs is not None and self._fuse_optimizer and alone:
            # the whole step is one recorded launch list; the optimizer runs where the gradients are (cirkit_amd/train_jobs.py)
            self._use_clock("device")
            self.step_count += 1
            self._grads_current = False
            return self._jobs.step(x, self._global_batch(int(x.shape[0]), global_batch))
        if self._fused_opt_ok() and alone:
            # the fused form with the optimizer in its backward epilogues: no optimizer launch, no parameter prologue before
            # the next forward (`grads` still receives every gradient)
            self._use_clock("device")
            self.step_count += 1
            with torch.cuda.device(self.device):
                self._grads_current = True
                B = int(x.shape[0])
                ll = self._forward(x)
                self._backward(B, self._global_batch(B, global_batch), None, with_opt=True)
                c.store.raw_writes += 1
            return ll
        ll = self.loss_and_grads(x, global_batch=global_batch)
        # the flag a batch with an out-of-range category raised is THIS step's (fused: handed on by the backward's first launch;
        # layer-wise: latched and cleared after the update); everything stays on the device -- no host synchronisation
        validate = c.validate_inputs and c._int_input
        self._reduce_and_apply((self._step_flag if self.fused else c._bad_input) if validate else None, alone, latch=not self.fused)
        return ll

    @property
    def skipped_steps(self) -> int:
        """Steps that changed nothing because their batch held an illegal category (a device read)."""
        return int(self._skipped.item()) + self.opt_counters()[1]


class _CircuitFunction(torch.autograd.Function):
    """``y = circuit(x)`` with the hand-written backward of `HipTrainer` behind it."""

    @staticmethod
    def forward(ctx, module, x, *params):
        tr = module._trainer
        with torch.cuda.device(tr.device):
            po, fo = int(tr.circuit._out_pairs[0, 0]), int(tr.circuit._out_pairs[0, 1])
            units = tr.circuit.layers[po].num_output_units
            if units == 1:
                tr._forward(x)  # the training forward (what the backward needs stays on the device)
            else:  # (K output units: the layer-wise forward as it is, there is no log-likelihood sum to take)
                tr.circuit._run(x)
            B = int(x.shape[0])
            bd = tr.circuit._bind(B)
            y = bd.views[po][fo].reshape(B, 1, units).clone()
        module._generation += 1
        ctx.module, ctx.B, ctx.generation = module, B, module._generation
        return y

    @staticmethod
    def backward(ctx, gout):
        m = ctx.module
        if ctx.generation != m._generation:
            raise RuntimeError("HipCircuitModule: backward of a forward that is not the last one (the activations live in ONE "
                               "arena: call backward before the next forward)")
        tr = m._trainer
        with torch.cuda.device(tr.device):
            tr._backward(ctx.B, float(ctx.B), gout.to(torch.float32).contiguous())
        return (None, None, *[tr.grads[n].clone() for n in m._names])


class HipCircuitModule(torch.nn.Module):
    """A ``torch.nn.Module`` over a plan: the reference's training loop, unchanged, on the plan-level HIP path --

        m = HipCircuitModule(plan, tensors);  opt = torch.optim.Adam(m.parameters(), lr=0.01)
        loss = -m(batch).mean();  loss.backward();  opt.step()          # notebooks/learning-a-circuit.ipynb, cell 18

    `forward` is the layer-wise HIP forward (``(B, 1, K)`` log-likelihoods like ``TorchCircuit.forward``), `backward` the
    launch list of cirkit_amd/csrc/ck_backward.hip (`HipTrainer`), for ANY gradient of the outputs.  The parameters are
    ``nn.Parameter``s over the trainer's own storage (one flat buffer), so any torch optimizer updates the circuit in place.
    One forward at a time: its activations live in one arena, `backward` must run before the next `forward`.  Same
    coverage as `HipTrainer` (real lse-sum circuits with one output fold); a root of K > 1 units -- a class-conditional
    circuit, notebooks/generative-vs-discriminative-circuit.ipynb: ``F.cross_entropy(m(x)[:, 0, :], y).backward()`` --
    always runs the layer-wise form."""

    def __init__(self, plan: Plan, tensors: Mapping[str, object], *, device: str | torch.device = "cuda:0") -> None:
        super().__init__()
        out = resolve_fold_index(plan.output, [l.num_folds for l in plan.layers]).reshape(-1, 2)
        multi = any(plan.layers[int(p)].num_output_units != 1 for p in out[:, 0])
        self._trainer = HipTrainer(plan, tensors, device=device, optimizer="sgd", lr=0.0, jobs=False,
                                   fused=False if multi else None)  # (any output gradient)
        self._names = list(self._trainer.plan.tensors)
        self._generation = 0
        self.params = torch.nn.ParameterList([torch.nn.Parameter(self._trainer.circuit.store[n]) for n in self._names])

    def named_tensors(self) -> dict[str, torch.nn.Parameter]:
        return dict(zip(self._names, self.params))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return _CircuitFunction.apply(self, x, *self.params)
