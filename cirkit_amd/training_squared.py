"""Plan-level training of squared circuits p(x) = |c(x)|^2 / Z with real parameters, under complex-lse-sum or lse-sum.

The reference trains such a model with autograd through its torch layers (``loss = -mean(2 Re c(x) - Re Z)``: c compiled under
complex-lse-sum -- Embedding + CP-T / sum layers, layers/input.py:258-266, optimized.py:171-178, semiring.py:441-476 -- and
Z = integrate(multiply(c, conj(c))) made of ConstantValue, Hadamard and TensorDot layers whose parameters are pointer / conj /
einsum / flatten graphs over the tensors of c, symbolic/operators.py:39-322; a REAL circuit squares the same way under lse-sum,
``loss = -mean(2 c(x) - Z)``, Categorical inputs whose products integrate to logs of Gram matrices, operators.py:51-63,
106-139).  `cirkit_amd.training.HipTrainer` covers single real circuits; this module is its counterpart for that model class:

* forward: two layer-wise `HipCircuit`s (c on the batch, Z on no input) sharing ONE parameter store;
* backward: a reverse launch list per circuit (cirkit_amd/train_reverse.py) over the gradient arena (complex64 or fp32) -- `ck_sum_lse_bwd_c` /
  `ck_sum_lse_bwd` for sum / CP-T / Tucker layers and, on a permuted copy of their input, TensorDot layers; `ck_hadamard_bwd`
  (on (re, im) pairs under the complex semiring); `ck_categorical_bwd` + d log w / dw for Embedding layers, +
  `ck_param_log_table_bwd` for Categorical layers; the batch sum (+ d log v / dv) for ConstantValue layers -- and
  `HipParameter.backward` through the parameter graphs (pointer gathers, conj of real values, softmax, einsum, log, flatten:
  cirkit_amd/parameters.py);
* where its layers allow it, c on signed-log blocks instead (cirkit_amd/train_signed.py: forward and backward in one list);
* one flat parameter / gradient / moment buffer: one optimizer launch, one all-reduce.

torch appears as storage only: after the forwards of c and Z (two recorded programs each) the backward lists, the
log-likelihood pair and -- on one rank -- the optimizer with its device clock (`ck_opt_state`) are three recorded `ck_program`s per
batch size (c, Z beside it on a second stream, the end), replayed by the native executor (`use_graph=True`: as hipGraphs -- measured
slower: 1.30 against 1.24 ms per 4096 rows); no tensor-library kernel and no allocation in a step.  Restrictions (checked, `NotImplementedError`): real parameter tensors, every (layer, fold)
read by exactly one consumer (trees: what `squared_partition_plan` and the region-graph templates give), a scalar output.

This module holds `HipSquaredTrainer` alone: the constructor, the stream choreography of a step (`_launch`), its parts as recorded
programs (`_part`, one `_enqueue_<part>` method each) and the public surface."""

from __future__ import annotations

from typing import Mapping

import numpy as np
import torch

from .distributed import world_size as _world_size
from . import _capi as capi
from .circuit import HipCircuit
from .plan import Plan
from .train_reverse import _PlanBackward
from .train_signed import _SignedCircuit
from .train_state import DeviceOptState, FlatBuffers, TrainerSurface


class HipSquaredTrainer(TrainerSurface):
    """Maximum-likelihood training of a squared circuit with real parameters: ``loss = -mean_b (2 Re c(x_b) - Re Z)``
    (the reference's loop for sum-of-squares circuits; c under complex-lse-sum -- or a real circuit under lse-sum --, Z built
    from the plan of c)."""

    def __init__(self, plan_c: Plan, tensors: Mapping[str, object], *, plan_z: Plan | None = None, device: str | torch.device = "cuda:0",
                 lr: float = 0.01, optimizer: str = "adam", betas: tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 use_graph: bool = False, signed: bool | None = None) -> None:
        if plan_c.semiring not in ("complex-lse-sum", "lse-sum"):
            raise NotImplementedError(f"HipSquaredTrainer: semiring {plan_c.semiring!r}")
        if optimizer not in ("adam", "sgd"):
            raise ValueError(f"unknown optimizer {optimizer!r}")
        if plan_z is None:
            from .functional import squared_partition_plan

            plan_z = squared_partition_plan(plan_c)
        dev = torch.device(device)
        for n in plan_c.tensors:
            v = tensors[n]
            if np.iscomplexobj(v) or (hasattr(v, "is_complex") and v.is_complex()):
                raise NotImplementedError("HipSquaredTrainer: complex parameter tensors")
        # parameters, gradients and moments: one flat buffer each (cirkit_amd/train_state.py): one optimizer launch, one all-reduce
        fb = FlatBuffers(plan_c.tensors, tensors, dev, optimizer)
        self._flat_param, self._flat_grad, self._m1, self._m2 = fb.param, fb.grad, fb.m1, fb.m2
        self.plan_c, self.plan_z, self.store, self.grads = plan_c, plan_z, fb.store, fb.grads
        # (every layer evaluates its own parameter graph -- no batched prologue --: `HipParameter.backward` differentiates what
        #  `HipParameter.evaluate` left behind)
        kw = dict(device=dev, use_graph=False, fuse=False, pad_units=False, signed_real=False, tiled_weights=False, dense_on_table=False,
                  fused_weight_softmax=False, batch_params=False)
        self.c = HipCircuit(plan_c, self.store, **kw)
        self.z = HipCircuit(plan_z, self.store, **kw)
        self.circuit, self.device = self.c, self.c.device  # (`circuit`: the one whose batches are validated)
        # Z's launches run beside c's on a second stream: their gradients go to a buffer of their own, added before the optimizer
        self._flat_grad_z = torch.zeros_like(self._flat_grad)
        self._bwd_c, self._bwd_z = _PlanBackward(self.c, self.grads), _PlanBackward(self.z, fb.views(self._flat_grad_z))
        # c on signed-log blocks where its layers allow it (`signed`: None = where they do, True = required, False = never)
        sc = _SignedCircuit(self.c, self.grads) if signed is not False else None
        if signed is True and sc.why is not None:
            raise NotImplementedError(f"HipSquaredTrainer(signed=True): {sc.why}")
        self._signed = sc if (sc is not None and sc.why is None) else None
        self.lr, self.optimizer, self.betas, self.eps = lr, optimizer, betas, eps
        self._bad_seen = torch.zeros(1, dtype=torch.int32, device=self.device)  # latched by `step`, reported by `check_inputs`
        self._ll = torch.zeros(2, dtype=torch.float64, device=self.device)
        self._opt = DeviceOptState(self.device)  # constants, clock, dropped steps
        self.use_graph = bool(use_graph)
        self._programs: dict[tuple, tuple[capi.Program | None, int]] = {}
        self._side: tuple[torch.cuda.Stream, torch.cuda.Stream] | None = None

    # -- the recorded step ----------------------------------------------------------------------------------------------
    def _enqueue_optimizer(self, stream: int, with_z: bool = False) -> None:
        """`with_z`: the optimizer reads c's and Z's gradient buffers and adds them itself (no axpy launch before it; `grads`
        then holds c's part only -- `loss_and_grads` leaves the sum)."""
        p = self._flat_param
        capi.call("ck_opt_step_range", p.data_ptr(), self._flat_grad.data_ptr(), self._flat_grad_z.data_ptr() if with_z else None,
                  None if self._m1 is None else self._m1.data_ptr(), None if self._m2 is None else self._m2.data_ptr(), p.numel(),
                  self._opt_state().ptr, stream)

    def _enqueue(self, part: str, B: int, gB: float, with_optimizer: bool, stream: int) -> None:
        getattr(self, "_enqueue_" + part)(B, gB, with_optimizer, stream)

    def _enqueue_pre(self, B: int, gB: float, with_optimizer: bool, stream: int) -> None:
        """Every buffer the two backward lists ADD into, zeroed on c's stream: Z's list is the longer chain beside c's whole-chip
        launches (LAB_NOTES R6.4), its backward waits for this list behind its forward."""
        n = self._flat_grad.numel()
        capi.call("ck_fill_f32", self._flat_grad.data_ptr(), n, 0.0, stream)
        capi.call("ck_fill_f32", self._flat_grad_z.data_ptr(), n, 0.0, stream)
        self._bwd_z.zero_pool(1, stream)

    def _enqueue_c(self, B: int, gB: float, with_optimizer: bool, stream: int) -> None:
        if self._signed is not None:  # (its forward is part of the list: only the staging of the batch is not)
            self._signed.forward(B, stream)
            self._signed.backward(B, -2.0 / gB, stream)
        else:
            self._bwd_c.run(B, -2.0 / gB, stream)

    def _enqueue_zf(self, B: int, gB: float, with_optimizer: bool, stream: int) -> None:
        """Parameters of Z and its forward (no input: everything is part of the list) ..."""
        self.z._enqueue_params(stream)
        self._bwd_z.forward(1, stream)

    def _enqueue_zb(self, B: int, gB: float, with_optimizer: bool, stream: int) -> None:
        """... its backward."""
        self._bwd_z.run(1, B / gB, stream, pool_zeroed=True)

    def _enqueue_mid(self, B: int, gB: float, with_optimizer: bool, stream: int) -> None:
        """Both forwards are there: the optimizer's clock and the log-likelihood pair (beside Z's backward)."""
        c, z = self.c, self.z
        validate = c.validate_inputs and c._int_input
        if with_optimizer:  # a batch with an illegal category drops the step (skip_now)
            capi.call("ck_opt_tick", self._opt_state().ptr, c._bad_input.data_ptr() if validate else None,
                      self._bad_seen.data_ptr() if validate else None, stream)
        yc = self._signed.output(B) if self._signed is not None else c._bind(B).views[int(c._out_pairs[0, 0])][int(c._out_pairs[0, 1])]
        yz = z._bind(1).views[int(z._out_pairs[0, 0])][int(z._out_pairs[0, 1])]
        capi.call("ck_squared_ll", yc.data_ptr(), B, 2 if yc.is_complex() else 1, yz.data_ptr(), self._ll.data_ptr(), stream)

    def _enqueue_end(self, B: int, gB: float, with_optimizer: bool, stream: int) -> None:
        """Both gradients are there: their sum, or the optimizer reading both."""
        if with_optimizer:
            self._enqueue_optimizer(stream, with_z=True)
        else:
            capi.call("ck_axpy_f32", self._flat_grad.data_ptr(), self._flat_grad_z.data_ptr(), 1.0, self._flat_grad.numel(), stream)

    def _part(self, part: str, B: int, gB: float, with_optimizer: bool, run: torch.cuda.Stream) -> None:
        """One of the recorded launch lists of a step -- "pre": the zero fills of both gradient buffers; "c": forward and backward of
        c; "zf" / "zb": parameters + forward and the backward of Z; "end": the sum of the two gradients, the log-likelihood pair and
        (alone) the optimizer ("mid": the clock and the pair, as soon as both forwards are there) -- per (batch size, global batch): the first two
        calls run eagerly (they size the scratch of the parameter graphs), the third records, later ones replay (as a hipGraph
        when `use_graph`)."""
        # (the lists point at the buffers of c's and Z's states at this batch size -- and, through them, of the circuits' bindings --:
        #  keyed on their serial numbers, never on an address a rebuilt state can get back)
        c_state = self._signed.bind(B) if self._signed is not None else self._bwd_c.bind(B)
        key = (part, B, float(gB), bool(with_optimizer), c_state.serial, self._bwd_z.bind(1).serial)
        prog, seen = self._programs.get(key, (None, 0))
        if prog is None:
            if seen < 2:
                self._enqueue(part, B, gB, with_optimizer, run.cuda_stream)
                self._programs[key] = (None, seen + 1)
                return
            for k in [k for k in self._programs if k[:4] == key[:4] and k != key]:  # (rebuilt states: their lists are stale)
                if self._programs[k][0] is not None:
                    self._programs[k][0].close()
                del self._programs[k]
            prog = capi.Program.record(lambda: self._enqueue(part, B, gB, with_optimizer, run.cuda_stream))
            self._programs[key] = (prog, seen)
        prog.launch(run.cuda_stream, self.use_graph)

    def _launch(self, x: torch.Tensor, B: int, gB: float, with_optimizer: bool) -> None:
        """Forward and backward of c on the caller's stream, forward and backward of Z (a few hundred launches on one row: they
        fill a fraction of the chip) on a second stream beside it, then the end of the step."""
        cur = torch.cuda.current_stream(self.device)
        if self._side is None:
            self._side = (torch.cuda.Stream(self.device), torch.cuda.Stream(self.device))
        main = self._side[0] if (self.use_graph and cur.cuda_stream == 0) else cur  # (a capture cannot run on the legacy stream)
        side = self._side[1]
        if main is not cur:
            main.wait_stream(cur)
        side.wait_stream(cur)
        with torch.cuda.stream(main):  # (the long list first)
            self._part("pre", B, gB, with_optimizer, main)
            zeroed = torch.cuda.Event()
            zeroed.record(main)
            if self._signed is not None:
                self._signed.stage(x, main.cuda_stream)
            else:
                self.c._run(x)  # (B, 1, 1) complex64 / fp32 in c's arena
            self._part("c", B, gB, with_optimizer, main)
        self._part("zf", B, gB, with_optimizer, side)
        z_forward = torch.cuda.Event()
        z_forward.record(side)
        side.wait_event(zeroed)
        self._part("zb", B, gB, with_optimizer, side)
        main.wait_event(z_forward)
        self._part("mid", B, gB, with_optimizer, main)
        main.wait_stream(side)
        self._part("end", B, gB, with_optimizer, main)
        if main is not cur:
            cur.wait_stream(main)

    def loss_and_grads(self, x: torch.Tensor, *, global_batch: int | None = None) -> torch.Tensor:
        """Forward of c on the batch and of Z, then both backward launch lists: the gradients of
        ``-(1 / global_batch) sum_b (2 Re c(x_b)) + (B / global_batch) Re Z`` land in `self.grads`; returns the device tensor
        ``[sum_b 2 Re c(x_b) - B Re Z, B]`` (the shard's summed log-likelihood and its rows; fp64, rewritten by the next call)."""
        with torch.cuda.device(self.device):
            B = int(x.shape[0])
            self._launch(x, B, self._global_batch(B, global_batch), False)
            return self._ll

    def apply_gradients(self, skip_flag: torch.Tensor | None = None) -> None:
        """The optimizer step on `self.grads`.  `skip_flag`: a device int32; nonzero at launch time = the step changes nothing
        (parameters, moments, Adam's step count), the flag is latched into what `check_inputs()` reports and cleared."""
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            capi.call("ck_opt_tick", self._opt_state().ptr, None if skip_flag is None else skip_flag.data_ptr(),
                      None if skip_flag is None else self._bad_seen.data_ptr(), stream)
            self._enqueue_optimizer(stream)
            self.store.touch()

    def step(self, x: torch.Tensor, *, global_batch: int | None = None) -> torch.Tensor:
        """One optimisation step.  A batch with an out-of-range category (an ``IndexError`` in the reference, NaN outputs here)
        must not reach the parameters, exactly as in `HipTrainer.step`: alone, the optimizer's clock (`ck_opt_tick`) moves the
        circuit's flag into the step's skip state and the update changes nothing; with several ranks this rank's gradients are
        zeroed before the all-reduce (every rank takes the same step).  The flag is latched into what `check_inputs()` reports
        and cleared -- no host synchronisation, and alone everything after the two forwards is one replayed launch list."""
        c = self.c
        validate = c.validate_inputs and c._int_input
        alone = _world_size() <= 1
        with torch.cuda.device(self.device):
            B = int(x.shape[0])
            self._launch(x, B, self._global_batch(B, global_batch), alone)
            if alone:
                self.store.touch()
                return self._ll
        self._reduce_and_apply(c._bad_input if validate else None, alone, latch=True)
        return self._ll

    @property
    def step_count(self) -> int:
        return self.opt_counters()[0]

    @property
    def skipped_steps(self) -> int:
        return self.opt_counters()[1]

    def gradients(self) -> dict[str, np.ndarray]:
        return {n: g.detach().cpu().numpy() for n, g in self.grads.items()}

    def parameters(self) -> dict[str, np.ndarray]:
        return {n: self.store.export(n) for n in self.plan_c.tensors}
