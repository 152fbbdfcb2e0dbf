"""What every trainer owns, whatever the form of its step (`HipTrainer` fused / layer-wise, its job form `JobStep`,
`HipSquaredTrainer`): the flat parameter / gradient / moment buffers, the DEVICE optimizer state `ck_opt_state`, and the public
surface that does not depend on how the gradients were formed (the all-reduce, the multi-rank end of `step`, input checks)."""

from __future__ import annotations

from typing import Mapping

import numpy as np
import torch

from . import _capi as capi
from .distributed import all_reduce_sum as _all_reduce_sum, default_comm as _default_comm, world_size as _world_size
from .parameters import TensorStore


class DeviceOptState:
    """The DEVICE `ck_opt_state` of one trainer: the optimizer's constants, its clock (steps taken and dropped) and `skip_now`.
    Created on first use; a change of the constants between steps rewrites them and keeps the clock.  Every byte offset comes
    from the ctypes mirror `capi.OptState`."""

    _CONSTANTS = (("lr", "eps"), ("b1d", "b2d"))  # (first, last) field of each range a change of the constants rewrites

    def __init__(self, device: str | torch.device) -> None:
        self.device = torch.device(device)
        self.bytes: torch.Tensor | None = None
        self._key = None

    def sync(self, lr: float, betas: tuple[float, float], eps: float, optimizer: str) -> DeviceOptState:
        key = (float(lr), tuple(float(b) for b in betas), float(eps), optimizer)
        if key != self._key:
            o = capi.OptState()
            o.lr, o.b1, o.b2, o.eps, o.bc1, o.bc2 = lr, betas[0], betas[1], eps, 1.0, 1.0
            o.kind = 1 if optimizer == "adam" else 0
            o.b1d, o.b2d = float(betas[0]), float(betas[1])  # the bias corrections are formed in double (torch.optim.Adam does)
            new = torch.frombuffer(bytearray(bytes(o)), dtype=torch.uint8).to(self.device)
            if self.bytes is None:
                self.bytes = new
            else:
                for first, last in self._CONSTANTS:
                    lo, hi = getattr(capi.OptState, first).offset, getattr(capi.OptState, last).offset + getattr(capi.OptState, last).size
                    self.bytes[lo:hi].copy_(new[lo:hi])
            self._key = key
        return self

    @property
    def ptr(self) -> int:
        return self.bytes.data_ptr()

    @property
    def skip_now_ptr(self) -> int:
        return self.ptr + capi.OptState.skip_now.offset

    def counters(self) -> tuple[int, int]:
        """(steps taken, steps dropped) of the clock (a device read)."""
        if self.bytes is None:
            return 0, 0
        lo, hi = capi.OptState.step.offset, capi.OptState.skipped.offset + capi.OptState.skipped.size
        v = self.bytes[lo:hi].cpu().view(torch.int32)
        return int(v[0]), int(v[-1])


class FlatBuffers:
    """A trainer's parameters, gradients and (Adam) moments, each ONE flat fp32 buffer in plan order: the store's tensors,
    `grads` and `moments` are views of them, so the optimizer step is a single launch and the all-reduce a single collective."""

    def __init__(self, tensors: Mapping[str, tuple], values: Mapping[str, object], device: str | torch.device, optimizer: str) -> None:
        dev = torch.device(device)
        self.shapes = {n: spec[0] for n, spec in tensors.items()}
        total = sum(int(np.prod(s)) for s in self.shapes.values())
        self.param = torch.empty(total, dtype=torch.float32, device=dev)
        self.store = TensorStore(dev)
        for n, view in self.views(self.param).items():
            v = values[n]
            view.copy_(torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v.detach().to(torch.float32))
            self.store._t[n] = view
        self.store.version += 1
        self.grad = torch.zeros(total, dtype=torch.float32, device=dev)
        self.grads = self.views(self.grad)
        self.m1 = self.m2 = None
        self.moments: dict[str, tuple[torch.Tensor, torch.Tensor]] = {}
        if optimizer == "adam":
            self.m1, self.m2 = torch.zeros_like(self.grad), torch.zeros_like(self.grad)
            m2 = self.views(self.m2)
            self.moments = {n: (v, m2[n]) for n, v in self.views(self.m1).items()}

    def views(self, flat: torch.Tensor) -> dict[str, torch.Tensor]:
        """The per-tensor views of a flat buffer of this layout."""
        out, off = {}, 0
        for n, shape in self.shapes.items():
            sz = int(np.prod(shape))
            out[n] = flat[off : off + sz].view(shape)
            off += sz
        return out


class TrainerSurface:
    """The part of a trainer's public surface the two trainers share.  A subclass sets `circuit` (whose batches are validated),
    `device`, `_flat_grad` (the gradient buffer of its FlatBuffers), `_opt` (DeviceOptState), `_bad_seen` and the optimizer's
    `lr`, `betas`, `eps`, `optimizer`."""

    def _opt_state(self) -> DeviceOptState:
        """The DEVICE `ck_opt_state`, its constants those of the trainer now."""
        return self._opt.sync(self.lr, self.betas, self.eps, self.optimizer)

    def opt_counters(self) -> tuple[int, int]:
        """(steps taken, steps dropped) of the optimizer's device clock (a device read)."""
        return self._opt.counters()

    @staticmethod
    def _global_batch(B: int, global_batch: int | None) -> float:
        """``global_batch`` defaults to the number of rows of ALL ranks when a process group is up (every rank is assumed to hold
        as many rows as this one; pass it explicitly otherwise), so that the SUM all-reduce yields the gradient of the mean NLL."""
        if global_batch is None and _world_size() > 1:
            global_batch = B * _world_size()
        return float(global_batch or B)

    def all_reduce_grads(self) -> None:
        """The one gradient exchange of data-parallel training: SUM over ranks of the flat buffer."""
        import torch.distributed as dist

        # (also at world size 1: the collective is then RCCL's identity, and the same call path is what a 1-GPU box can test)
        # RCCL through the C ABI (ck_comm_all_reduce_f32, on the launch stream) when a HipComm is set; torch.distributed otherwise
        if _default_comm() is not None or (dist.is_available() and dist.is_initialized()):
            _all_reduce_sum(self._flat_grad)

    def _reduce_and_apply(self, flag: torch.Tensor | None, alone: bool, latch: bool) -> None:
        """The end of a step whose gradients are in the flat buffer.  `flag`: the device int32 a batch with an out-of-range
        category raised (None: no validation) -- such a batch must not reach the parameters: alone the optimizer launch skips
        on it; with several ranks the other ranks' gradients are valid and every rank must take the same step, so this rank's
        are zeroed before the all-reduce.  `latch`: the flag is then latched into what `check_inputs()` reports and cleared."""
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if flag is not None and not alone:
            with torch.cuda.device(self.device):
                capi.call("ck_zero_if_flag", self._flat_grad.data_ptr(), self._flat_grad.numel(), flag.data_ptr(), stream)
        self.all_reduce_grads()
        self.apply_gradients(flag if alone else None)
        if flag is not None and latch:
            with torch.cuda.device(self.device):
                capi.call("ck_latch_flag", flag.data_ptr(), self._bad_seen.data_ptr(), stream)

    def check_inputs(self) -> None:
        """Raise ``IndexError`` if a batch since the last check held a category out of range (as the reference's indexing by
        it would have, layers/input.py:258-266, 399-412).  On a single rank the steps on such batches changed nothing
        (parameters, moments, Adam's step count); later valid batches train normally."""
        if int(self._bad_seen.item()) != 0:
            self._bad_seen.zero_()
            self.circuit._bad_input.zero_()
            raise IndexError("a batch held a category outside [0, num_categories) of its variable")
        self.circuit.check_inputs()
