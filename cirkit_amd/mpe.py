"""Most probable explanation on the GPU: `HipCircuit.mpe` ("Most probable explanation").

Given per-row evidence ``x_O``, the completion of the other variables that maximises the circuit under max-product: the
upward pass evaluates every unit in the max-product ("Viterbi") semiring -- a sum-type unit takes ``max_i (log w_i + v_i)``
over its entries with ``w_i > 0``, a product unit adds its children's values, an input unit gives ``log p(x_v)`` where
``x_v`` is observed and ``max_c log p(c)`` where it is maximised -- and the walk follows, top down, the argmax entry of every
unit on the row's induced tree (smallest index on ties).  On a deterministic circuit this is the exact MPE; otherwise it is
the usual max-product approximation and its value a lower bound of ``max_x log c(x_O, x)``.

The reference has no max semiring and no MAP / MPE query.  This module reuses the circuit's `Sampler`: its structure,
descriptor table, choice maps and `prepare()`d weights; the log weights and the input layers' maxima are built here, per
parameter state, on the first `mpe` call.  Kernels: cirkit_amd/csrc/ck_mpe.hip.
"""

from __future__ import annotations

from typing import TYPE_CHECKING

import torch

from . import _capi as capi
from .parameters import HipParameter
from .sampling import Sampler, chunk_rows, fold_block_offsets, pack, ptr_table, sampler

if TYPE_CHECKING:  # pragma: no cover
    from .circuit import HipCircuit

_ALIGN = 64  # elements: every layer's (F, B, Ko) block of the arena starts on a 256-byte boundary


class MPEState:
    """The MPE state of one `HipCircuit`, next to its `Sampler`: the per-parameter-state tables (kept in the sampler's
    layer dicts: ``lw``, ``vmax``, ``amax``, ``src``, ``lp``), their device pointer tables and the upward arenas."""

    def __init__(self, s: Sampler) -> None:
        self.s = s
        for d in s.layers:
            if d["kind"] == capi.CK_SAMPLE_GAUSSIAN and "log_partition" in d["spec"].params:
                d["lp"] = HipParameter(d["spec"].params["log_partition"], s.store)
        self._key = None
        self._logw_tab: torch.Tensor | None = None
        self._amax_tab: torch.Tensor | None = None
        self._arenas: dict[int, tuple[torch.Tensor, torch.Tensor, list[int]]] = {}  # rows -> (arena, val_off, bases)
        sizes = [d["F"] * d["Ko"] for d in s.layers]
        self.sizes_per_row = sizes
        self.bytes_per_row = 4 * int(sum(sizes))

    # -- once per parameter state ------------------------------------------------------------------------------------
    def tables(self) -> None:
        """Log weights of the sum-type layers and the maxima of the input layers for the store's current values."""
        s = self.s
        s.prepare()
        if self._key == s._key:
            return
        dev = s.device
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            for d in s.layers:
                F, Ko, M, kind = d["F"], d["Ko"], d["M"], d["kind"]
                if "w" in d:  # sum / mixing / CP-T / Tucker: (F, Ko, M) linear weights evaluated by prepare()
                    w = d["w"]
                    d["lw"] = torch.where(w > 0, torch.log(w), torch.full((), float("-inf"), device=dev)).contiguous()
                    continue
                if kind not in (capi.CK_SAMPLE_CATEGORICAL, capi.CK_SAMPLE_GAUSSIAN):
                    continue
                d["vmax"] = torch.empty((F, Ko), dtype=torch.float32, device=dev)
                d["amax"] = torch.empty((F, Ko), dtype=torch.int32, device=dev)
                # src: the (tab, sf, sk, sc, t_log, C, mean, stddev, log_partition) arguments of both input launches
                if kind == capi.CK_SAMPLE_GAUSSIAN:
                    d["lp_v"] = d["lp"].evaluate(stream).reshape(F, Ko).contiguous().clone() if "lp" in d else None
                    lp = d["lp_v"].data_ptr() if d["lp_v"] is not None else None
                    d["src"] = (None, 0, 0, 0, 0, 0, d["mean_v"].data_ptr(), d["stddev_v"].data_ptr(), lp)
                elif d["spec"].type == "binomial":  # prepare()'s (F, T + 2, K) log-pmf table
                    d["src"] = (d["tab"].data_ptr(), (M + 1) * Ko, 1, Ko, 1, M, None, None, None)
                else:  # prepare()'s (F, K, C) table of probabilities or logits
                    d["src"] = (d["tab"].data_ptr(), Ko * M, M, 1, 1 if d["is_logits"] else 0, M, None, None, None)
                capi.call("ck_mpe_input_max", kind, *d["src"], F, Ko, d["vmax"].data_ptr(), d["amax"].data_ptr(), stream)
            self._logw_tab = ptr_table([d.get("lw") for d in s.layers], dev)
            self._amax_tab = ptr_table([d.get("amax") if d["kind"] == capi.CK_SAMPLE_CATEGORICAL else None for d in s.layers],
                                       dev)
        self._key = s._key

    # -- per chunk size ----------------------------------------------------------------------------------------------
    def _arena(self, R: int) -> tuple[torch.Tensor, torch.Tensor, list[int]]:
        hit = self._arenas.get(R)
        if hit is None:
            bases, total = [], 0
            for n in self.sizes_per_row:
                bases.append(total)
                total += -(-n * R // _ALIGN) * _ALIGN
            arena = torch.empty(total, dtype=torch.float32, device=self.s.device)
            off = fold_block_offsets(bases, [d["F"] for d in self.s.layers], [d["Ko"] for d in self.s.layers], R)
            hit = self._arenas[R] = (arena, torch.from_numpy(off).to(self.s.device), bases)
        return hit

    def _up_layer(self, j: int, xm: torch.Tensor, R: int, flag: torch.Tensor | None, bad: torch.Tensor, stream: int) -> None:
        """The upward launch of layer j into the arena of R rows."""
        s = self.s
        arena, val_off, _ = self._arena(R)
        vals, vo = arena.data_ptr(), val_off.data_ptr()
        d = s.layers[j]
        F, H, Ki, Ko, M, kind, g0 = d["F"], d["H"], d["Ki"], d["Ko"], d["M"], d["kind"], int(s.fold_off[j])
        if kind in (capi.CK_SAMPLE_CATEGORICAL, capi.CK_SAMPLE_GAUSSIAN):
            capi.call("ck_mpe_up_input", kind, d["scope"].data_ptr(), *d["src"], d["vmax"].data_ptr(), F, Ko, xm.data_ptr(),
                      1 if s.float_out else 0, R, s.D, vals, vo, g0, None if flag is None else flag.data_ptr(), bad.data_ptr(),
                      stream)
        elif kind in (capi.CK_SAMPLE_HADAMARD, capi.CK_SAMPLE_KRONECKER):
            capi.call("ck_mpe_up_product", kind, d["child"].data_ptr(), F, H, Ki, Ko, vals, vo, g0, R, stream)
        else:
            capi.call("ck_mpe_up_sum", kind, d["child"].data_ptr(), d["lw"].data_ptr(), F, H, Ki, Ko, M, vals, vo, g0, R, stream)

    def _upward(self, xm: torch.Tensor, R: int, flag: torch.Tensor | None, bad: torch.Tensor, stream: int, after_input=None):
        """Every layer's upward launch, in plan order (`after_input(j)`: called after the launch of input layer j -- the soft
        max leaf of `soft_mpe`, cirkit_amd/soft_decode.py)."""
        for j, d in enumerate(self.s.layers):
            self._up_layer(j, xm, R, flag, bad, stream)
            if after_input is not None and "scope" in d:
                after_input(j)
        arena, val_off, _ = self._arena(R)
        return arena, val_off

    # -- once per call ------------------------------------------------------------------------------------------------
    def mpe(self, x: torch.Tensor, query_vars, return_choices: bool = False, return_log_value: bool = False,
            rows_per_chunk: int | None = None):
        s = self.s
        hc = s.hc
        xm = s.evidence_batch(x, query_vars)
        B = int(xm.shape[0])
        chunks = chunk_rows(B, rows_per_chunk, self.bytes_per_row)
        sizes = {nb for _, nb in chunks}
        self.tables()
        for r in [r for r in self._arenas if r not in sizes]:  # two arenas at most: the chunk and the tail
            del self._arenas[r]
        dev = s.device
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            out = xm.clone()  # (the sentinels mark what is left to fill)
            logv = torch.empty(B, dtype=torch.float32, device=dev)
            bad = torch.zeros(B, dtype=torch.int32, device=dev)
            flag = hc._bad_input if hc.validate_inputs else None
            table, choices = s.choice_table(B) if return_choices else (s._table, None)
            for r0, nb in chunks:
                xc = xm[r0 : r0 + nb]
                arena, val_off = self._upward(xc, nb, flag, bad[r0:], stream)
                capi.call("ck_mpe_walk", table.data_ptr(), self._logw_tab.data_ptr(), self._amax_tab.data_ptr(), len(s.layers),
                          s.root_fold, 0, s.total_folds, s.S, arena.data_ptr(), val_off.data_ptr(), bad.data_ptr(), r0, nb, B,
                          s.D, xc.data_ptr(), out[r0].data_ptr(), 1 if s.float_out else 0, logv.data_ptr(), stream)
            s.fill_uncovered(out, logv)
        return pack(out, choices, logv if return_log_value else None)


def mpe(hc: "HipCircuit", x: torch.Tensor, query_vars, *, return_choices: bool = False, return_log_value: bool = False,
        rows_per_chunk: int | None = None):
    """`HipCircuit.mpe`: see its docstring."""
    s = sampler(hc)
    if s._mpe is None:
        s._mpe = MPEState(s)
    return s._mpe.mpe(x, query_vars, return_choices, return_log_value, rows_per_chunk)
