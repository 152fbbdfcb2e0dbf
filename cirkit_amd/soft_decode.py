"""Decoding under soft evidence on the GPU: `HipCircuit.soft_mpe` and `HipCircuit.sample_soft` (DESIGN.md section 11,
"Decoding under soft evidence").

Soft evidence (cirkit_amd/soft_evidence.py) gives every soft variable of a row a weight per state, ``log_lik[n, s, c] = log
lambda``.  These two queries return an assignment under ``c(x) prod_v lambda_v(x_v)``: `soft_mpe` the max-product completion
(`mpe`'s upward pass and argmax walk, an input unit over a soft variable worth ``max_c (t_k(c) + log_lik[n, s, c])``),
`sample_soft` an exact joint draw (`sample_conditional`'s walk over the values of the soft bottom-up pass, a soft leaf on the
tree drawing ``c`` in proportion to ``exp(t_k(c) + log_lik[n, s, c])``).  Intervals and arbitrary per-variable sets are the
0 / -inf special case, so `sample_soft` is also exact truncated sampling.

Per chunk of rows both run a bottom-up pass, one walk that records, per (row, soft variable), the input node the row's tree
reached, and one decode-leaf launch over those nodes.  The reference has no such query.  Kernels:
cirkit_amd/csrc/ck_soft_decode.hip.
"""

from __future__ import annotations

from typing import TYPE_CHECKING

import numpy as np
import torch

from . import _capi as capi
from . import sampling
from .mpe import MPEState
from .sampling import Sampler, _seed, chunk_rows, pack, ptr_table, sampler
from .soft_evidence import SoftEvidenceState, _rows, check_call

if TYPE_CHECKING:  # pragma: no cover
    from .circuit import HipCircuit

ARGMAX, DRAW = 0, 1  # the modes of ck_soft_decode_leaf


class SoftDecodeState:
    """The decoding state of one `HipCircuit`, next to its `Sampler`: of its own only the per-set pointer tables and the
    transposed log tables of the decode leaf; the other tables, the arenas and the launches are those of `Sampler._soft` and
    `Sampler._mpe`."""

    def __init__(self, s: Sampler) -> None:
        self.s = s
        if s._soft is None:
            s._soft = SoftEvidenceState(s)
        if s._mpe is None:
            s._mpe = MPEState(s)
        self.soft: SoftEvidenceState = s._soft
        self.mpe: MPEState = s._mpe
        self._key = None  # the parameter state of the transposed log tables
        self._logT: dict[int, torch.Tensor] = {}  # discrete input layer -> (F, K, C) log table, transposed
        self._sets: dict[tuple, dict] = {}  # soft ids -> the decode tables of that set (`_set`)

    # -- once per soft-variable set --------------------------------------------------------------------------------------
    def _set(self, ids: list[int]) -> tuple[dict, dict]:
        """(q, d): the soft set's tables of `SoftEvidenceState` and the decode tables kept here beside them: ``spos_tab`` the
        device array of one ``spos`` pointer per layer (NULL: no soft fold), ``vars`` (S,) int64 the variable ids, ``C_max`` the
        largest state count and ``entries``, q's entries with the address of each fold's block of the transposed log table,
        (K, C), in place of the (C + 1, K) one: the decode leaf reads a unit's states as it reads log_lik, contiguously.  The
        decode tables hold addresses of q's tensors and of the current parameter state's tables, so they live as long as
        that q and that state do."""
        soft, s = self.soft, self.s
        if self._key != soft._key:
            self._logT, self._sets, self._key = {}, {}, soft._key
        q = soft._sets.get(ids, False)
        d = self._sets.get(tuple(ids))
        if d is None or d["q"] is not q:
            dev, zc = s.device, s._z_circuit()
            ent = q["entries_host"].copy()  # (g, K, C, table address, ...) per input fold over a soft variable
            for j in q["spos"]:
                if j not in self._logT:
                    l = zc.layers[j]
                    self._logT[j] = l._table[:, : l.num_categories, :].permute(0, 2, 1).contiguous()  # (F, K, C), the same bits
            lay = np.searchsorted(s.fold_off, ent[:, 0], side="right") - 1
            for i, j in enumerate(lay):
                f, K, C = int(ent[i, 0] - s.fold_off[j]), int(ent[i, 1]), int(ent[i, 2])
                ent[i, 3] = self._logT[int(j)].data_ptr() + f * K * C * 4
            d = {"q": q, "spos_tab": ptr_table([q["spos"].get(j) for j in range(len(s.layers))], dev),
                 "vars": torch.tensor(ids, dtype=torch.int64, device=dev), "C_max": int(ent[:, 2].max()),
                 "entries": torch.from_numpy(ent).to(dev)}
            if len(self._sets) >= 8:  # (as many as `QuerySets` keeps)
                self._sets.pop(next(iter(self._sets)))
            self._sets[tuple(ids)] = d
        return q, d

    # -- per chunk -------------------------------------------------------------------------------------------------------
    def max_leaf(self, j: int, q: dict, ll: torch.Tensor, R: int, bad: torch.Tensor, stream: int) -> None:
        """The max leaf of input layer j over its soft folds, into the MPE arena of R rows."""
        s = self.s
        l = s._z_circuit().layers[j]
        arena, val_off, _ = self.mpe._arena(R)
        capi.call("ck_soft_max_leaf", l._table.data_ptr(), ll.data_ptr(), q["spos"][j].data_ptr(), arena.data_ptr(),
                  val_off.data_ptr(), int(s.fold_off[j]), bad.data_ptr(), l.num_folds, R, l.num_output_units, l.num_categories,
                  int(ll.shape[1]), int(ll.shape[2]), stream)

    def decode_leaf(self, mode: int, q: dict, d: dict, ll: torch.Tensor, node: torch.Tensor, r0: int, nb: int, seed: int,
                    out: torch.Tensor, stream: int) -> None:
        """The value of every soft variable with a recorded node, rows r0 .. r0 + nb - 1 (`ll`, `out`: the chunk's)."""
        s = self.s
        capi.call("ck_soft_decode_leaf", mode, d["entries"].data_ptr(), q["start"].data_ptr(), d["vars"].data_ptr(),
                  int(ll.shape[1]), int(ll.shape[2]), d["C_max"], ll.data_ptr(), node.data_ptr(), r0, nb, s.D, seed,
                  out.data_ptr(), 1 if s.float_out else 0, stream)

    # -- once per call ---------------------------------------------------------------------------------------------------
    def soft_mpe(self, log_lik, x, ids: list[int], return_choices: bool, return_log_value: bool, rows_per_chunk: int | None):
        s, m = self.s, self.mpe
        hc = s.hc
        xm, ll = self.soft._evidence(log_lik, x, ids)
        B, S = int(ll.shape[0]), int(ll.shape[1])
        chunks = chunk_rows(B, rows_per_chunk, m.bytes_per_row)
        sizes = {nb for _, nb in chunks}
        m.tables()
        for r in [r for r in m._arenas if r not in sizes]:  # two arenas at most: the chunk and the tail
            del m._arenas[r]
        dev = s.device
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            self.soft.tables(stream, flows=False)  # (the layer-wise circuit's log tables, which the leaves read)
            q, d = self._set(ids)
            out = xm.clone()  # (the sentinels mark what is left to fill)
            logv = torch.empty(B, dtype=torch.float32, device=dev)
            bad = torch.zeros(B, dtype=torch.int32, device=dev)
            node = torch.full((B, S), -1, dtype=torch.int32, device=dev)
            flag = hc._bad_input if hc.validate_inputs else None
            table, choices = s.choice_table(B) if return_choices else (s._table, None)
            for r0, nb in chunks:
                xc, lc, bc = xm[r0 : r0 + nb], ll[r0 : r0 + nb], bad[r0:]

                def leaf(j: int) -> None:
                    if j in q["spos"]:
                        self.max_leaf(j, q, lc, nb, bc, stream)

                arena, val_off = m._upward(xc, nb, flag, bc, stream, after_input=leaf)
                capi.call("ck_soft_mpe_walk", table.data_ptr(), m._logw_tab.data_ptr(), m._amax_tab.data_ptr(),
                          d["spos_tab"].data_ptr(), len(s.layers), s.root_fold, 0, s.total_folds, s.S, arena.data_ptr(),
                          val_off.data_ptr(), bad.data_ptr(), r0, nb, B, s.D, S, node.data_ptr(), xc.data_ptr(),
                          out[r0].data_ptr(), 1 if s.float_out else 0, logv.data_ptr(), stream)
                self.decode_leaf(ARGMAX, q, d, lc, node, r0, nb, 0, out[r0], stream)
            s.fill_uncovered(out, logv)
        return pack(out, choices, logv if return_log_value else None)

    def sample_soft(self, log_lik, x, ids: list[int], seed: int | None, return_choices: bool, return_log_evidence: bool,
                    rows_per_chunk: int | None):
        s, soft = self.s, self.soft
        xm, ll = soft._evidence(log_lik, x, ids)
        B, S = int(ll.shape[0]), int(ll.shape[1])
        chunks = chunk_rows(B, rows_per_chunk, s.hc.arena_bytes(1))
        seed = _seed(seed)
        soft._release({nb for _, nb in chunks})
        dev = s.device
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            soft.tables(stream, flows=True)  # (and `Sampler.prepare()`: the walk's descriptors and linear weights)
            q, d = self._set(ids)
            out = xm.clone()  # (the sentinels mark what is left to draw)
            logev = torch.empty(B, dtype=torch.float32, device=dev)
            bad = torch.zeros(B, dtype=torch.int32, device=dev)
            node = torch.full((B, S), -1, dtype=torch.int32, device=dev)
            table, choices = s.choice_table(B) if return_choices else (s._table, None)
            wtab = s._weight_table()
            for r0, nb in chunks:
                xc, lc = xm[r0 : r0 + nb], ll[r0 : r0 + nb]
                bd = soft.evidence_forward(nb, q, xc, lc, bad[r0:], stream)
                capi.call("ck_soft_sample_walk", table.data_ptr(), wtab.data_ptr(), d["spos_tab"].data_ptr(), len(s.layers),
                          s.root_fold, 0, s.total_folds, s.S, bd.arena.data_ptr(), s._val_off_table(bd).data_ptr(),
                          bad.data_ptr(), r0, nb, B, s.D, seed, S, node.data_ptr(), xc.data_ptr(), out[r0].data_ptr(),
                          1 if s.float_out else 0, logev.data_ptr(), stream)
                self.decode_leaf(DRAW, q, d, lc, node, r0, nb, seed, out[r0], stream)
            s.fill_uncovered(out, logev)
        return pack(out, choices, logev if return_log_evidence else None)


def _state(hc: "HipCircuit", log_lik, x, soft_vars) -> tuple[SoftDecodeState, list[int]]:
    """Every refusal and argument error -- soft evidence's, in its order, then the sampler's -- and then the circuit's state:
    nothing is allocated or launched, and no `Sampler` is built, before them."""
    ids = check_call(hc, log_lik, x, soft_vars)
    sampling.check_plan(hc.user_plan)
    s = sampler(hc)
    if s._soft_decode is None:
        s._soft_decode = SoftDecodeState(s)
    return s._soft_decode, ids


def soft_mpe(hc: "HipCircuit", log_lik: torch.Tensor, x: torch.Tensor | None = None, *, soft_vars=None,
             return_choices: bool = False, return_log_value: bool = False, rows_per_chunk: int | None = None):
    """`HipCircuit.soft_mpe`: see its docstring."""
    rows_per_chunk = _rows(rows_per_chunk)
    st, ids = _state(hc, log_lik, x, soft_vars)
    return st.soft_mpe(log_lik, x, ids, return_choices, return_log_value, rows_per_chunk)


def sample_soft(hc: "HipCircuit", log_lik: torch.Tensor, x: torch.Tensor | None = None, *, soft_vars=None,
                seed: int | None = None, return_choices: bool = False, return_log_evidence: bool = False,
                rows_per_chunk: int | None = None):
    """`HipCircuit.sample_soft`: see its docstring."""
    rows_per_chunk = _rows(rows_per_chunk)
    st, ids = _state(hc, log_lik, x, soft_vars)
    return st.sample_soft(log_lik, x, ids, seed, return_choices, return_log_evidence, rows_per_chunk)
