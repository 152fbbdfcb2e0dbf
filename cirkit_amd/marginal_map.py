"""Marginal MAP on the GPU: `HipCircuit.marginal_map` ("Marginal MAP").

`mpe` with a third role for a variable.  The variables of the call's query set ``Q`` are maximised, every other variable is
evidence where ``x`` holds a value and SUMMED OUT where it holds the sentinel.  Upward, a fold of a sum-type layer whose
scope is disjoint from ``Q`` is a sum fold, ``log sum_i w_i exp(v_i)``, the value of the marginal forward; a fold whose scope
meets ``Q`` is a max fold, ``max_i (log w_i + v_i)`` in `mpe`'s arithmetic; product units add their children; an input unit
gives ``log p(x_v)`` where observed, ``vmax`` where maximised and its log integral ``vsum`` where summed out.  Downward, the
argmax walk of `mpe` ends at the first sum fold on the tree: nothing below it holds a query variable.

``log_value`` is the mixed sum / max value of the root, which is the value of the returned completion's induced tree;
``log_prob`` is the exact ``log c(q*, x_E)`` of the returned completion, the marginal forward run on the returned rows.
``log_value <= log_prob <= max_q log c(q, x_E)``: a sum of non-negative terms is at least one of them, and ``q*`` is one
assignment.  So ``log_prob`` is a true lower bound of the marginal MAP optimum; ``log_value`` is not an upper bound of
anything.

The reference has no max semiring and no MAP query.  This module reuses the circuit's `Sampler` and its `MPEState`: the
arena layout, ``lw``, ``vmax``, ``amax`` and ``src``; the input layers' log integrals ``vsum`` are built here per parameter
state, the roles ``is_query`` and ``max_fold`` per query set.  Kernels: cirkit_amd/csrc/ck_mmap.hip.
"""

from __future__ import annotations

from typing import TYPE_CHECKING

import numpy as np
import torch

from . import _capi as capi
from .mpe import MPEState
from .plan import resolve_fold_index
from .sampling import Sampler, _is_mixing, chunk_rows, pack, sampler

if TYPE_CHECKING:  # pragma: no cover
    from .circuit import HipCircuit


def query_mask(query_vars, D: int) -> np.ndarray:
    """The (D,) bool mask of the call's query set, from an iterable of ids or a (D,) / (1, D) bool mask."""
    if isinstance(query_vars, np.ndarray) and query_vars.dtype == np.bool_:
        query_vars = torch.from_numpy(query_vars)
    if isinstance(query_vars, torch.Tensor):
        if query_vars.dim() == 2 and query_vars.shape[0] > 1:
            raise ValueError("marginal_map takes one query set for the whole batch: a (D,) or (1, D) mask (the mode of a fold "
                             f"is a property of the call, not of a row; got a {tuple(query_vars.shape)} mask)")
        if query_vars.dtype != torch.bool:
            raise ValueError(f"Expected dtype of tensor to be torch.bool, got {query_vars.dtype}")
        if query_vars.dim() not in (1, 2) or query_vars.shape[-1] != D:
            raise ValueError(f"Circuit scope has {D} variables but query_vars was defined over "
                             f"{query_vars.shape[-1] if query_vars.dim() else 0} != {D} variables")
        return np.ascontiguousarray(query_vars.reshape(-1).cpu().numpy())
    ids = sorted({int(v) for v in query_vars})
    if ids and (ids[0] < 0 or ids[-1] >= D):
        raise ValueError("The variables to maximise must be a subset of the circuit scope")
    mask = np.zeros(D, dtype=bool)
    mask[ids] = True
    return mask


class MarginalMapState:
    """The marginal MAP state of one `HipCircuit`, next to its `Sampler` and `MPEState`: the host structure the fold modes
    are propagated on, the input layers' ``vsum`` (in the sampler's layer dicts) and the tables of the last query set."""

    def __init__(self, s: Sampler, mpe_state: MPEState) -> None:
        self.s, self.mpe = s, mpe_state
        folds = [l.num_folds for l in s.plan.layers]
        covered = np.zeros(s.D, dtype=bool)
        self._structure: list[tuple[bool, np.ndarray]] = []  # per layer: (input?, (F,) variables or (F, H) global child folds)
        self._mixing: list[int] = []
        for d in s.layers:
            spec = d["spec"]
            if spec.inputs is None:
                scope = np.asarray(spec.scope_idx[:, 0], dtype=np.int64)
                covered[scope] = True
                self._structure.append((True, scope))
            else:
                ch = resolve_fold_index(spec.inputs, folds)
                self._structure.append((False, (s.fold_off[ch[..., 0]] + ch[..., 1]).astype(np.int64)))
            self._mixing.append(1 if "weight" in d and _is_mixing(spec) else 0)
        self._uncovered = ~covered
        self._key = None
        self._query: tuple | None = None  # (mask bytes, is_query, max_fold, uncovered query variables or None)

    # -- once per parameter state ------------------------------------------------------------------------------------
    def tables(self) -> None:
        """`MPEState.tables()`, and the log integrals ``vsum`` of the input layers for the store's current values."""
        s = self.s
        self.mpe.tables()
        if self._key == s._key:
            return
        dev = s.device
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            for d in s.layers:
                if d["kind"] not in (capi.CK_SAMPLE_CATEGORICAL, capi.CK_SAMPLE_GAUSSIAN):
                    continue
                tab, sf, sk, sc, t_log, C, _, _, lp = d["src"]
                d["vsum"] = torch.empty((d["F"], d["Ko"]), dtype=torch.float32, device=dev)
                row_c = 1 if d["spec"].type == "binomial" else 0  # (its log-pmf table ends with the integral row)
                capi.call("ck_mmap_input_sum", d["kind"], tab, sf, sk, sc, t_log, C, row_c, lp, d["F"], d["Ko"],
                          d["vsum"].data_ptr(), stream)
        self._key = s._key

    # -- once per query set ------------------------------------------------------------------------------------------
    def query_tables(self, q: np.ndarray) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor | None]:
        """(is_query (D,) uint8, max_fold (total folds,) uint8, the query variables no input layer covers) on the device.
        A fold is a max fold where its scope meets the query set: an input fold where its variable is in it, any other fold
        where one of its child folds is.  One query set is kept."""
        key = q.tobytes()
        if self._query is None or self._query[0] != key:
            s = self.s
            mf = np.zeros(s.total_folds, dtype=np.uint8)
            for j, (is_input, a) in enumerate(self._structure):  # (plan order: children come first)
                g0 = int(s.fold_off[j])
                mf[g0 : g0 + a.shape[0]] = q[a] if is_input else mf[a].any(axis=1)
            unc = np.nonzero(self._uncovered & q)[0]
            self._query = (key, torch.from_numpy(q.astype(np.uint8)).to(s.device), torch.from_numpy(mf).to(s.device),
                           torch.from_numpy(unc).to(s.device) if unc.size else None)
        return self._query[1:]

    # -- per chunk ---------------------------------------------------------------------------------------------------
    def _upward(self, xm: torch.Tensor, R: int, is_query: torch.Tensor, max_fold: torch.Tensor, flag: torch.Tensor | None,
                bad: torch.Tensor, stream: int):
        s = self.s
        arena, val_off, _ = self.mpe._arena(R)
        vals, vo = arena.data_ptr(), val_off.data_ptr()
        x_float = 1 if s.float_out else 0
        for j, d in enumerate(s.layers):
            F, H, Ki, Ko, M, kind, g0 = d["F"], d["H"], d["Ki"], d["Ko"], d["M"], d["kind"], int(s.fold_off[j])
            if kind in (capi.CK_SAMPLE_CATEGORICAL, capi.CK_SAMPLE_GAUSSIAN):
                capi.call("ck_mmap_up_input", kind, d["scope"].data_ptr(), *d["src"], d["vmax"].data_ptr(),
                          d["vsum"].data_ptr(), is_query.data_ptr(), F, Ko, xm.data_ptr(), x_float, R, s.D, vals, vo, g0,
                          None if flag is None else flag.data_ptr(), bad.data_ptr(), stream)
            elif kind in (capi.CK_SAMPLE_HADAMARD, capi.CK_SAMPLE_KRONECKER):
                capi.call("ck_mpe_up_product", kind, d["child"].data_ptr(), F, H, Ki, Ko, vals, vo, g0, R, stream)
            else:
                capi.call("ck_mmap_up_sum", kind, d["child"].data_ptr(), d["lw"].data_ptr(), d["w"].data_ptr(),
                          max_fold.data_ptr(), self._mixing[j], F, H, Ki, Ko, M, vals, vo, g0, R, stream)
        return arena, val_off

    def _walk(self, table: torch.Tensor, arena: torch.Tensor, val_off: torch.Tensor, is_query: torch.Tensor,
              max_fold: torch.Tensor, bad: torch.Tensor, r0: int, nb: int, B: int, xc: torch.Tensor, out: torch.Tensor,
              logv: torch.Tensor, stream: int) -> None:
        s, m = self.s, self.mpe
        capi.call("ck_mmap_walk", table.data_ptr(), m._logw_tab.data_ptr(), m._amax_tab.data_ptr(), max_fold.data_ptr(),
                  is_query.data_ptr(), len(s.layers), s.root_fold, 0, s.total_folds, s.S, arena.data_ptr(), val_off.data_ptr(),
                  bad.data_ptr(), r0, nb, B, s.D, xc.data_ptr(), out[r0].data_ptr(), 1 if s.float_out else 0, logv.data_ptr(),
                  stream)

    # -- once per call ------------------------------------------------------------------------------------------------
    def marginal_map(self, x: torch.Tensor, query_vars, return_choices: bool = False, return_log_value: bool = False,
                     return_log_prob: bool = False, rows_per_chunk: int | None = None):
        s = self.s
        hc = s.hc
        q = query_mask(query_vars, s.D)  # (refusals first: nothing has been copied, prepared or launched)
        xm = s.evidence_batch(x, torch.from_numpy(q))  # (the query entries of x are ignored: they hold the sentinel from here)
        B = int(xm.shape[0])
        per_row = max(self.mpe.bytes_per_row, hc.arena_bytes(1)) if return_log_prob else self.mpe.bytes_per_row
        chunks = chunk_rows(B, rows_per_chunk, per_row)
        sizes = {nb for _, nb in chunks}
        self.tables()
        for r in [r for r in self.mpe._arenas if r not in sizes]:  # two arenas at most: the chunk and the tail
            del self.mpe._arenas[r]
        ps = None
        if return_log_prob:
            from .posterior import _state

            ps, zc = _state(hc), s._z_circuit()
            for b in [b for b in zc._bindings if b != 1 and b not in sizes]:  # (and two bindings of the marginal forward)
                zc._bindings.pop(b).destroy()
                s._val_off.pop(b, None)
        is_query, max_fold, uncovered = self.query_tables(q)
        dev = s.device
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            out = xm.clone()  # (the sentinels of the query entries mark what is left to fill)
            logv = torch.empty(B, dtype=torch.float32, device=dev)
            logp = torch.empty(B, dtype=torch.float32, device=dev) if return_log_prob else None
            bad = torch.zeros(B, dtype=torch.int32, device=dev)
            flag = hc._bad_input if hc.validate_inputs else None
            table, choices = s.choice_table(B) if return_choices else (s._table, None)
            for r0, nb in chunks:
                xc = xm[r0 : r0 + nb]
                arena, val_off = self._upward(xc, nb, is_query, max_fold, flag, bad[r0:], stream)
                self._walk(table, arena, val_off, is_query, max_fold, bad, r0, nb, B, xc, out, logv, stream)
                if ps is not None:  # log c(q*, x_E): the marginal forward of the returned rows
                    bd = ps.evidence_forward(out[r0 : r0 + nb], bad[r0:], stream)
                    logp[r0 : r0 + nb].copy_(bd.views[s.root_layer][s.root_f, :, 0])
            if uncovered is not None:  # query variables outside every input layer's scope read 0, as `mpe` writes them
                cols = out[:, uncovered]
                sent = torch.isnan(cols) if s.float_out else cols < 0
                zero = torch.zeros((), dtype=out.dtype, device=dev)
                out[:, uncovered] = torch.where(sent & torch.isfinite(logv)[:, None], zero, cols)
            if logp is not None:  # (a row without finite mass, or with bad evidence, has no completion: -inf / NaN)
                logp = torch.where(torch.isfinite(logv), logp, logv)
        res = pack(out, choices, logv if return_log_value else None)
        if logp is not None:
            res = (res if isinstance(res, tuple) else (res,)) + (logp,)
        return res


def _state(hc: "HipCircuit") -> MarginalMapState:
    s = sampler(hc)
    if s._mpe is None:
        s._mpe = MPEState(s)
    if s._mmap is None:
        s._mmap = MarginalMapState(s, s._mpe)
    return s._mmap


def marginal_map(hc: "HipCircuit", x: torch.Tensor, query_vars, *, return_choices: bool = False,
                 return_log_value: bool = False, return_log_prob: bool = False, rows_per_chunk: int | None = None):
    """`HipCircuit.marginal_map`: see its docstring."""
    return _state(hc).marginal_map(x, query_vars, return_choices, return_log_value, return_log_prob, rows_per_chunk)
