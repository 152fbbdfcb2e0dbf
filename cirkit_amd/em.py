"""Expectation-maximisation training on the GPU: `HipEMTrainer` ("EM training").

The E-step is `HipCircuit.expected_statistics` (cirkit_amd/expected.py) as it is; the M-step is ONE launch over a job table
built once per trainer (`ck_em_update`, cirkit_amd/csrc/ck_em.hip): every job inverts one parameter graph in closed form on
the batch-summed statistics and updates the raw tensor of the store in place.  The graphs it inverts:

=================  ==========================================================  =========================================
kind               parameter graph                                             layers
=================  ==========================================================  =========================================
CK_EM_ROW_SOFTMAX  tensor -> softmax (last axis)                               sum, CP-T, Tucker weights, Categorical probs
CK_EM_ROW_LINEAR   tensor                                                      the same, and Categorical logits
CK_EM_MIXING       tensor [-> softmax] -> mixing_weight                        mixing (sum) layers
CK_EM_GAUSSIAN     mean: tensor; stddev: tensor -> scaled_sigmoid(vmin, vmax)  Gaussian
CK_EM_BINOMIAL     probs: tensor -> sigmoid                                    Binomial
=================  ==========================================================  =========================================

Everything else is refused at construction, before anything is allocated or launched.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Mapping

import numpy as np
import torch

from . import _capi as capi
from .expected import ExpectedStatistics, _expected
from .plan import IDX_ARRAY, IDX_NONE, FoldIndex, Plan
from .sampling import check_plan

_SUM_TYPES = ("sum", "cpt", "tucker")


@dataclass(frozen=True)
class EMParam:
    """One M-step job as `em_jobs` reads it off a plan: the layer, its kind, the raw tensor(s) and how they are written."""

    layer: int
    kind: int
    tensor: str
    tensor2: str | None = None  # CK_EM_GAUSSIAN: the stddev's raw tensor
    raw_log: bool = False  # row kinds: the raw row holds logarithms
    lo: float = 0.0
    hi: float = 1.0


def _identity(fi: FoldIndex, src: int, folds: int) -> bool:
    if list(fi.ids) != [src]:
        return False
    return fi.kind == IDX_NONE or (fi.kind == IDX_ARRAY and np.array_equal(np.asarray(fi.array).reshape(-1), np.arange(folds)))


def em_jobs(plan: Plan) -> list[EMParam]:
    """The M-step jobs of a plan, or the refusal of `HipEMTrainer`: ``NotImplementedError`` naming the layer, the parameter
    and its ops for a graph outside the module docstring's table, for fold indices inside a graph that are not the
    identity, and for a tensor that more than one parameter reads.  Pure host code: nothing is allocated or launched."""
    check_plan(plan)
    jobs: list[EMParam] = []
    used: dict[str, str] = {}
    for j, l in enumerate(plan.layers):
        kinds: dict[str, tuple] = {}
        for pn, g in l.params.items():
            ops = list(g.ops)
            where = f"layer {j} ({l.type}), parameter {pn!r} with ops {ops}"
            kind = None
            if l.type in _SUM_TYPES and pn == "weight" or l.type == "categorical" and pn == "probs":
                if ops == ["tensor"]:
                    kind = (capi.CK_EM_ROW_LINEAR, False)
                elif ops == ["tensor", "softmax"]:
                    kind = (capi.CK_EM_ROW_SOFTMAX, True)
                elif l.type == "sum" and ops in (["tensor", "mixing_weight"], ["tensor", "softmax", "mixing_weight"]):
                    kind = (capi.CK_EM_MIXING, "softmax" in ops)
            elif l.type == "categorical" and pn == "logits" and ops == ["tensor"]:
                kind = (capi.CK_EM_ROW_LINEAR, True)
            elif l.type == "gaussian" and (pn, ops) in (("mean", ["tensor"]), ("stddev", ["tensor", "scaled_sigmoid"])):
                kind = (capi.CK_EM_GAUSSIAN, False)
            elif l.type == "binomial" and pn == "probs" and ops == ["tensor", "sigmoid"]:
                kind = (capi.CK_EM_BINOMIAL, False)
            if kind is None:
                raise NotImplementedError(f"EM has no closed-form M-step for {where}: the graphs it inverts are tensor, tensor -> "
                                          "softmax, tensor [-> softmax] -> mixing_weight, a Gaussian's tensor / tensor -> "
                                          "scaled_sigmoid and a Binomial's tensor -> sigmoid")
            chain = all(_identity(n.inputs[0], i - 1, g.nodes[i - 1].num_folds) for i, n in enumerate(g.nodes) if i) and \
                _identity(g.output, len(g.nodes) - 1, g.nodes[-1].num_folds) and g.nodes[0].num_folds == l.num_folds
            if not chain:
                raise NotImplementedError(f"EM needs identity fold indices inside a parameter graph: {where}")
            sm = next((n for n in g.nodes if n.op == "softmax"), None)
            if sm is not None and int(sm.config["dim"]) != len(sm.shape) - 1:
                raise NotImplementedError(f"EM needs the softmax over the last axis: {where}")
            if len(g.nodes[0].shape) != (1 if kind[0] in (capi.CK_EM_GAUSSIAN, capi.CK_EM_BINOMIAL) else 2):
                raise NotImplementedError(f"EM over a raw tensor of per-fold shape {tuple(g.nodes[0].shape)}: {where}")
            name = g.nodes[0].config["tensor"]
            if name in used:
                raise NotImplementedError(f"tensor {name!r} is read by {used[name]} and by {where}: EM does not share a tensor "
                                          "between parameters")
            used[name] = where
            kinds[pn] = (kind, name, g)
        if l.type == "gaussian":
            if set(kinds) != {"mean", "stddev"}:
                raise NotImplementedError(f"EM for layer {j} (gaussian) needs exactly the parameters mean and stddev, found "
                                          f"{sorted(l.params)} with ops {[list(g.ops) for g in l.params.values()]}")
            c = kinds["stddev"][2].nodes[1].config
            jobs.append(EMParam(j, capi.CK_EM_GAUSSIAN, kinds["mean"][1], kinds["stddev"][1], False,
                                float(c.get("vmin", 0.0)), float(c.get("vmax", 1.0))))
        else:
            jobs += [EMParam(j, kind, name, None, bool(lg)) for (kind, lg), name, _ in kinds.values()]
    return jobs


class HipEMTrainer:
    """EM training of a monotonic circuit: ``step(x)`` is one E-step (`HipCircuit.expected_statistics`, missing values
    integrated out) and one M-step launch that writes the new raw tensors of the store in place.

    ``theta = (1 - step_size) theta_old + step_size theta_hat`` with ``theta_hat`` the closed form of
    `ExpectedStatistics.normalised` under `pseudocount`.  EM's closed form ASSUMES A LOCALLY NORMALISED CIRCUIT (every sum
    unit's weights and every input unit's distribution sum to 1): guaranteed for softmax graphs, the caller's
    responsibility for bare tensors."""

    def __init__(self, plan: Plan, tensors: Mapping[str, object], *, device: str | torch.device = "cuda:0",
                 step_size: float = 1.0, pseudocount: float = 0.0, pad_units: bool = True) -> None:
        if not 0.0 < float(step_size) <= 1.0:
            raise ValueError(f"step_size must lie in (0, 1], got {step_size}")
        if not 0.0 <= float(pseudocount) < float("inf"):
            raise ValueError(f"pseudocount must be non-negative, got {pseudocount}")
        params = em_jobs(plan)  # (refusals first: nothing has been allocated or launched)
        from .circuit import HipCircuit

        self.user_plan = plan
        self.step_size, self.pseudocount = float(step_size), float(pseudocount)
        self.circuit = HipCircuit(plan, tensors, device=device, pad_units=pad_units)
        self.device = self.circuit.device
        self._params = params
        self._es = _expected(self.circuit)
        ps = self._es.ps
        s = ps.s
        ps.down.structure()
        ps.tables()  # (the evaluated weights behind the support pointers exist from here on)
        dev = self.device
        with torch.cuda.device(dev):
            # the running sums: one flat buffer in the device plan's shapes, zeroed by one launch after every M-step
            shapes = {}
            for j, d in enumerate(s.layers):
                if "w" in d:
                    shapes[("edge", j)] = tuple(d["w"].shape)
                elif "scope" in d:
                    shapes[("leaf", j)] = (d["F"], d["Ko"], 3 if d["kind"] == capi.CK_SAMPLE_GAUSSIAN else d["M"])
            sizes = [int(np.prod(sh)) for sh in shapes.values()] + [int(self._es.unit_at[-1])]
            at = np.concatenate([[0], np.cumsum([-(-n // 64) * 64 for n in sizes])])  # (every block on a 256-byte boundary)
            self._sums = torch.zeros(int(at[-1]), dtype=torch.float32, device=dev)
            views = {k: self._sums[int(a) : int(a) + n].view(sh) for (k, sh), a, n in zip(shapes.items(), at, sizes)}
            self._edge = {j: v for (what, j), v in views.items() if what == "edge"}
            self._leaf = {j: v for (what, j), v in views.items() if what == "leaf"}
            self._unit = self._sums[int(at[-2]) : int(at[-2]) + sizes[-1]]
            # padded units are copies of real ones (cirkit_amd/padding.py): (tensor, axis, first copy, copies, their originals)
            self._copies = []
            if self.circuit._pad_info is not None:
                for n in plan.tensors:
                    for ax, old, new in self.circuit._pad_info.duplicated_axes(n):
                        self._copies.append((n, ax, old, new - old, torch.arange(old, new, device=dev) % old))
        self._pending = False
        self._table: tuple | None = None  # (pointers it was built from, host jobs, device copy)

    # -- the job table: built once, rebuilt only if a buffer it names has moved ---------------------------------------------
    def _job_table(self):
        s, store = self._es.ps.s, self.circuit.store
        rows = []
        for p in self._params:
            d = s.layers[p.layer]
            raw = store[p.tensor]
            stats = self._edge[p.layer] if p.layer in self._edge else self._leaf[p.layer]
            support = d["w"] if "w" in d else None
            rows.append((p, raw, None if p.tensor2 is None else store[p.tensor2], stats, support))
        key = tuple(t.data_ptr() for _, *ts in rows for t in ts if t is not None)
        if self._table is not None and self._table[0] == key:
            return self._table
        arr = (capi.EMJob * len(rows))()
        blocks = 0
        for a, (p, raw, raw2, stats, support) in zip(arr, rows):
            if not raw.is_contiguous() or raw.dtype != torch.float32:
                raise NotImplementedError(f"EM over tensor {p.tensor!r}: not a contiguous fp32 tensor")
            if p.kind == capi.CK_EM_MIXING:
                F, K, H = raw.shape
                n_rows, ln, want = F * K, H, (F, K, H * K)
            elif p.kind in (capi.CK_EM_GAUSSIAN, capi.CK_EM_BINOMIAL):
                n_rows, ln, want = raw.numel(), int(stats.shape[-1]), (*raw.shape, int(stats.shape[-1]))
            else:
                n_rows, ln, want = raw.numel() // raw.shape[-1], int(raw.shape[-1]), tuple(raw.shape)
            if tuple(stats.shape) != tuple(want) or (support is not None and tuple(support.shape) != tuple(want)):
                raise ValueError(f"EM: tensor {p.tensor!r} of shape {tuple(raw.shape)} against statistics of shape "
                                 f"{tuple(stats.shape)} (layer {p.layer})")
            a.raw, a.raw2 = raw.data_ptr(), None if raw2 is None else raw2.data_ptr()
            a.stats, a.support = stats.data_ptr(), None if support is None else support.data_ptr()
            a.rows, a.len, a.kind, a.k = n_rows, ln, p.kind, int(raw.shape[1]) if p.kind == capi.CK_EM_MIXING else 0
            a.raw_log, a.lo, a.hi, a.block_begin = int(p.raw_log), p.lo, p.hi, blocks
            n = capi.load().ck_em_job_blocks(p.kind, n_rows, ln)
            capi.check(min(n, 0), "ck_em_job_blocks")
            blocks += n
        dev_copy = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device)
        self._table = (key, arr, dev_copy)
        return self._table

    def _m_step(self) -> None:
        """The M-step launch on the running sums, which it leaves zeroed; every consumer sees the new parameters.  On a padded
        plan the launch is followed by one gather and one copy per padded unit axis, so that the copies follow their units."""
        hc = self.circuit
        self._es.ps.tables()  # (the support masks are the weights of the store's CURRENT values; a no-op right after an E-step)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            _, arr, dev_copy = self._job_table()
            capi.call("ck_em_update", arr, dev_copy.data_ptr(), len(arr), self.step_size, self.pseudocount, stream)
            self._sums.zero_()
            for n, ax, first, count, idx in self._copies:
                t = hc.store[n]
                t.narrow(ax, first, count).copy_(t.index_select(ax, idx))
        self._pending = False
        hc.store.touch()  # (raw pointers were written: the forward, the sampler's CDF tables, the posterior's tables go stale)

    # -- the public surface ------------------------------------------------------------------------------------------
    def accumulate(self, x: torch.Tensor, missing_vars=None, *, rows_per_chunk: int | None = None) -> torch.Tensor:
        """Add one batch's expected statistics to the running sums (device-side adds, in call order); returns the mean log
        evidence of the batch's live rows, a 0-d device tensor -- NaN (0 / 0) for a batch without a live row.  The E-step
        itself reads one flag back per PARAMETER STATE (`Sampler.prepare`: the monotonicity check behind its CDF tables), so the
        first batch after every `update` waits for the host once; nothing else does."""
        *_, logev, rows = self._es.device_statistics(x, missing_vars, rows_per_chunk, into=(self._edge, self._leaf, self._unit))
        with torch.cuda.device(self.device):
            total = torch.where(torch.isfinite(logev), logev, torch.zeros((), device=self.device)).sum()
            self._pending = True
            return total / rows

    def update(self) -> None:
        """The M-step on the running sums of the `accumulate` calls since the last one."""
        self._m_step()

    def step(self, x: torch.Tensor, missing_vars=None, *, rows_per_chunk: int | None = None) -> torch.Tensor:
        """`accumulate` then `update`; returns the mean log evidence of the live rows under the parameters BEFORE the update,
        as a 0-d device tensor that is not read back here (NaN for a batch without a live row).  The E-step's own read per
        parameter state (`accumulate`) happens once per step, since every step changes the parameters."""
        ll = self.accumulate(x, missing_vars, rows_per_chunk=rows_per_chunk)
        self.update()
        return ll

    def apply(self, stats: ExpectedStatistics) -> None:
        """The M-step on statistics the caller supplies, in the USER plan's shapes (`HipCircuit.expected_statistics`'s)."""
        if self._pending:
            raise RuntimeError("apply(): the running sums hold accumulated batches; call update() first")
        es = self._es
        with torch.cuda.device(self.device):
            for j, us in enumerate(self.user_plan.layers):
                ko = us.num_output_units
                if j in self._edge:
                    dst, src = self._edge[j][:, :ko], stats.edge[j].to(self.device, torch.float32)
                    if es.cols_d[j] is None:
                        dst.copy_(src)
                    else:
                        dst.index_copy_(2, es.cols_d[j], src)
                elif j in self._leaf:
                    self._leaf[j][:, :ko].copy_(stats.leaf[j].to(self.device, torch.float32))
        self._m_step()

    @property
    def num_jobs(self) -> int:
        """Jobs of the M-step launch: one per parameter tensor, one per Gaussian layer."""
        return len(self._params)

    def m_step_bytes(self) -> tuple[int, int]:
        """(bytes of statistics the M-step launch reads, bytes of raw tensors it reads and writes once each)."""
        stats = sum(t.numel() for t in self._edge.values()) + sum(t.numel() for t in self._leaf.values())
        raw = sum(self.circuit.store[n].numel() for p in self._params for n in (p.tensor, p.tensor2) if n is not None)
        return 4 * stats, 4 * raw

    def parameters(self) -> dict[str, np.ndarray]:
        """The current parameter values, host copies in the shapes of the user's plan."""
        return {n: self.circuit.store.export(n) for n in self.user_plan.tensors}

    def check_inputs(self) -> None:
        """Raises ``IndexError`` if a batch since the last call held an observed category out of range (`HipCircuit.check_inputs`)."""
        self.circuit.check_inputs()
