"""Exact marginals and conditionals of a squared circuit ``p(x) = |c(x)|^2 / Z`` on the GPU.

The reference answers ``integral of |c(x_O, x_M)|^2 dx_M`` by building the product circuit symbolically,
``integrate(multiply(c, conjugate(c)), scope=M)`` (cirkit/symbolic/functional.py:161-258 integrate, :259-593 multiply),
and evaluating ALL of it: every fold of ``c`` becomes a fold with ``K^2`` units per row.  Here every fold of ``c`` falls, for
the set ``M`` of a call, into one of three classes (`fold_classes`):

* OBSERVED -- its scope does not meet ``M``: the value of its product fold is the outer product of the ``K`` outputs of
  ``c``'s own forward with their conjugates; never materialised, lifted while it is read (kind RANK-1);
* INTEGRATED -- its scope lies inside ``M``: the value does not depend on the row and is what the partition-function
  circuit (`functional.squared_partition_plan`) computes for that fold once, at batch 1 (kind CONST);
* MIXED -- its scope meets both: only these folds are evaluated at ``K^2`` units per row, by `ck_squared_mixed_fwd`
  (cirkit_amd/csrc/ck_sqmar.hip; kind FULL), one launch per layer of ``c`` that has any.

Under point evidence an input fold has one variable and is never mixed, so the leaf layer of the product circuit is never
materialised.  Soft and interval evidence (cirkit_amd/squared_soft.py: `soft_evidence_log_prob`, `interval_log_prob`, `log_cdf`)
add a third state of a variable -- a weight per state: the input folds of those variables are evaluated too, as weighted Gram
matrices (`ck_squared_soft_leaf`, cirkit_amd/csrc/ck_sqsoft.hip), and read by the same launches as FULL children.

Sampling and the posterior of one variable over all its states walk the other way, from the root down to one input fold
(cirkit_amd/squared_sampling.py: `sample`, `sample_conditional`, `state_log_marginals`, `posterior`), and read the folds beside
that path by the same three kinds.  The posteriors of a whole SET of variables keep that walk for every fold above the set,
layer by layer (cirkit_amd/squared_posterior.py: `query_log_marginals`, `posterior_marginals`).

Out of scope: per-row masks (the class of a fold is a property of the call), complex parameter tensors, fusing ``c``'s
forward with the mixed pass, and a backward beyond those walks (no gradients with respect to parameters).
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import Mapping

import numpy as np
import torch

from . import _capi as capi
from .plan import Plan
from .squared_graph import INTEGRATED, MIXED, OBSERVED, FoldGraph, graph_of, mask_bits

_INPUTS = ("embedding", "categorical", "gaussian")
_CHUNK_BYTES = 2 << 30  # c's arena + the mixed arena of one chunk of rows


def check_squarable(plan: Plan) -> None:
    """What `HipSquaredCircuit` refuses about a plan, before anything is allocated."""
    for l in plan.layers:
        if l.inputs is None and (l.scope_idx is None or l.scope_idx.shape[1] != 1):
            raise NotImplementedError("HipSquaredCircuit: input layers over several variables")
        if l.inputs is None and l.type not in _INPUTS:
            raise NotImplementedError(f"HipSquaredCircuit: squaring {l.type!r} input layers")
        if l.inputs is not None and not (l.type in ("hadamard", "cpt") or (l.type == "sum" and l.arity == 1)):
            raise NotImplementedError(f"HipSquaredCircuit: squaring {l.type!r} layers of arity {l.arity}")


def put_bounded(cache: dict, key, value, capacity: int):
    """`value` into `cache`, which then drops its oldest entries beyond `capacity`."""
    cache[key] = value
    while len(cache) > capacity:
        cache.pop(next(iter(cache)))
    return value


def fold_classes(plan: Plan, mask: np.ndarray, graph: FoldGraph | None = None) -> list[np.ndarray]:
    """Per layer of ``c`` the class of every fold -- OBSERVED (scope disjoint from the integrated set), INTEGRATED (scope
    inside it) or MIXED -- for the ``(D,)`` bool mask of integrated variables, from the variables under each fold."""
    return graph_of(plan, graph).classes(mask)


@dataclass
class MixedLayer:
    """The launch of one layer of ``c``: its evaluated folds, and per (fold, child) the kind and where the child lives --
    ``(layer of c, fold)`` for RANK-1 and CONST children, ``(layer of c, position among that layer's evaluated folds)`` for FULL."""

    layer: int
    folds: np.ndarray  # (n,) folds of the layer, ascending
    kind: np.ndarray  # (n, H) CK_SQ_*
    src: np.ndarray  # (n, H, 2)


@dataclass
class SoftLeaf:
    """The evaluated input folds of one input layer of ``c`` under soft or interval evidence: per fold its variable and that
    variable's position among the soft variables in ascending order (the ``S`` axis of ``log_lik``)."""

    layer: int
    folds: np.ndarray  # (n,) folds of the layer, ascending
    var: np.ndarray  # (n,)
    pos: np.ndarray  # (n,)


@dataclass
class MixedPlan:
    classes: list[np.ndarray]
    layers: list[MixedLayer]
    root: tuple[int, int, int]  # (class of the output fold, layer, fold -- or position among the evaluated folds when MIXED)
    dev: dict = field(default_factory=dict)  # batch size -> device tables
    leaves: list[SoftLeaf] = field(default_factory=list)  # (soft evidence only)

    @property
    def num_mixed(self) -> int:
        return int(sum(len(m.folds) for m in self.layers))


def mixed_plan(plan: Plan, mask: np.ndarray, const_available=None, path=None, readers=None, graph: FoldGraph | None = None,
               soft: np.ndarray | None = None) -> MixedPlan:
    """Which folds a call with this mask evaluates at K^2 units, layer by layer in plan order, and the kind tables of their
    children.  `const_available(layer)`: whether the partition-function circuit keeps that layer's squared output in memory;
    an INTEGRATED child without one is evaluated here like a mixed fold (from CONST children: still exact).  `path`: a set of
    ``(layer, fold)`` that needs no value -- the ancestry of one variable, walked downwards by `squared_sampling` -- but whose
    other children do; the root of the result is then not looked up among the evaluated folds.  `readers`: a set of
    ``(layer, fold)`` whose children are read as well (the down folds of `squared_posterior`) while they keep their own class.
    `soft`: a ``(D,)`` bool mask of variables that carry a weight per state (disjoint from `mask`); every fold whose scope
    meets it is evaluated, INPUT folds too: those form `MixedPlan.leaves`, one record per input layer, and their readers see
    them as FULL children."""
    graph = graph_of(plan, graph)
    cls, children = graph.classes(mask), graph.children
    if soft is not None:
        sbits = mask_bits(soft)
        cls = [np.where(np.asarray([bool(b & sbits) for b in row]), np.int8(MIXED), c) for row, c in zip(graph.bits, cls)]
    need = [set(np.nonzero(c == MIXED)[0].tolist()) for c in cls]
    path = path or set()
    on_path: list[set] = [set() for _ in plan.layers]
    for i, f in path:
        need[i].discard(f)
        on_path[i].add(f)
    for i, f in readers or ():
        on_path[i].add(f)
    for i in range(len(plan.layers) - 1, -1, -1):  # (children sit below their readers)
        if children[i] is None:
            continue
        for f in sorted(need[i] | on_path[i]):
            for p, g in children[i][f]:
                p, g = int(p), int(g)
                if (p, g) in path:
                    continue
                if cls[p][g] == INTEGRATED and const_available is not None and not const_available(p):
                    if plan.layers[p].inputs is None:
                        raise NotImplementedError("HipSquaredCircuit: the partition-function circuit keeps no value of an input layer")
                    need[p].add(g)
    out: list[MixedLayer] = []
    pos: list[dict[int, int]] = [{} for _ in plan.layers]
    leaves: list[SoftLeaf] = []
    for i, l in enumerate(plan.layers):
        if not need[i]:
            continue
        fs = np.asarray(sorted(need[i]), dtype=np.int64)
        pos[i] = {int(f): j for j, f in enumerate(fs)}
        if children[i] is None:  # (only with `soft`: an input fold is otherwise OBSERVED or INTEGRATED)
            var = np.asarray([int(l.scope_idx[f][0]) for f in fs], dtype=np.int64)
            leaves.append(SoftLeaf(i, fs, var, np.cumsum(soft)[var] - 1))
            continue
        kind = np.zeros((len(fs), l.arity), dtype=np.int32)
        src = np.zeros((len(fs), l.arity, 2), dtype=np.int64)
        for j, f in enumerate(fs):
            for h, (p, g) in enumerate(children[i][f]):
                p, g = int(p), int(g)
                if g in pos[p]:
                    kind[j, h], src[j, h] = capi.CK_SQ_FULL, (p, pos[p][g])
                elif cls[p][g] == OBSERVED:
                    kind[j, h], src[j, h] = capi.CK_SQ_RANK1, (p, g)
                else:
                    kind[j, h], src[j, h] = capi.CK_SQ_CONST, (p, g)
        out.append(MixedLayer(i, fs, kind, src))
    op, of = graph.top
    rc = int(cls[op][of])
    return MixedPlan(cls, out, (rc, op, pos[op][of] if rc == MIXED and (op, of) not in path else of), leaves=leaves)


@dataclass
class MixedLaunch:
    """One launch of `ck_squared_mixed_fwd` at a batch size: its counts, where its output starts in the mixed arena, its tables."""

    layer: int
    n: int
    H: int
    Ki: int
    Ko: int
    stages: int
    base: int
    kind: torch.Tensor
    off: torch.Tensor
    wfold: torch.Tensor

    @property
    def units2(self) -> int:
        """Squared units per row of an evaluated fold."""
        return (self.Ko if self.stages else self.Ki) ** 2


@dataclass
class MixedTables:
    """The launches of a (mask, batch size) and the mixed arena they fill (`arena` / `mid` None: a caller brings buffers of
    `total` / `mid_size` values)."""

    key: tuple
    launches: list[MixedLaunch]
    where: dict[tuple[int, int], int]  # (layer, fold) -> offset of its block in the mixed arena
    total: int
    mid_size: int
    arena: torch.Tensor | None
    mid: torch.Tensor | None
    leaves: list = field(default_factory=list)  # `squared_soft.SoftLaunch`: the leaf launches of soft evidence, before `launches`

    def offset(self, layer: int, fold: int) -> int | None:
        """Where the mixed pass wrote fold `fold` of layer `layer`, or None: it did not evaluate it."""
        return self.where.get((layer, fold))


def _mask_of(integrate_vars, D: int, what: str = "marginalize") -> np.ndarray:
    """``(D,)`` bool numpy mask from an iterable of ids or a ``(D,)`` / ``(1, D)`` bool tensor (worded as
    `HipCircuit._apply_integration_mask` words its errors)."""
    if integrate_vars is None:
        return np.zeros(D, dtype=bool)
    if isinstance(integrate_vars, (torch.Tensor, np.ndarray)):
        m = torch.as_tensor(integrate_vars)
        if m.dtype != torch.bool:
            raise ValueError(f"Expected dtype of tensor to be torch.bool, got {m.dtype}")
        if m.dim() == 1:
            m = m.unsqueeze(0)
        if m.dim() != 2 or m.shape[1] != D:
            raise ValueError(f"Circuit scope has {D} variables but integrate_vars was defined over "
                             f"{m.shape[-1] if m.dim() else 0} != {D} variables")
        if m.shape[0] != 1:
            raise ValueError("HipSquaredCircuit takes ONE scope to integrate over per call (a (D,) or (1, D) mask): "
                             "which folds are mixed is a property of the call")
        return np.ascontiguousarray(m[0].cpu().numpy())
    ids = sorted({int(v) for v in integrate_vars})
    if ids and (ids[0] < 0 or ids[-1] >= D):
        raise ValueError(f"The variables to {what} must be a subset of the circuit scope")
    mask = np.zeros(D, dtype=bool)
    mask[ids] = True
    return mask


class HipSquaredCircuit:
    """``p(x) = |c(x)|^2 / Z`` for a circuit ``c`` of Embedding / Categorical / Gaussian inputs (one variable each), Hadamard
    products and dense sums (as such or fused into CP-T layers) with REAL parameter tensors: `log_partition`, `log_prob`,
    `log_marginal` and `conditional_log_prob`, all exact.

    It owns a `HipCircuit` of ``c`` that materialises every fold (no cross-layer fusion; unit counts padded to 32 where
    `HipCircuit` pads them), a `HipCircuit` of the partition function over the same parameter store, and the fold classes
    of the masks it has seen.  Refused (``NotImplementedError``, before anything is allocated): complex parameter tensors,
    layers `functional.squared_partition_plan` refuses (Tucker, Kronecker, dense sums of arity > 1), input layers over several
    variables.  `sample`, `sample_conditional`, `state_log_marginals` and `posterior` (exact too; discrete inputs and region
    graphs that are trees) refuse Gaussian inputs and DAG ancestries; so do `query_log_marginals` and `posterior_marginals`,
    the posteriors of a whole set of query variables from one pass down the folds above them, and `leave_one_out_log_marginals`,
    `leave_one_out` and `conditional_log_probs`, every variable given all the others from one K-sized pass over ``c`` itself.
    `soft_evidence_log_prob`, `interval_log_prob` and `log_cdf` put a weight per state, or a box, on any set of discrete variables
    (DAG region graphs included; Gaussian variables stay hard evidence or integrated); `soft_query_log_marginals`,
    `soft_posterior_marginals` and `sample_soft` give the posteriors of all soft variables and exact joint draws under that
    evidence (trees only, as `posterior_marginals`).
    `autoregressive_conditionals`, `autoregressive_log_probs` and `coding_tables` give the chain rule along an order for rows that
    are known -- one forward of ``c`` and one launch for all steps in `tree_order` -- and cirkit_amd/codec.py compresses with them
    (discrete inputs, trees).  Not
    offered: per-row masks, gradients with respect to parameters; ``c``'s forward and the mixed pass are separate launches."""

    def __init__(self, plan_c: Plan, tensors: Mapping[str, object], *, device: str | torch.device = "cuda:0", rows_per_block: int = 1) -> None:
        from .circuit import HipCircuit
        from .functional import squared_partition_plan

        if plan_c.semiring not in ("complex-lse-sum", "lse-sum"):
            raise NotImplementedError(f"HipSquaredCircuit: semiring {plan_c.semiring!r}")
        for n in plan_c.tensors:
            v = tensors[n]
            if np.iscomplexobj(v) or (hasattr(v, "is_complex") and v.is_complex()):
                raise NotImplementedError("HipSquaredCircuit: complex parameter tensors")
        check_squarable(plan_c)
        squared_partition_plan(plan_c)  # (whatever else it refuses, refused here)
        self.device = torch.device(device)
        self.rows_per_block = int(rows_per_block)
        self.c = HipCircuit(plan_c, tensors, device=self.device, fuse=False)
        if self.c._virtual or self.c._clin is not None or self.c._cp_leftover or self.c._cp_subset:
            raise RuntimeError("HipSquaredCircuit: the circuit of c does not materialise every fold")
        self.plan = self.c.plan  # (padded where HipCircuit pads)
        z_plan, self._z_of = squared_partition_plan(self.plan, return_layer_map=True)
        self.z = HipCircuit(z_plan, self.c.store, device=self.device)
        self._complex = self.plan.semiring == "complex-lse-sum"
        self._esize = 8 if self._complex else 4
        self._cache: dict[bytes, MixedPlan] = {}
        self._z_state = None
        self._z_bd = None
        self.last_launches = 0  # launches of `ck_squared_mixed_fwd` in the last call of `log_marginal`
        self.last_mixed_launches = 0  # ... in the last call of `state_log_marginals` / `posterior` / `sample` / `sample_conditional`
        self._sampler = None
        self.graph = FoldGraph(self.plan)
        self._down_plans: dict = {}  # (Q, I) -> `squared_posterior.DownPlan`
        self.last_down_launches = 0  # launches of `ck_squared_down_bwd` and `ck_squared_down_leaf` in the last call of
        #                              `query_log_marginals` / `posterior_marginals` (their mixed launches: `last_mixed_launches`)
        self._loo_plans: dict = {}  # Q -> `squared_loo.LooPlan`
        self._loo_buf = None  # the derivative arena of the leave-one-out pass, grown to the largest call
        self.last_loo_launches = 0  # launches of `ck_squared_loo_down` and `ck_squared_loo_leaf` in the last leave-one-out call
        self._soft_plans: dict = {}  # (M, S) -> `MixedPlan` with leaves
        self._soft_side = None  # (parameter state, input layer -> (F, K) column maxima of its table of logarithms)
        self.last_soft_launches = 0  # launches of `ck_squared_soft_leaf` in the last soft / interval call (its mixed launches: `last_launches`)
        self._soft_down_plans: dict = {}  # (I, S) -> `squared_posterior.DownPlan` over a soft mixed plan (squared_soft_posterior.py)

    @property
    def num_variables(self) -> int:
        return self.plan.num_variables

    # -- the partition function ------------------------------------------------------------------------------------------------
    def _z_binding(self):
        """The binding of the partition-function circuit at batch 1 with current values (re-evaluated when a parameter changed)."""
        state = (self.c.store.version, self.c.store.state())
        if self._z_bd is None or self._z_state != state:
            self._z_bd = self.z._run(None)
            self._z_state = state
        return self._z_bd

    def _root_of_z(self) -> torch.Tensor:
        bd = self._z_binding()
        p, f = (int(v) for v in self.z._out_pairs[0])
        v = bd.views[p][f, 0, 0]
        return (v.real if self._complex else v).to(torch.float32)

    def log_partition(self) -> torch.Tensor:
        """``log Z`` (0-d fp32)."""
        return self._root_of_z().clone()

    def log_prob(self, x: torch.Tensor) -> torch.Tensor:
        """``(B,)``: ``2 Re log c(x) - log Z``."""
        y = self.c(x)[:, 0, 0]
        return 2 * (y.real if self._complex else y).to(torch.float32) - self._root_of_z()

    # -- marginals ---------------------------------------------------------------------------------------------------------------
    def classify(self, integrate_vars) -> MixedPlan:
        """The fold classes and launch tables of a mask (cached by mask)."""
        mask = _mask_of(integrate_vars, self.plan.num_variables)
        key = mask.tobytes()
        mp = self._cache.get(key)
        if mp is None:
            mp = put_bounded(self._cache, key, mixed_plan(self.plan, mask, self._const_available(), graph=self.graph), 16)
        return mp

    def _const_available(self):
        """`mixed_plan`'s test of a layer: whether the partition-function circuit keeps its squared output in memory."""
        views = self._z_binding().views
        return lambda p: views[self._z_of[p]] is not None

    def _row_bytes(self, mp: MixedPlan) -> int:
        """Bytes per row of c's arena plus the mixed arena (with the shape-generic form's block between the stages)."""
        n = sum(l.num_folds * l.num_output_units for l in self.plan.layers)
        for m in mp.layers:
            l = self.plan.layers[m.layer]
            n += len(m.folds) * (self.graph.units(l) ** 2 + (0 if self._special(l) else l.num_input_units * l.num_output_units))
        n += sum(len(lf.folds) * self.graph.units(self.plan.layers[lf.layer]) ** 2 for lf in mp.leaves)  # the weighted Gram blocks
        return n * self._esize

    @staticmethod
    def _special(l) -> bool:
        return l.type == "hadamard" or (l.num_input_units == 32 and l.num_output_units in (1, 32))

    def rows_per_chunk(self, integrate_vars=None) -> int:
        """How many rows one chunk of `log_marginal` holds by default: c's arena plus the mixed arena at or below 2 GiB."""
        return max(1, _CHUNK_BYTES // self._row_bytes(self.classify(integrate_vars)))

    def child(self, p: int, g: int, K: int, B: int, cls: int, tb: MixedTables | None, bd_c, bd_z) -> tuple[int, int]:
        """(kind, element offset) of fold `g` of layer `p`, of class `cls`, read at `K` units and batch size `B` by a launch of any
        of the queries: FULL in the mixed arena of `tb` where the mixed pass evaluated it, else RANK-1 in c's arena where it is
        OBSERVED, else CONST in the arena of the partition-function circuit."""
        if self.graph.units(self.plan.layers[p]) != K:
            raise ValueError("a layer's children do not all have its number of input units")
        off = None if tb is None else tb.offset(p, g)
        if off is not None:
            return capi.CK_SQ_FULL, off
        if cls == OBSERVED:
            return capi.CK_SQ_RANK1, bd_c.views[p].storage_offset() + g * B * K
        return capi.CK_SQ_CONST, bd_z.views[self._z_of[p]].storage_offset() + g * K * K

    def _tables(self, mp: MixedPlan, B: int, bd_c, bd_z, alloc: bool = True) -> MixedTables:
        """Device tables of a mask at batch size B: per launch (kind, off, wfold), and the mixed arena's layout."""
        key = (B, bd_c.arena.data_ptr(), bd_z.arena.data_ptr(), alloc)  # (an entry without buffers never serves a caller that needs them)
        hit = mp.dev.get(B)
        if hit is not None and hit.key == key:
            return hit
        dt = torch.complex64 if self._complex else torch.float32
        tb = MixedTables(key, [], {}, 0, 0, None, None)
        for m in mp.layers:
            l = self.plan.layers[m.layer]
            ko2 = self.graph.units(l) ** 2
            tb.where.update(((m.layer, int(f)), tb.total + j * B * ko2) for j, f in enumerate(m.folds))
            tb.total += (len(m.folds) * B * ko2 + 3) // 4 * 4
            if not self._special(l):
                tb.mid_size = max(tb.mid_size, len(m.folds) * B * l.num_input_units * l.num_output_units)
        if mp.leaves:
            from .squared_soft import bind_leaves

            bind_leaves(self, mp, tb, B)
        for m in mp.layers:
            l = self.plan.layers[m.layer]
            rows = [[self.child(p, g, l.num_input_units, B, mp.classes[p][g], tb, bd_c, bd_z) for p, g in self.graph.children[m.layer][f].tolist()]
                    for f in m.folds]
            kind, off = np.asarray(rows, dtype=np.int64).reshape(len(m.folds), l.arity, 2).transpose(2, 0, 1)
            tb.launches.append(MixedLaunch(
                m.layer, len(m.folds), l.arity, l.num_input_units, l.num_output_units, 0 if l.type == "hadamard" else 2, tb.where[(m.layer, int(m.folds[0]))],
                torch.from_numpy(np.ascontiguousarray(kind, dtype=np.int32)).to(self.device), torch.from_numpy(np.ascontiguousarray(off)).to(self.device),
                torch.from_numpy(m.folds.astype(np.int32)).to(self.device)))
        tb.total = max(tb.total, 1)
        if alloc:
            tb.arena = torch.empty(tb.total, dtype=dt, device=self.device)
            tb.mid = torch.empty(tb.mid_size, dtype=dt, device=self.device) if tb.mid_size else None
        return put_bounded(mp.dev, B, tb, 2)

    def _stage_weights(self, layer: int, Ko: int, Ki: int):
        """The real (F, Ko, Ki) weight blocks of the two TensorDot stages of a sum / CP-T layer of ``c``."""
        zl = self._z_of[layer]
        w1, w2 = self.z.layers[zl - 1]._w, self.z.layers[zl]._w
        for w in (w1, w2):
            if w is None or w.dtype != torch.float32 or not w.is_contiguous() or tuple(w.shape[-2:]) != (Ko, Ki):
                raise NotImplementedError("HipSquaredCircuit: sum weights that are not real (F, Ko, Ki) blocks")
        return w1, w2

    def _launch_mixed(self, launches, arena, mid, bd_c, bd_z, B: int) -> int:
        """The launches of `_tables` into `arena`, in order; how many there were."""
        esz = self._esize
        stream = torch.cuda.current_stream(self.device).cuda_stream
        with torch.cuda.device(self.device):
            for la in launches:
                w1, w2 = self._stage_weights(la.layer, la.Ko, la.Ki) if la.stages else (None, None)
                capi.call("ck_squared_mixed_fwd", arena.data_ptr(), bd_z.arena.data_ptr(), bd_c.arena.data_ptr(), la.kind.data_ptr(),
                          la.off.data_ptr(), la.H, None if w1 is None else w1.data_ptr(), None if w2 is None else w2.data_ptr(),
                          la.wfold.data_ptr(), None if mid is None else mid.data_ptr(), arena.data_ptr() + la.base * esz,
                          la.n, B, la.Ki, la.Ko, la.stages, self.rows_per_block, 1 if self._complex else 0, stream)
        return len(launches)

    def _chunk(self, x: torch.Tensor, mp: MixedPlan) -> torch.Tensor:
        """Unnormalised log marginal of the (cleaned) rows x."""
        B = int(x.shape[0])
        rc, rl, rf = mp.root
        if rc == INTEGRATED:
            return self._root_of_z().expand(B).clone()
        bd_c = self.c._run(x)
        if rc == OBSERVED:
            y = bd_c.views[rl][rf, :, 0]
            return 2 * (y.real if self._complex else y).to(torch.float32)
        bd_z = self._z_binding()
        tb = self._tables(mp, B, bd_c, bd_z)
        self.last_launches += self._launch_mixed(tb.launches, tb.arena, tb.mid, bd_c, bd_z, B)
        return self._mixed_root(tb, mp, B).clone()

    def _mixed_root(self, tb: MixedTables, mp: MixedPlan, B: int) -> torch.Tensor:
        """(B,) fp32: the MIXED output fold as the last launch of the mixed pass left it -- the unnormalised log evidence."""
        last, (_, rl, rf) = tb.launches[-1], mp.root
        if last.layer != rl:
            raise RuntimeError("HipSquaredCircuit: the output fold is not in the last evaluated layer")
        y = tb.arena[last.base: last.base + last.n * B * last.units2].view(last.n, B, last.units2)[rf, :, 0]
        return (y.real if self._complex else y).to(torch.float32)

    def _clean(self, x: torch.Tensor, ignored: np.ndarray) -> tuple[torch.Tensor, torch.Tensor]:
        """x on the device -- fp32 for Gaussian inputs, else int64 -- with 0 where it is ignored or absent (NaN for Gaussian
        inputs, else negative); (B,) bool: the rows with an absent OBSERVED entry."""
        D = self.plan.num_variables
        if x.dim() != 2 or x.shape[1] != D:
            raise ValueError(f"expected x of shape (B, {D}), found {tuple(x.shape)}")
        floating = self.c._float_input
        x = x.to(self.device).to(torch.float32 if floating else torch.int64)
        mask = torch.from_numpy(ignored).to(self.device)
        absent = torch.isnan(x) if floating else x < 0
        return torch.where(mask | absent, torch.zeros((), dtype=x.dtype, device=self.device), x).contiguous(), (absent & ~mask).any(dim=1)

    @staticmethod
    def _chunk_rows(rows_per_chunk, row_bytes) -> int:
        """Rows evaluated at a time: as asked, else what `row_bytes()` bytes per row let into 2 GiB."""
        step = int(rows_per_chunk) if rows_per_chunk is not None else max(1, _CHUNK_BYTES // row_bytes())
        if step <= 0:
            raise ValueError("rows_per_chunk must be positive")
        return step

    def _leaf_table(self, layer: int) -> tuple[torch.Tensor, int, int, int]:
        """(table, C, K, 1 for a table of logarithms) of an input layer of ``c`` -- after c's forward, which builds the tables."""
        table = self.c.layers[layer]._table
        if table.dtype != torch.float32 or not table.is_contiguous():
            raise NotImplementedError("HipSquaredCircuit: an input table that is not real fp32")
        return table, int(table.shape[1]) - 1, int(table.shape[2]), 1 if self.plan.layers[layer].type == "categorical" else 0

    def log_marginal(self, x: torch.Tensor, integrate_vars=None, *, normalized: bool = True, rows_per_chunk: int | None = None) -> torch.Tensor:
        """``(B,)`` fp32: ``log integral of |c(x_O, x_M)|^2 dx_M`` over the variables ``M = integrate_vars`` (an iterable of
        ids or a ``(D,)`` / ``(1, D)`` bool mask; one mask per call), minus ``log Z`` when `normalized`.  Entries of ``x`` at
        integrated variables are ignored; a negative entry (NaN for Gaussian inputs) at an OBSERVED variable makes that row
        NaN.  With no mixed fold -- nothing or everything integrated -- nothing beyond ``c``'s forward / the partition function
        is launched.  `rows_per_chunk`: rows evaluated at a time (default: c's arena plus the mixed arena within 2 GiB); the
        results do not depend on it."""
        D = self.plan.num_variables
        if x.dim() != 2 or x.shape[1] != D:  # (before a mask is refused)
            raise ValueError(f"expected x of shape (B, {D}), found {tuple(x.shape)}")
        mp = self.classify(integrate_vars)
        x, bad = self._clean(x, _mask_of(integrate_vars, D))
        B = int(x.shape[0])
        step = self._chunk_rows(rows_per_chunk, lambda: self._row_bytes(mp))
        self.last_launches = 0
        out = torch.empty(B, dtype=torch.float32, device=self.device)
        for r0 in range(0, B, step):
            out[r0: r0 + step] = self._chunk(x[r0: r0 + step], mp)
        if normalized:
            out = out - self._root_of_z()
        return torch.where(bad, torch.full((), float("nan"), device=self.device), out)

    def conditional_log_prob(self, x: torch.Tensor, query_vars, integrate_vars=None, *, rows_per_chunk: int | None = None) -> torch.Tensor:
        """``(B,)``: ``log p(x_Q | x_O)`` with ``M = integrate_vars`` integrated out and ``O`` the rest:
        ``log_marginal(x, M) - log_marginal(x, M + Q)``, both unnormalised."""
        D = self.plan.num_variables
        m = _mask_of(integrate_vars, D)
        q = _mask_of(query_vars, D, "query")
        if not q.any():
            raise ValueError("conditional_log_prob needs at least one query variable")
        if (q & m).any():
            raise ValueError("a query variable cannot be integrated out")
        num = self.log_marginal(x, torch.from_numpy(m), normalized=False, rows_per_chunk=rows_per_chunk)
        den = self.log_marginal(x, torch.from_numpy(m | q), normalized=False, rows_per_chunk=rows_per_chunk)
        return num - den

    # -- all states of one variable, sampling (cirkit_amd/squared_sampling.py) ---------------------------------------------------
    def state_log_marginals(self, x: torch.Tensor, var: int, integrate_vars=None, *, normalized: bool = True,
                            rows_per_chunk: int | None = None) -> torch.Tensor:
        """``(B, C)`` fp32: ``log integral of |c(x_O, X_var = s, x_M)|^2 dx_M`` for every state ``s`` of `var` at once, minus
        ``log Z`` when `normalized` -- row ``b``, column ``s`` is ``log_marginal`` of row ``b`` with ``x_var = s``, from ONE launch
        on top of ``c``'s forward (and the mixed launches of the folds beside the path of `var`, `last_mixed_launches`).
        `integrate_vars` as in `log_marginal`, without `var`.  The entry of ``x`` at `var` is ignored; a negative entry at an
        observed variable makes the row NaN.  ``NotImplementedError`` for Gaussian inputs and for a variable whose ancestry
        is not a path (a DAG region graph).

        Accuracy: a state is a sum of ``K^2`` signed terms in fp32 and is accurate to about 1e-5 OF ITS ROW'S LARGEST STATE,
        not of itself -- all a sampler or a normalised posterior needs, but the LOGARITHM of a state that holds ``e^-g`` of the
        largest has a relative error of about ``e^g 1e-5``: within ``1e-4 |log m|`` down to ``e^-4`` of the largest, unreliable
        below about ``e^-6`` (most states of a 256-state posterior on real images).  Where the logarithm of such a state
        matters, take `log_marginal` with ``x_var = s``, one call per state ("Sampling squared circuits")."""
        from .squared_sampling import state_log_marginals

        return state_log_marginals(self, x, var, integrate_vars, normalized=normalized, rows_per_chunk=rows_per_chunk)

    def posterior(self, x: torch.Tensor, var: int, integrate_vars=None, *, rows_per_chunk: int | None = None) -> torch.Tensor:
        """``(B, C)``: ``log p(X_var = s | x_O)`` with `integrate_vars` integrated out: `state_log_marginals` normalised over
        ``s``, with its accuracy: the probabilities are right to about 1e-5 absolute, so the logarithm of a state far below the
        most probable one (``e^-6`` of it or less) is not; `conditional_log_prob`, one call per state, is there for those."""
        from .squared_sampling import posterior

        return posterior(self, x, var, integrate_vars, rows_per_chunk=rows_per_chunk)

    # -- all states of every query variable at once (cirkit_amd/squared_posterior.py) -----------------------------------------------
    def query_log_marginals(self, x: torch.Tensor, query_vars, integrate_vars=None, *, normalized: bool = True,
                            return_log_evidence: bool = False, rows_per_chunk: int | None = None):
        """``(B, |Q|, C)`` fp32: for every query variable ``v`` (the ``Q`` axis in ascending variable order) and every state ``s``,
        ``log integral of |c(x_O, X_v = s, x_{M - v})|^2`` with ``M = Q + integrate_vars`` integrated out and ``O`` the rest observed
        -- what `state_log_marginals(x, v, M - v)` returns, for all of ``Q`` from ONE pass down the folds above ``Q`` on top of
        ``c``'s forward and the mixed launches (`last_mixed_launches`, `last_down_launches`) -- minus ``log Z`` when `normalized`.
        ``C`` is the largest number of states among the query variables; columns past a variable's own count are ``-inf``.
        `return_log_evidence`: also ``(B,)`` `log_marginal(x, Q + integrate_vars)` with the same `normalized` (the root of the
        mixed pass: it costs nothing).  `query_vars` / `integrate_vars` in the forms `log_marginal` takes, one set each per call;
        entries of ``x`` at ``M`` are ignored, a negative entry at an observed variable makes the row NaN.  ``ValueError`` for an
        empty ``Q`` or one that meets `integrate_vars`; ``NotImplementedError`` for Gaussian inputs and DAG ancestries, as
        `state_log_marginals`, whose accuracy it shares: right to about 1e-5 of the row's largest state.  The results do not
        depend on `rows_per_chunk` or `rows_per_block`."""
        from .squared_posterior import query_log_marginals

        return query_log_marginals(self, x, query_vars, integrate_vars, normalized=normalized, return_log_evidence=return_log_evidence,
                                   rows_per_chunk=rows_per_chunk)

    def posterior_marginals(self, x: torch.Tensor, query_vars, integrate_vars=None, *, return_log_evidence: bool = False,
                            rows_per_chunk: int | None = None):
        """``(B, |Q|, C)``: ``log p(X_v = s | x_O)`` for every ``v`` in `query_vars` with the other query variables and
        `integrate_vars` integrated out: `query_log_marginals` normalised over ``s`` per ``(b, v)``, in log space like `posterior`
        (and with its accuracy).  `return_log_evidence`: also ``(B,)`` ``log p(x_O)``."""
        from .squared_posterior import posterior_marginals

        return posterior_marginals(self, x, query_vars, integrate_vars, return_log_evidence=return_log_evidence, rows_per_chunk=rows_per_chunk)

    # -- every variable given all the others (cirkit_amd/squared_loo.py) -------------------------------------------------------------
    def leave_one_out_log_marginals(self, x: torch.Tensor, query_vars=None, *, normalized: bool = True,
                                    rows_per_chunk: int | None = None) -> torch.Tensor:
        """``(B, |Q|, C)`` fp32: ``log |c(x_{-v}, X_v = s)|^2`` for every query variable ``v`` (the ``Q`` axis in ascending variable
        order; None: every variable) and every state ``s``, with EVERY other entry of the row observed, the other query variables
        included -- `log_prob` of the row with ``x_v = s``, for all ``v`` and ``s`` from one K-sized derivative pass over ``c`` itself on
        top of ``c``'s forward (`last_loo_launches`: one launch per layer with a fold above ``Q``, one for the leaves) -- minus
        ``log Z`` when `normalized`.  ``C`` is the largest number of states among the query variables; columns past a variable's
        own count are ``-inf``.  A negative entry anywhere in a row, at a query variable too, makes that row NaN.  ``ValueError``
        for an empty ``Q``; ``NotImplementedError`` for Gaussian inputs and DAG ancestries, before anything is allocated.  The
        results do not depend on `rows_per_chunk`.  Accuracy: a state is a sum of ``K`` signed terms, right to about 1e-6 of its
        row's largest state ("Leave-one-out conditionals of squared circuits").

        Out of scope: integrated variables (the derivative is then not rank-1: `posterior_marginals`), per-row masks, fusing the
        pass with ``c``'s forward."""
        from .squared_loo import leave_one_out_log_marginals

        return leave_one_out_log_marginals(self, x, query_vars, normalized=normalized, rows_per_chunk=rows_per_chunk)

    def leave_one_out(self, x: torch.Tensor, query_vars=None, *, rows_per_chunk: int | None = None) -> torch.Tensor:
        """``(B, |Q|, C)``: ``log p(X_v = s | x_{-v})``, `leave_one_out_log_marginals` normalised over ``s`` inside the leaf launch.
        A (row, variable) without any leave-one-out mass is NaN."""
        from .squared_loo import leave_one_out

        return leave_one_out(self, x, query_vars, rows_per_chunk=rows_per_chunk)

    def conditional_log_probs(self, x: torch.Tensor, *, rows_per_chunk: int | None = None) -> torch.Tensor:
        """``(B, D)``: ``log p(x_v | x_{-v})`` of every entry of every row, without the ``(B, D, C)`` table; ``.sum(1)`` is the
        pseudo-log-likelihood.  An observed state without mass is ``-inf``; a (row, variable) without any leave-one-out mass, and
        every entry of a row with a negative entry, is NaN."""
        from .squared_loo import conditional_log_probs

        return conditional_log_probs(self, x, rows_per_chunk=rows_per_chunk)

    # -- a weight per state, a box (cirkit_amd/squared_soft.py) ------------------------------------------------------------------------
    def soft_evidence_log_prob(self, log_lik: torch.Tensor, x: torch.Tensor | None = None, *, soft_vars=None, integrate_vars=None,
                               normalized: bool = True, rows_per_chunk: int | None = None) -> torch.Tensor:
        """``(B,)`` fp32: ``log sum_{x_S, x_M} |c(x_O, x_S, x_M)|^2 prod_{v in S} lambda[n, v, x_v]``, minus ``log Z`` when
        `normalized`: soft (likelihood, virtual) evidence on the variables ``S = soft_vars``, ``M = integrate_vars`` integrated out,
        the others observed at ``x``.  `log_lik`: ``(B, |S|, C)`` floating point, ``log lambda``, the ``S`` axis in ascending variable
        order; ``C`` at least the largest state count among ``S``, entries past a variable's own count are never read; ``-inf`` is
        weight 0 (a variable whose read entries are all ``-inf`` makes the row ``-inf``, not NaN); a NaN or ``+inf`` in a read
        entry makes that row alone NaN.  `soft_vars` / `integrate_vars` in the forms `log_marginal` takes, one set each per call
        and disjoint (``ValueError``); `soft_vars` None: every variable not integrated; an empty soft set is a ``ValueError``.
        `x`: required when a variable is in neither set (``ValueError``), ignored at the others; a negative entry at an observed
        variable makes the row NaN.  ``NotImplementedError``, before anything is allocated, for a soft variable under a Gaussian
        layer (Gaussian variables stay hard evidence or integrated).  DAG region graphs are fine: one bottom-up pass, c's
        forward, one `ck_squared_soft_leaf` launch per input layer with a soft fold (`last_soft_launches`) and the mixed launches
        of every fold whose scope meets ``S`` or both ``M`` and its complement (`last_launches`).  The results do not depend on
        `rows_per_chunk` (default: c's arena plus the mixed arena, ``|S| K^2`` values per row for the leaves alone, within 2 GiB)
        or `rows_per_block`.

        Posteriors and sampling under the same evidence: `soft_posterior_marginals`, `sample_soft`.  Out of scope: MPE under soft
        evidence, fusing the leaf Gram into the first product layer, the Gram's symmetry, Gaussian boxes, per-row soft sets,
        gradients."""
        from .squared_soft import soft_evidence_log_prob

        return soft_evidence_log_prob(self, log_lik, x, soft_vars=soft_vars, integrate_vars=integrate_vars, normalized=normalized,
                                      rows_per_chunk=rows_per_chunk)

    # -- posteriors and sampling under soft evidence (cirkit_amd/squared_soft_posterior.py) ------------------------------------------
    def soft_query_log_marginals(self, log_lik: torch.Tensor, x: torch.Tensor | None = None, *, soft_vars=None, integrate_vars=None,
                                 normalized: bool = True, return_log_evidence: bool = False, rows_per_chunk: int | None = None):
        """``(B, |S|, C_max)`` fp32: for every soft variable ``v`` (the ``S`` axis in ascending variable order) and every state ``s``,
        ``log lambda_v(s) + log sum_{x: x_v = s} |c(x)|^2 prod_{u in S - v} lambda_u(x_u)`` with `integrate_vars` summed out and the
        rest observed at ``x``, minus ``log Z`` when `normalized`: the joint of ``X_v = s`` and the soft evidence.  ``C_max`` is the
        largest state count among ``S``; columns past a variable's own count are ``-inf``.  `return_log_evidence`: also ``(B,)``
        what `soft_evidence_log_prob` returns, from the root of the same pass at no extra launch.  `log_lik`, the sets, `x`, the
        refusals and the NaN rows as in `soft_evidence_log_prob`; in addition ``NotImplementedError`` for Gaussian inputs and, as
        `posterior_marginals`, for a soft variable read by several input folds or below a fold with several readers (DAG region
        graphs).  One pass: ``c``'s forward, the leaf Gram launches (`last_soft_launches`), the mixed launches (`last_launches`), one
        `ck_squared_down_bwd` per layer with a fold above ``S`` and one `ck_squared_soft_down_leaf` (`last_down_launches`).  The
        results do not depend on `rows_per_chunk` (default: c's arena, the mixed arena with its leaf blocks and the down arena
        within 2 GiB) or `rows_per_block`.  Accuracy as `query_log_marginals`: right to about 1e-5 of the row's largest state.

        Out of scope: MPE under soft evidence (not tractable here), variables without a weight (pass ``log_lik = 0`` for them),
        boxes read from their bounds (pass 0 / ``-inf`` weights), per-row soft sets, Gaussian inputs, gradients."""
        from .squared_soft_posterior import soft_query_log_marginals

        return soft_query_log_marginals(self, log_lik, x, soft_vars=soft_vars, integrate_vars=integrate_vars, normalized=normalized,
                                        return_log_evidence=return_log_evidence, rows_per_chunk=rows_per_chunk)

    def soft_posterior_marginals(self, log_lik: torch.Tensor, x: torch.Tensor | None = None, *, soft_vars=None, integrate_vars=None,
                                 return_log_evidence: bool = False, rows_per_chunk: int | None = None):
        """``(B, |S|, C_max)``: ``log p(X_v = s | lambda, x_O)`` for every soft variable at once: `soft_query_log_marginals`
        normalised over ``s`` per ``(b, v)``.  A (row, variable) without mass is NaN.  `return_log_evidence`: also ``(B,)`` the
        normalised log evidence of `soft_evidence_log_prob`."""
        from .squared_soft_posterior import soft_posterior_marginals

        return soft_posterior_marginals(self, log_lik, x, soft_vars=soft_vars, integrate_vars=integrate_vars,
                                        return_log_evidence=return_log_evidence, rows_per_chunk=rows_per_chunk)

    def sample_soft(self, log_lik: torch.Tensor, x: torch.Tensor | None = None, *, soft_vars=None, integrate_vars=None,
                    seed: int | None = None, order=None, rows_per_chunk: int | None = None) -> torch.Tensor:
        """``(B, D)`` int64: the soft variables of every row drawn exactly from ``p(x_S | lambda, x_O)``, proportional to
        ``|c(x)|^2 prod_v lambda_v(x_v)`` with `integrate_vars` summed out; observed entries are returned untouched, integrated
        columns as given (0 where `x` is None).  With 0 / ``-inf`` weights this is exact truncated sampling.  `order`: a
        permutation of the soft variables (``ValueError`` otherwise; default `tree_order` restricted to them); an order that
        leaves a fold beside a variable's path with some soft variables drawn and others not is a ``NotImplementedError``, raised
        while planning (`tree_order` never does).  `seed` and the Philox counters as `sample_conditional`: the draws depend on the
        seed and the order only.  A row without mass, with an absent observed entry or with a NaN / ``+inf`` among its read weights
        gets -1 in every soft column.  Per chunk one soft bottom-up pass (`last_soft_launches`, `last_launches`), then per variable
        ``c``'s forward and one `ck_squared_path_soft_bwd` launch (`last_mixed_launches`: the steps' own mixed launches, 0 in
        `tree_order` without integrated variables)."""
        from .squared_soft_posterior import sample_soft

        return sample_soft(self, log_lik, x, soft_vars=soft_vars, integrate_vars=integrate_vars, seed=seed, order=order,
                           rows_per_chunk=rows_per_chunk)

    def interval_log_prob(self, lo: torch.Tensor, hi: torch.Tensor, x: torch.Tensor | None = None, *, box_vars=None, integrate_vars=None,
                          normalized: bool = True, rows_per_chunk: int | None = None) -> torch.Tensor:
        """``(B,)`` fp32: the log mass of the box ``lo <= x_v <= hi`` over ``v in box_vars`` (inclusive on both sides), with
        `integrate_vars` integrated out and the others observed at ``x`` -- the 0/1 case of `soft_evidence_log_prob`, read from the
        bounds themselves by the same leaf launch: no ``(B, S, C)`` tensor is built and the states outside a row's bounds are
        skipped.  `lo`, `hi`: ``(B, D)`` integer, read at `box_vars` only and clamped into ``0 .. C_v - 1``; an empty interval
        gives ``-inf``; ``lo < 0 and hi < 0`` means the full range, `HipCircuit.interval_log_prob`'s sentinel.  `box_vars` None:
        every variable not integrated.  Sets, `x`, refusals, chunking and the launch counters as in `soft_evidence_log_prob`."""
        from .squared_soft import interval_log_prob

        return interval_log_prob(self, lo, hi, x, box_vars=box_vars, integrate_vars=integrate_vars, normalized=normalized,
                                 rows_per_chunk=rows_per_chunk)

    def log_cdf(self, x: torch.Tensor, *, integrate_vars=None, rows_per_chunk: int | None = None) -> torch.Tensor:
        """``(B,)``: ``log P(X_v <= x_v for every v not integrated)``: `interval_log_prob` of ``[0, x]`` over all those variables,
        normalised."""
        from .squared_soft import log_cdf

        return log_cdf(self, x, integrate_vars=integrate_vars, rows_per_chunk=rows_per_chunk)

    def sample(self, num_samples: int, *, seed: int | None = None, order=None, rows_per_chunk: int | None = None) -> torch.Tensor:
        """``(N, D)`` int64 exact samples of ``p(x) = |c(x)|^2 / Z``, one variable after the other: `order` (a permutation of
        the variables; default `squared_sampling.tree_order`, in which a step is ``c``'s forward plus one launch and
        `last_mixed_launches` stays 0).  `seed`: the 64-bit Philox key (None: drawn from torch's CPU generator); the draw of
        variable v in row n takes counter (n, global fold id of v's input fold), so the samples depend on the seed and the
        order only: not on `rows_per_chunk` or `rows_per_block`.  Nothing waits for the device between the steps."""
        from .squared_sampling import sample

        return sample(self, num_samples, seed=seed, order=order, rows_per_chunk=rows_per_chunk)

    def sample_conditional(self, x: torch.Tensor, sample_vars, *, seed: int | None = None, order=None,
                           rows_per_chunk: int | None = None) -> torch.Tensor:
        """``(B, D)`` int64: the variables `sample_vars` (the forms `integrate_vars` takes; one set per call) of every row drawn
        exactly from ``p(x_S | x_O)``; observed entries are returned untouched.  `order`: a permutation of the sampled
        variables (``ValueError`` otherwise; default `tree_order` restricted to them).  An entry at a sampled variable is
        ignored whatever it holds.  A row whose evidence has no mass gets -1 in every sampled column.

        DIFFERENT from `HipCircuit.sample_conditional`: there a negative entry of ``x`` marks, row by row, one more variable to
        draw.  Here the sampled set is ONE per call (which folds are mixed is a property of the call), so a negative entry at
        a variable outside `sample_vars` cannot be drawn as well: it is absent evidence, and that row gets -1 in every sampled
        column (its other entries come back as given).  To draw it, put the variable into `sample_vars`."""
        from .squared_sampling import sample_conditional

        return sample_conditional(self, x, sample_vars, seed=seed, order=order, rows_per_chunk=rows_per_chunk)

    # -- the chain rule along an order, coding (cirkit_amd/squared_autoregressive.py) ----------------------------------------------
    def autoregressive_conditionals(self, x: torch.Tensor, order=None, *, positions=None, integrate_vars=None,
                                    rows_per_chunk: int | None = None) -> torch.Tensor:
        """``(B, P, C)`` fp32: ``[b, j, s] = log p(X_{order[i]} = s | x_{order[:i]})`` at ``i = positions[j]``, every row
        normalised over ``s`` by its own logsumexp as `posterior` does; columns past a variable's own state count are -inf.
        `order`: a permutation of the variables outside `integrate_vars` (``ValueError`` otherwise; default `tree_order`
        restricted to them); `integrate_vars`: one set per call, integrated out at every step; `positions`: the steps wanted
        (None: all; ids, a range or a bool mask over the steps).  Per chunk of rows ONE forward of ``c`` and, in `tree_order`,
        ONE launch over (row, step) (`last_mixed_launches` stays 0); a step whose siblings the order splits runs its mixed
        launches and its own launch.  A row with a negative or out-of-range entry at a variable that a selected step observes
        is NaN in every entry; a prefix without mass gives NaN.  Accuracy: that of `posterior`.  The results do not depend
        on `rows_per_chunk` or `rows_per_block`.  ``NotImplementedError``: Gaussian inputs, ancestries that are not paths."""
        from .squared_autoregressive import autoregressive_conditionals

        return autoregressive_conditionals(self, x, order, positions=positions, integrate_vars=integrate_vars, rows_per_chunk=rows_per_chunk)

    def autoregressive_log_probs(self, x: torch.Tensor, order=None, *, positions=None, integrate_vars=None,
                                 rows_per_chunk: int | None = None) -> torch.Tensor:
        """``(B, P)`` fp32: ``log p(x_{order[i]} | x_{order[:i]})`` of the row's own states, formed inside the leaf as
        ``log m(x_v) - logsumexp_s log m(s)``: no ``(B, P, C)`` tensor exists.  Over all steps the columns sum to
        ``log_prob(x)`` (nothing integrated).  Arguments, refusals and edge rows as `autoregressive_conditionals`; the entry at
        the last selected step's own variable is read too."""
        from .squared_autoregressive import autoregressive_log_probs

        return autoregressive_log_probs(self, x, order, positions=positions, integrate_vars=integrate_vars, rows_per_chunk=rows_per_chunk)

    def coding_tables(self, x: torch.Tensor, order=None, *, positions=None, integrate_vars=None, precision: int = 16,
                      rows_per_chunk: int | None = None) -> torch.Tensor:
        """``(B, P, C + 1)`` int32 cumulative frequency tables of `autoregressive_conditionals` at ``2**precision`` counts, the
        contract of `HipCircuit.coding_tables`: ``[..., 0] = 0``, ``[..., C] = 2**precision``, every state of the step's
        variable at least one count (`ck_ar_quantise` on ``exp`` of the conditionals, a chunk of steps at a time).  A NaN row
        gets the uniform table.  What cirkit_amd/codec.py codes with."""
        from .squared_autoregressive import coding_tables

        return coding_tables(self, x, order, positions=positions, integrate_vars=integrate_vars, precision=precision,
                             rows_per_chunk=rows_per_chunk)
