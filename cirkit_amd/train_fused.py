"""The FUSED form of `HipTrainer`'s step (cirkit_amd/training.py, module docstring): qualification of a plan, the tables of its
backward that depend on the plan alone (`FusedTables`), what one batch size adds to them (`FusedBinding`, owned by the layer-wise
backward binding and rebuilt with it when the circuit's arena moves), and the backward launch list.

The forward is the circuit's own (`HipCircuit.log_likelihood_sum` with `keep_levels`); `HipTrainer` decides between the forms."""

from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import _capi as capi
from .circuit import HipCircuit
from .fusion import SubtreeGroup, balanced_segments, interleave_8_apart, leaf_bwd_unit_tables
from .layers import HipCategoricalLayer, HipCPTLayer, HipSumLayer
from .train_leaf import leaf_backward

# one fold of `ck_tail_bwd` and one job of `ck_param_softmax_bwd_batch` (include/cirkit_hip.h)
TAIL_FOLD_DTYPE = np.dtype([("w", "<u8"), ("gout", "<u8"), ("dw_part", "<u8"), ("child", "<u8", 4), ("gchild", "<u8", 4), ("H", "<i4"), ("Ko", "<i4")])
assert TAIL_FOLD_DTYPE.itemsize == 96
SOFTMAX_JOB_DTYPE = np.dtype([("w", "<u8"), ("dw", "<u8"), ("dtheta", "<u8"), ("rows", "<i8"), ("len", "<i4"), ("first", "<i4"),
                              ("part_stride", "<i8"), ("n_part", "<i4"), ("reserved", "<i4"),
                              ("theta", "<u8"), ("m1", "<u8"), ("m2", "<u8"), ("w_out", "<u8")])
assert SOFTMAX_JOB_DTYPE.itemsize == 88


@dataclass(slots=True)
class FusedTables:
    """What the fused backward needs of the plan alone."""
    group: SubtreeGroup
    launches: list[tuple[torch.Tensor, int]]  # top first: (unit table of `ck_leaf_walk_bwd`, level of P)
    fold_order: torch.Tensor  # the Categorical scatter's workgroup -> table fold (folds of one gradient tile 8 apart)
    gfold: torch.Tensor  # table fold -> the level-1 node whose gradient tile it takes
    var: torch.Tensor  # table fold -> its variable


@dataclass(slots=True)
class TailTables:
    """Descriptors of `ck_tail_bwd`: the few-fold layers above the leaf region in ONE backward launch."""
    folds: torch.Tensor  # (n_folds, 96) bytes: TAIL_FOLD_DTYPE rows, top layer first
    n_folds: int
    levels: torch.Tensor  # first fold of every layer, and the end
    n_levels: int
    part: torch.Tensor  # per-tile slots of the layers' weight gradients
    part_of: dict[int, int]  # layer -> address of its slots in `part`
    stride: int
    n_tiles: int


@dataclass(slots=True)
class SoftmaxJobs:
    """The job table of `ck_param_softmax_bwd_batch` over every sum layer but the dense one."""
    table: torch.Tensor  # (n_jobs, 88) bytes: SOFTMAX_JOB_DTYPE rows
    n_blocks: int


@dataclass(slots=True)
class FusedBinding:
    """What one batch size adds: built with the layer-wise backward binding (`HipTrainer._bind_backward`), whose buffers every
    address below points into, and dropped with it."""
    work: list[torch.Tensor]  # per leaf launch: its work segments
    G: list[torch.Tensor]  # per leaf launch: the gradient tiles it leaves for the level below its Q nodes
    dw_sum: torch.Tensor  # the part of the flat linear-gradient buffer that float atomics add to
    tail: TailTables | None  # None: the tail runs layer by layer
    sm_jobs: SoftmaxJobs  # gradients to the flat buffer ...
    sm_jobs_opt: SoftmaxJobs  # ... or the optimizer in the epilogue as well
    seed_gB: float | None = None  # the global batch whose constant seed -1 / gB the output's gradient block holds


def fused_circuit(plan, store, device, cache_params: bool) -> HipCircuit:
    # (`cache_params`: with the optimizer in the backward epilogues -- `step`, one rank -- the launches that update the logits
    #  write the derived parameters of the next forward themselves; the prologue runs only after the store was changed
    #  from outside)
    return HipCircuit(plan, store, device=device, use_graph=False, fuse=True, batch_params=True, tiled_weights=False,
                      dense_on_table=True, pad_units=False, fused_weight_softmax=False, persistent_leaf=True,
                      params_at_end=False, keep_levels=True, direct_input=True, cache_params=cache_params)


def why_not_fused(c: HipCircuit, plan, fast_softmax) -> str | None:
    """None when the fused circuit `c` of `plan` trains in the fused form, else why not.  `fast_softmax(layer)`: its weights
    are softmax(tensor) evaluated by the batched prologue."""
    if len(c._out_pairs) != 1 or c._signed or len(c._groups) != 1:
        return "needs one output and exactly one fused leaf region"
    g = c._groups[0]
    c._ensure_param_batch()
    cat = c.layers[g.input_layer]
    if g.depth not in (2, 4) or g.dense_layer is None or g.root not in c._table_fused or not c.linear_levels:
        return "the leaf region must be Categorical -> dense -> 2 or 4 CP-T levels with the table built by one prologue job"
    if not isinstance(cat, HipCategoricalLayer) or cat.num_output_units != 32 or cat.num_categories > 256:
        return "the leaf region needs a 32-unit Categorical input layer of at most 256 categories"
    covered = set(g.virtual) | {g.root} | set(c._tail)
    if covered != set(range(len(c.layers))) or c._tdense or c._cp_blocks or c._regions or c._input_prod:
        return "layers outside the leaf region and the tail"
    if c._tail and not c._tail16_ok():
        return "the tail does not fit the 16-row walk"
    for j in list(g.levels) + [g.dense_layer] + list(c._tail):
        l = c.layers[j]
        if not (isinstance(l, (HipSumLayer, HipCPTLayer)) and type(l) in (HipSumLayer, HipCPTLayer) and fast_softmax(l)
                and l.num_input_units == 32):
            return f"layer {j}: weights must be softmax(tensor) over 32 inputs"
    for j in g.levels:
        if c.layers[j].num_output_units != 32 or c.layers[j].arity != 2:
            return "fused levels must be binary CP-T layers of 32 units"
    if cat.probs is None or cat.probs.softmax_source() is None:
        return "Categorical layers need probs = softmax(tensor)"
    leaf_of_dense = c._children[g.dense_layer][:, 0, 1].astype(np.int64)
    if not np.array_equal(leaf_of_dense, np.arange(cat.num_folds)):
        return "the dense layer must read the Categorical folds in order"
    Cn = cat.num_categories
    if (((Cn + 1 + 31) // 32) + 3) * 4096 + 8 * 4096 > 160 * 1024:
        return "too many categories for the table backward's LDS"
    # every parameter gradient of the fused backward is WRITTEN, exactly once, by the launch that owns its tensor (nothing
    # zeroes the flat gradient): the tensors behind the Categorical table, the dense layer, the levels and the tail must be
    # pairwise distinct and cover the plan's tensors
    owned = [cat.probs.graph.nodes[0].config["tensor"]] + [
        c.layers[j].weight.graph.nodes[0].config["tensor"] for j in [g.dense_layer] + list(g.levels) + list(c._tail)]
    if len(set(owned)) != len(owned) or set(owned) != set(plan.tensors):
        return "parameter tensors shared between layers (or not reached by any layer)"
    return None


def build_tables(c: HipCircuit) -> FusedTables:
    """The unit tables of the leaf-walk backward, the scatter tables and the scatter's fold order of a qualified circuit."""
    g = c._groups[0]
    dev = c.device
    cat, dl = c.layers[g.input_layer], c.layers[g.dense_layer]
    kl = 1 << g.depth
    nodes = np.asarray(g.nodes).astype(np.int64)
    n_roots = c.layers[g.root].num_folds
    off = [int(v) for v in g.node_off]
    var_of_leaf = cat.scope_idx[:, 0].astype(np.int64)
    launches = [(torch.from_numpy(tab).to(dev), top) for tab, top in leaf_bwd_unit_tables(g, n_roots, var_of_leaf)]
    # Categorical scatter: table fold d takes the gradient tile of the level-1 node above it
    gfold = np.zeros(dl.num_folds, dtype=np.int32)
    var_of_table = np.zeros(dl.num_folds, dtype=np.int64)
    for t in range(n_roots):
        for i in range(kl):
            d = int(nodes[off[0] + t * kl + i])
            gfold[d] = int(nodes[off[1] + t * (kl >> 1) + (i >> 1)])
            var_of_table[d] = var_of_leaf[int(nodes[g.leaf_off + t * kl + i])]
    # the two leaves under a level-1 node read the same gradient tile: their workgroups are placed 8 apart (same XCD, same time)
    by_tile: dict[int, list[int]] = {}
    for d in range(dl.num_folds):
        by_tile.setdefault(int(gfold[d]), []).append(d)
    fold_order = [d for d in interleave_8_apart(list(by_tile.values())) if d >= 0]  # (ragged groups: the holes close up)
    assert sorted(fold_order) == list(range(dl.num_folds))
    return FusedTables(group=g, launches=launches, fold_order=torch.from_numpy(np.asarray(fold_order, dtype=np.int32)).to(dev),
                       gfold=torch.from_numpy(gfold).to(dev), var=torch.from_numpy(var_of_table).to(dev))


class FusedStep:
    """The fused form of a `HipTrainer`: `why` is None and `circuit` / `tables` are set, or `why` says why the plan does not
    qualify."""

    def __init__(self, tr, store, device) -> None:
        self.tr, self.circuit, self.tables = tr, None, None
        if tr._pad_info is not None:
            self.why = "padded unit counts"
            return
        c = fused_circuit(tr.plan, store, device, tr._fuse_optimizer)
        self.why = why_not_fused(c, tr.plan, tr._fast_softmax)
        if self.why is not None:
            return
        self.circuit, self.tables = c, build_tables(c)
        # wavefronts per workgroup of the backward walk: 8 = two per SIMD; 4 = one per SIMD with the next unit's tiles in
        # flight (ck_leaf_bwd.hip), within 3 %
        self.waves = int(os.environ.get("CK_BWD_WAVES", "8"))

    # ---- binding -----------------------------------------------------------------------------------------------------
    def bind(self, B: int, bd, st) -> FusedBinding:
        """The fused part of the backward binding `st` (over the forward binding `bd`) at batch size B."""
        c, g = self.circuit, self.tables.group
        dev = c.device
        n_tiles = (B + 31) // 32
        work, G = [], []
        for tab, top in self.tables.launches:
            work.append(torch.from_numpy(balanced_segments(int(tab.shape[0]), n_tiles, c._n_cu, waves=self.waves)).to(dev))
            # the tiles this launch leaves for the level below its Q nodes (one per Q node)
            # (tile-native between two of these launches, row-major where the Categorical scatter reads them)
            nq = c.layers[g.levels[top - 2]].num_folds
            G.append(torch.empty((nq, B, 32) if top == 2 else (nq, n_tiles, 1024), dtype=torch.float32, device=dev))
        # float atomics add to everything in the flat linear-gradient buffer but the table gradient, which the scatter
        # overwrites (it is the last block: the Categorical layer comes first in the plan ... or not)
        dT, flat = st.dws[g.input_layer], st.dw_flat
        lo = (dT.data_ptr() - flat.data_ptr()) // 4
        hi = lo + dT.numel()
        dw_sum = flat[hi:] if lo == 0 else flat[:lo] if hi == flat.numel() else flat
        tail = self._tail_tables(B, bd, st)
        return FusedBinding(work=work, G=G, dw_sum=dw_sum, tail=tail, sm_jobs=self._softmax_jobs(st, tail, False),
                            sm_jobs_opt=self._softmax_jobs(st, tail, True))

    def _tail_tables(self, B: int, bd, st) -> TailTables | None:
        """Descriptors of `ck_tail_bwd` for this binding, or None when a layer does not qualify (then they run layer by layer,
        `HipTrainer._bwd_sum_layer`): CP-T / arity-1 layers of 32 input units and 32 outputs (1 for a scalar root), every child
        read by exactly one fold."""
        c = self.circuit
        layers = list(reversed(c._tail))
        ok = bool(layers) and os.environ.get("CK_TAIL_BWD", "1") != "0"
        for i in layers:
            l = c.layers[i]
            ok = ok and (st.flags[i] == 0 and st.shared.get(i) is None and l.num_input_units == 32 and l.arity <= 2
                         and (l.num_output_units == 32 or (l.num_output_units == 1 and l.num_folds == 1 and i == layers[0]))
                         and (l._mode == capi.CK_SUM_PROD or l.arity == 1) and not l.is_complex and l._w_layout == capi.CK_W_ROWMAJOR)
        if not ok:
            return None
        n_tiles = (B + 31) // 32
        n_folds = sum(c.layers[i].num_folds for i in layers)
        stride = sum(c.layers[i].num_folds * c.layers[i].num_output_units * 32 for i in layers)
        part = torch.empty(n_tiles * stride, dtype=torch.float32, device=c.device)
        tab = np.zeros(n_folds, dtype=TAIL_FOLD_DTYPE)
        level_begin, k, off, part_of = [0], 0, 0, {}
        arena, garena = bd.arena.data_ptr(), st.garena.data_ptr()
        for i in layers:
            l = c.layers[i]
            ro = bd.row_off[i].cpu().numpy().reshape(l.num_folds, l.arity)
            part_of[i] = part.data_ptr() + 4 * off
            wbytes = l.num_output_units * 32 * 4
            for f in range(l.num_folds):
                r = tab[k]
                r["w"] = l._w.data_ptr() + f * wbytes
                r["gout"] = st.gviews[i].data_ptr() + f * B * l.num_output_units * 4
                r["dw_part"] = part_of[i] + f * wbytes
                for h in range(2):  # (a single child is named twice: the launch issues a fixed number of loads and stores)
                    r["child"][h] = arena + 4 * int(ro[f, min(h, l.arity - 1)])
                    r["gchild"][h] = garena + 4 * int(ro[f, min(h, l.arity - 1)])
                r["H"], r["Ko"] = l.arity, l.num_output_units
                k += 1
            off += l.num_folds * l.num_output_units * 32
            level_begin.append(k)
        return TailTables(folds=torch.from_numpy(tab.view(np.uint8).reshape(n_folds, -1)).to(c.device), n_folds=n_folds,
                          levels=torch.from_numpy(np.asarray(level_begin, dtype=np.int32)).to(c.device), n_levels=len(layers),
                          part=part, part_of=part_of, stride=stride, n_tiles=n_tiles)

    def _softmax_jobs(self, st, tail: TailTables | None, with_opt: bool) -> SoftmaxJobs:
        """The jobs of `ck_param_softmax_bwd_batch` over every sum layer of the fused trainer; the tail layers' weight gradients
        are the per-tile slots `ck_tail_bwd` left (summed by that launch) when `tail` is given.  `with_opt`: the jobs also name
        the logits, their moments and the evaluated weights (the optimizer epilogue)."""
        tr, c, g = self.tr, self.circuit, self.tables.group
        layers = list(c._tail) + list(g.levels)  # (the dense layer's is part of ck_table_dense_bwd)
        jt = np.zeros(len(layers), dtype=SOFTMAX_JOB_DTYPE)
        first = 0
        for r, j in zip(jt, layers):
            l = c.layers[j]
            parted = tail is not None and j in tail.part_of
            name = l.weight.graph.nodes[0].config["tensor"]
            r["w"], r["dw"], r["dtheta"] = l._w.data_ptr(), tail.part_of[j] if parted else st.dws[j].data_ptr(), tr.grads[name].data_ptr()
            r["rows"], r["len"], r["first"] = l.num_folds * l.num_output_units, l.num_input_units, first
            r["part_stride"], r["n_part"] = (tail.stride, tail.n_tiles) if parted else (0, 0)
            if with_opt:
                m1, m2 = tr._moments.get(name, (None, None))
                r["theta"], r["w_out"] = c.store[name].data_ptr(), l._w.data_ptr()
                r["m1"], r["m2"] = 0 if m1 is None else m1.data_ptr(), 0 if m2 is None else m2.data_ptr()
            first += (int(r["rows"]) + 3) // 4
        return SoftmaxJobs(table=torch.from_numpy(jt.view(np.uint8).reshape(len(layers), -1)).to(c.device), n_blocks=first)

    # ---- the backward launch list ------------------------------------------------------------------------------------
    def backward(self, B: int, gB: float, seed, bd, st, stream: int, with_opt: bool = False) -> None:
        fb = st.fused
        state = self.tr._opt_state().ptr if with_opt else None  # (its clock of this step: the fill launch at the start of the list)
        self._seed_and_fills(B, gB, seed, st, fb, state, stream)
        self._tail(B, bd, st, fb, stream)
        gin = self._leaf_levels(B, bd, st, fb, stream)
        self._scatter_and_table(B, bd, st, gin, state, stream)
        # softmax parameterisation of every sum layer's weights (tail, fused levels, dense layer): one launch
        jobs = fb.sm_jobs_opt if with_opt else fb.sm_jobs
        capi.call("ck_param_softmax_bwd_batch", jobs.table.data_ptr(), jobs.table.shape[0], jobs.n_blocks, state, stream)

    def _seed_and_fills(self, B: int, gB: float, seed, st, fb: FusedBinding, state, stream: int) -> None:
        tr, c, gviews = self.tr, self.circuit, st.gviews
        # ONE fill: the linear-space weight gradients (float atomics add to them).  The parameter gradients themselves are
        # written, each exactly once, by the parameter backward launches; the table gradient by the scatter.  The launch also
        # turns the validation flag of the forward into this step's flag (`step`: what the optimizer launch skips on)
        # (with the optimizer in the epilogues -- `state`, one rank -- it is the optimizer's clock as well: a flagged step is dropped)
        capi.call("ck_fill_latch", fb.dw_sum.data_ptr(), fb.dw_sum.numel(), 0.0, c._bad_input.data_ptr(),
                  tr._step_flag.data_ptr(), tr._bad_seen.data_ptr(), state, stream)
        for p in st.need_zero:
            if gviews[p] is not None:
                capi.call("ck_fill_f32", gviews[p].data_ptr(), gviews[p].numel(), 0.0, stream)
        po, fo = int(c._out_pairs[0, 0]), int(c._out_pairs[0, 1])
        if c.layers[po].num_output_units != 1:
            raise NotImplementedError("training needs a scalar output unit")
        if gviews[po].numel() != B:
            capi.call("ck_fill_f32", gviews[po].data_ptr(), gviews[po].numel(), 0.0, stream)
        if seed is None:
            # nobody writes this block: the constant seed -1 / gB of the mean log-likelihood is filled once per binding, and again
            # when the caller's global batch changes or a caller-supplied seed has overwritten it
            if fb.seed_gB != float(gB):
                capi.call("ck_fill_f32", gviews[po][fo].data_ptr(), B, -1.0 / gB, stream)
                fb.seed_gB = float(gB)
        else:
            gviews[po][fo].reshape(-1)[:B].copy_(seed.reshape(-1))
            fb.seed_gB = None

    def _tail(self, B: int, bd, st, fb: FusedBinding, stream: int) -> None:
        tail = fb.tail
        if tail is not None:  # the few-fold layers above the leaf region: one launch, a workgroup per 32-row tile
            capi.call("ck_tail_bwd", tail.folds.data_ptr(), tail.n_folds, tail.levels.data_ptr(), tail.n_levels, B, tail.stride, stream)
        else:
            for i in reversed(self.circuit._tail):  # ... or layer by layer
                self.tr._bwd_sum_layer(i, bd, st, B, stream)

    def _leaf_levels(self, B: int, bd, st, fb: FusedBinding, stream: int) -> torch.Tensor:
        """The leaf region (`train_leaf.leaf_backward`); returns the gradient tiles of level 1."""
        tr, c, g = self.tr, self.circuit, self.tables.group
        keep, redo = bd.keep[g.root]
        cat = c.layers[g.input_layer]
        nodes, table, _, scale = c._group_dev[g.root][:4]
        leaf_backward(g, unit_tabs=[tab.data_ptr() for tab, _ in self.tables.launches], tops=[top for _, top in self.tables.launches],
                      works=[w.data_ptr() for w in fb.work], n_segs=[int(w.shape[0]) for w in fb.work],
                      gouts=[G.data_ptr() for G in fb.G], w=[c.layers[j]._w.data_ptr() for j in g.levels],
                      dw=[st.dws[j].data_ptr() for j in g.levels], keep=[None if t is None else t.data_ptr() for t in keep],
                      redo=redo.data_ptr(), table=table.data_ptr(), scale=scale.data_ptr(), x_rows=bd.x_last.data_ptr(),
                      nodes=nodes.data_ptr(), scope=cat._scope(tr.device).data_ptr(), B=B, Cn=cat.num_categories,
                      D=tr.plan.num_variables, n_roots=c.layers[g.root].num_folds, n_wg=c._n_cu, waves=self.waves,
                      gin=st.gviews[g.root].data_ptr(), gin_rowmajor=1, is_signed=0, gin_fold=None, stream=stream)
        return fb.G[-1]

    def _scatter_and_table(self, B: int, bd, st, gin: torch.Tensor, state, stream: int) -> None:
        tr, c, fz = self.tr, self.circuit, self.tables
        g = fz.group
        cat, dl = c.layers[g.input_layer], c.layers[g.dense_layer]
        # leaves: scatter by category into the gradient of the (F0, C + 1, 32) table T' = dense(log-table) ...
        Cn = cat.num_categories
        dTp = st.dws[g.input_layer]
        capi.call("ck_transpose_i64_to_i32", bd.x_last.data_ptr(), bd.xt_i.data_ptr(), B, tr.plan.num_variables, stream)
        capi.call("ck_categorical_bwd", gin.data_ptr(), fz.gfold.data_ptr(), bd.xt_i.data_ptr(), fz.var.data_ptr(),
                  dTp.data_ptr(), dl.num_folds, B, 32, Cn, 0, (fz.fold_order.data_ptr() if B >= 256 else None), stream)
        # ... then the dense layer and the log-softmax of the Categorical layer backward ON THE TABLE (C + 1 rows per fold)
        n_cat, n_dense = cat.probs.graph.nodes[0].config["tensor"], dl.weight.graph.nodes[0].config["tensor"]
        topt = None
        if state is not None:
            # the optimizer in the epilogues (one rank): the launch that
            # holds the gradients of the Categorical and dense logits updates them and writes the next forward's table, the
            # launch that differentiates the weight softmaxes updates those logits and writes the next forward's weights
            topt = capi.TableOpt()
            topt.state = state
            (m1c, m2c), (m1d, m2d) = tr._moments.get(n_cat, (None, None)), tr._moments.get(n_dense, (None, None))
            ph = tr._flat_grad  # (SGD: the moment pointers are never read)
            topt.m1_cat, topt.m2_cat = (ph if m1c is None else m1c).data_ptr(), (ph if m2c is None else m2c).data_ptr()
            topt.m1_dense, topt.m2_dense = (ph if m1d is None else m1d).data_ptr(), (ph if m2d is None else m2d).data_ptr()
            topt.table, topt.table_scale = c._group_dev[g.root][1].data_ptr(), c._group_dev[g.root][3].data_ptr()
        capi.call("ck_table_dense_bwd", cat.probs.softmax_source().data_ptr(), None, dl.weight.softmax_source().data_ptr(),
                  dTp.data_ptr(), tr.grads[n_cat].data_ptr(), tr.grads[n_dense].data_ptr(), dl.num_folds, Cn,
                  None if topt is None else C.byref(topt), stream)
