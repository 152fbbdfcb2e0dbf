"""c(x) of `HipSquaredTrainer` on SIGNED-LOG blocks (cirkit_amd/training_squared.py, module docstring; cirkit_amd/csrc/ck_signed.hip):
which circuits qualify (`_SignedCircuit.why`), what one batch size adds (`SignedBinding`: both arenas, the gather and row-offset
tables of the forward, the routes of the gradients; `LeafBinding`: the tables and buffers of the fused leaf region), and the
forward and backward launch lists, which issue calls of the C ABI only."""

from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Mapping

import numpy as np
import torch

from . import _capi as capi
from .circuit import HipCircuit
from .fusion import SubtreeGroup, balanced_segments, find_subtree_groups, interleave_8_apart, leaf_bwd_unit_tables, leaf_segments
from .layers import HipCPTLayer, HipEmbeddingLayer, HipSumLayer
from .train_leaf import leaf_backward
from .train_reverse import MAX_BOUND, embedding_bwd_fits_lds, state_serials

Parents = dict[tuple[int, int], tuple[int, int]]  # (layer, fold) -> the (layer, fold) that reads it


@dataclass(slots=True)
class GatherTables:
    """What a layer over Embedding folds gathers by: per (fold, child) the Embedding fold and its variable."""
    folds: torch.Tensor
    variables: torch.Tensor
    emb: int  # the Embedding layer


@dataclass(slots=True)
class EmbTables:
    """The signed-log form of an Embedding layer's weight table: (F (C + 1), 32) log|w| and a sign word per row."""
    table: torch.Tensor
    signs: torch.Tensor


@dataclass(slots=True)
class GradRoute:
    """Where the folds of an Embedding layer find the gradient of their output."""
    fold: torch.Tensor  # Embedding fold -> the fold of `reader` whose gradient block it takes
    reader: int  # the layer that gathers from it
    order: torch.Tensor  # workgroup -> Embedding fold (folds that share a block 8 apart)


@dataclass(slots=True)
class LeafLaunchTables:
    """One `ck_leaf_walk_bwd` launch of the leaf region."""
    unit_tab: torch.Tensor
    top: int  # the level of its P nodes
    work: torch.Tensor  # its work segments


@dataclass(slots=True)
class LeafBinding:
    """Descriptors and buffers of the leaf region's launches at one batch size."""
    launches: list[LeafLaunchTables]  # top first
    keep: list[torch.Tensor | None]  # the kept tiles of every second level
    G: list[torch.Tensor | None]  # per backward launch: the gradient tiles it leaves (None: level 1's, in the gradient arena)
    redo: torch.Tensor  # (root, tile) units whose forward walk left the linear range
    nodes: torch.Tensor
    node_off: C.Array
    scope: torch.Tensor
    scale: torch.Tensor
    work: torch.Tensor  # the forward launch's work segments
    n_wg: int
    root_tab: torch.Tensor
    x64: torch.Tensor  # the batch as it came (the leaf launches read it: a copy at a recorded address)
    gin_fold: torch.Tensor  # root -> the block of the gradient arena that holds the gradient of its output
    pairs: int


@dataclass(slots=True)
class SignedBinding:
    """What one batch size adds to a `_SignedCircuit`."""
    serial: int  # `state_serials`
    arena: torch.Tensor  # a block of (F, Bp, 32) floats per sum layer: log|v| ...
    signs: torch.Tensor  # ... and a sign word per row
    garena: torch.Tensor  # at a layer's offset: the gradient w.r.t. the product of its children
    seed: torch.Tensor  # the output layer's gradient
    xt: torch.Tensor  # the staged batch, (D, B) int32
    off: dict[int, int]  # layer -> offset of its block in both arenas
    Bp: int  # rows of a fold's block: whole 32-row tiles
    ro: dict[int, torch.Tensor] = field(default_factory=dict)  # sum layers: the children's offsets
    tabs: dict[int, GatherTables] = field(default_factory=dict)  # layers over Embedding folds
    ltab: dict[int, EmbTables] = field(default_factory=dict)  # Embedding layers
    gout_off: dict[int, torch.Tensor] = field(default_factory=dict)  # sum layers: per fold its reader's block in `garena`
    gfold: dict[int, GradRoute] = field(default_factory=dict)  # Embedding layers
    leaf: LeafBinding | None = None


class _SignedCircuit:
    """c(x) of a squared circuit with real parameters on SIGNED-LOG blocks (cirkit_amd/csrc/ck_signed.hip): fp32 log|v| plus one
    sign word per row instead of the reference's (log|v|, 0 or pi) pairs -- half the bytes and half the contractions of the
    complex layers, Embedding outputs never stored (the first sum layer reads the weight table), weight gradients added
    straight into the flat gradient.  Qualifies: Embedding layers (weight = a tensor, 32 units) under CP-T / arity-1 sum
    layers of 32 inputs and 32 (or, not directly over an Embedding layer, 1 .. 4) outputs whose weights are tensors; every
    fold read once; one scalar output.  `why` says what does not fit (the trainer then keeps the complex launch lists)."""

    def __init__(self, circuit: HipCircuit, grads: Mapping[str, torch.Tensor]) -> None:
        self.c, self.grads = circuit, grads
        self.leaf: SubtreeGroup | None = None
        self.why = self._analyse()
        self._bound: dict[int, SignedBinding] = {}

    def _analyse(self) -> str | None:
        c = self.c
        if c.plan.semiring != "complex-lse-sum":
            return "not a complex-lse-sum circuit"
        if len(c._out_pairs) != 1:
            return "several outputs"
        self.kind: dict[int, str] = {}
        self.wname: dict[int, str] = {}
        for i, (spec, l) in enumerate(zip(c.plan.layers, c.layers)):
            ch = c._children[i]
            if isinstance(l, HipEmbeddingLayer):
                if (l.num_output_units != 32 or l.weight.ops != ["tensor"] or not embedding_bwd_fits_lds(l.num_states, 32)
                        or l.scope_idx.shape[1] != 1):
                    return f"layer {i}: Embedding layers need 32 units, a plain weight tensor and a table that fits the LDS"
                self.kind[i] = "emb"
                self.wname[i] = l.weight.graph.nodes[0].config["tensor"]
            elif type(l) in (HipSumLayer, HipCPTLayer) and not getattr(l, "_mixing", False):
                if type(l) is HipSumLayer and l.arity != 1:
                    return f"layer {i}: a sum layer over several concatenated children"
                Ko = l.num_output_units
                if l.num_input_units != 32 or not (Ko == 32 or 1 <= Ko <= 4) or l.weight.ops != ["tensor"]:
                    return f"layer {i}: needs 32 input units, 32 or 1 .. 4 output units and a plain weight tensor"
                kinds = {self.kind.get(int(p)) for p in np.unique(ch[..., 0])}
                if kinds == {"emb"}:
                    if Ko != 32 or len(np.unique(ch[..., 0])) != 1:
                        return f"layer {i}: a layer over Embedding folds needs 32 outputs and ONE Embedding layer beneath it"
                    self.kind[i] = "gather"
                elif kinds == {"sum"} or kinds == {"sum", "gather"} or kinds == {"gather"}:
                    self.kind[i] = "sum"
                else:
                    return f"layer {i}: children of mixed kinds"
                self.wname[i] = l.weight.graph.nodes[0].config["tensor"]
            else:
                return f"layer {i}: {spec.type!r} has no signed-log form"
        names = list(self.wname.values())
        if len(set(names)) != len(names):
            return "a parameter tensor shared between layers"
        for n in names:
            if self.c.store[n].is_complex():
                return "complex parameter tensors"
        po = int(c._out_pairs[0, 0])
        if self.kind.get(po) not in ("sum", "gather") or c.layers[po].num_output_units != 1:
            return "the output is not a scalar sum unit"
        # The LEAF REGION -- Embedding -> 2 or 4 levels of binary CP-T layers, every fold read once (fusion.find_subtree_groups) -- as
        # ONE forward launch on signed LINEAR tiles (ck_leaf_walk_fwd, signed + keep_levels: no exponential or logarithm below the
        # region's roots, the tiles of every second level kept) and one backward launch per two levels (ck_leaf_walk_bwd, is_signed):
        # what the trainer of real circuits does for Categorical -> CP-T regions (training.py), on values of either sign.
        self.leaf = self._leaf_region() if os.environ.get("CK_SLSE_LEAF", "1") != "0" else None
        for i, k in self.kind.items():  # an Embedding fold read by nobody would keep an unwritten gradient block
            if k == "emb":
                read = np.zeros(c.layers[i].num_folds, dtype=bool)
                for ch in c._children:
                    if ch is not None:
                        read[ch[..., 1][ch[..., 0] == i]] = True
                if not read.all():
                    return f"layer {i}: Embedding folds that nothing reads"
        return None

    def _leaf_region(self) -> SubtreeGroup | None:
        """The fused leaf region of c (a `fusion.SubtreeGroup` of depth 2 or 4), or None."""
        c = self.c
        for depth in (4, 2):
            groups = [g for g in find_subtree_groups(c.plan, c.layers, c._children, c._out_pairs, max_depth=depth, signed=True)
                      if g.depth == depth]
            if groups:
                break
        else:
            return None
        if len(groups) != 1:  # (several Embedding layers with a region each: layer by layer)
            return None
        g = groups[0]
        if (self.kind.get(g.input_layer) != "emb" or self.kind.get(g.levels[0]) != "gather"
                or any(self.kind.get(j) != "sum" for j in g.levels[1:]) or c.layers[g.input_layer].num_states >= 65535):
            return None
        return g

    # ---- what a batch size adds -----------------------------------------------------------------------------------------------
    def bind(self, B: int) -> SignedBinding:
        st = self._bound.get(B)
        if st is not None:
            return st
        c = self.c
        st = self._arenas(B)
        parent = self._parents()
        self._forward_tables(st)
        self._gradient_routes(st, parent)
        if self.leaf is not None:
            if B * max(1, c.plan.num_variables) * 8 >= 2**32 or B * 32 >= 2**31:
                raise NotImplementedError(f"squared-circuit training: a batch of {B} rows exceeds the 32-bit offsets of the leaf launches")
            st.leaf = self._bind_leaf(st, B, parent)
        while len(self._bound) >= MAX_BOUND:
            self._bound.pop(next(iter(self._bound)))
        self._bound[B] = st
        return st

    def _arenas(self, B: int) -> SignedBinding:
        """The layout of the blocks and the buffers of their size (the activation arena first, the gradient arena second of its size)."""
        c, dev = self.c, self.c.device
        off, n = {}, 0
        Bp = (B + 31) // 32 * 32  # rows of a fold's block: whole 32-row tiles (TILE-NATIVE blocks, ck_signed.hip)
        for i, k in self.kind.items():  # a block of (F, Bp, 32) floats per sum layer -- values, and at the same offset in the
            if k != "emb":              # gradient arena the gradient w.r.t. the product of its children
                off[i] = n
                n += c.layers[i].num_folds * Bp * 32  # (a 1 .. 4 unit layer: rows of Ko floats at the start of its block)
        po = int(c._out_pairs[0, 0])
        return SignedBinding(
            serial=next(state_serials),
            arena=torch.zeros(max(n, 32), dtype=torch.float32, device=dev),
            signs=torch.zeros(max(n // 32, 1), dtype=torch.int32, device=dev),
            garena=torch.zeros(max(n, 32), dtype=torch.float32, device=dev),
            seed=torch.zeros(c.layers[po].num_folds * B, dtype=torch.float32, device=dev),
            xt=torch.zeros((max(1, c.plan.num_variables), B), dtype=torch.int32, device=dev),
            off=off, Bp=Bp)

    def _parents(self) -> Parents:
        parent: Parents = {}
        for i, k in self.kind.items():
            if k == "emb":
                continue
            ch = self.c._children[i]  # (F, H, 2)
            for f in range(ch.shape[0]):
                for h in range(ch.shape[1]):
                    parent[(int(ch[f, h, 0]), int(ch[f, h, 1]))] = (i, f)
        return parent

    def _forward_tables(self, st: SignedBinding) -> None:
        """What the forward launches read by: the signed-log tables of the Embedding layers, the gather tables of the layers over
        them, the children's row offsets of the others."""
        c, dev = self.c, self.c.device
        for i, k in self.kind.items():
            ch = c._children[i]
            if k == "emb":
                l = c.layers[i]
                rows = l.num_folds * (l.num_states + 1)
                st.ltab[i] = EmbTables(table=torch.zeros(rows * 32, dtype=torch.float32, device=dev),
                                       signs=torch.zeros(rows, dtype=torch.int32, device=dev))
            elif k == "gather":
                e = int(ch[0, 0, 0])
                folds = ch[..., 1].astype(np.int32)
                st.tabs[i] = GatherTables(
                    folds=torch.from_numpy(np.ascontiguousarray(folds)).to(dev),
                    variables=torch.from_numpy(np.ascontiguousarray(c.layers[e].scope_idx[folds, 0].astype(np.int32))).to(dev), emb=e)
            else:
                ro = np.zeros(ch.shape[:2], dtype=np.int64)
                for p in np.unique(ch[..., 0]):
                    sel = ch[..., 0] == p
                    ro[sel] = st.off[int(p)] + ch[..., 1][sel].astype(np.int64) * st.Bp * 32
                st.ro[i] = torch.from_numpy(ro).to(dev)

    def _gradient_routes(self, st: SignedBinding, parent: Parents) -> None:
        """Where each fold finds the gradient of its output: its reader's block."""
        c, dev = self.c, self.c.device
        po = int(c._out_pairs[0, 0])
        for i, k in self.kind.items():
            F = c.layers[i].num_folds
            if i == po:
                continue
            if k == "emb":
                gather = {parent[(i, f)][0] for f in range(F)}
                assert len(gather) == 1
                gfold = np.asarray([parent[(i, f)][1] for f in range(F)], dtype=np.int32)
                # folds that share a gradient block: 8 workgroups apart (one XCD, the same time: the block is read from HBM once)
                by_block: dict[int, list[int]] = {}
                for f in range(F):
                    by_block.setdefault(int(gfold[f]), []).append(f)
                groups = list(by_block.values())
                order = interleave_8_apart(groups)
                if -1 in order or len(groups) % 8 != 0:  # (ragged groups, a short last stretch: the plain order)
                    order = list(range(F))
                assert sorted(order) == list(range(F))
                st.gfold[i] = GradRoute(fold=torch.from_numpy(gfold).to(dev), reader=gather.pop(),
                                        order=torch.from_numpy(np.asarray(order, dtype=np.int32)).to(dev))
            else:
                if any((i, f) not in parent for f in range(F)):
                    raise NotImplementedError(f"layer {i}: folds that nothing reads")
                st.gout_off[i] = torch.from_numpy(np.asarray(
                    [st.off[parent[(i, f)][0]] + parent[(i, f)][1] * st.Bp * 32 for f in range(F)], dtype=np.int64)).to(dev)

    def _tiles(self, j: int, tiles: int) -> torch.Tensor:
        """Tile-native storage of layer j's folds: (F, tiles, 32 x 32)."""
        return torch.empty((self.c.layers[j].num_folds, tiles, 1024), dtype=torch.float32, device=self.c.device)

    def _bind_leaf(self, st: SignedBinding, B: int, parent: Parents) -> LeafBinding:
        """Descriptors and buffers of the leaf region's launches at batch size B."""
        c, g = self.c, self.leaf
        dev = c.device
        emb = c.layers[g.input_layer]
        D, Bp, tiles = g.depth, st.Bp, st.Bp // 32
        n_wg = c._n_cu
        n_roots = c.layers[g.root].num_folds
        noff = [int(v) for v in g.node_off]
        root_of = np.asarray(g.nodes).astype(np.int64)[noff[D] : noff[D] + n_roots]  # root t's fold of the root layer
        # where a root finds the gradient of its output: the block of the fold that reads it, as a block index of the gradient arena
        gin_block = np.asarray([(st.off[parent[(g.root, f)][0]] + parent[(g.root, f)][1] * Bp * 32) // (Bp * 32) for f in range(n_roots)],
                               dtype=np.int32)
        launches = []
        for tab, top in leaf_bwd_unit_tables(g, n_roots, emb.scope_idx[:, 0].astype(np.int64), gin_block=gin_block, leaves_from_nodes=False):
            work = balanced_segments(int(tab.shape[0]), tiles, n_wg, waves=8)
            launches.append(LeafLaunchTables(unit_tab=torch.from_numpy(tab).to(dev), top=top, work=torch.from_numpy(work).to(dev)))
        nodes_dev = torch.from_numpy(np.ascontiguousarray(g.nodes)).to(dev)
        scope = emb._scope(dev)
        node_off_c = (C.c_int32 * (D + 1))(*noff)
        return LeafBinding(
            launches=launches, keep=[self._tiles(j, tiles) if l % 2 == 1 else None for l, j in enumerate(g.levels)],
            redo=torch.zeros(n_roots * tiles, dtype=torch.int32, device=dev),
            G=[self._tiles(g.levels[la.top - 2], tiles) if la.top > 2 else None for la in launches],
            nodes=nodes_dev, node_off=node_off_c, scope=scope,
            scale=torch.zeros((emb.num_folds, emb.num_states + 1), dtype=torch.float32, device=dev),
            work=torch.from_numpy(leaf_segments(n_roots, tiles, n_wg)).to(dev), n_wg=n_wg,
            root_tab=c._leaf_root_table(nodes_dev, node_off_c, g.leaf_off, scope, D, n_roots),
            x64=torch.zeros((B, max(1, c.plan.num_variables)), dtype=torch.int64, device=dev),
            gin_fold=torch.from_numpy(gin_block[root_of].copy()).to(dev),
            pairs=1 if c._leaves_in_adjacent_pairs(g) else 0)

    # ---- the launch lists -------------------------------------------------------------------------------------------------------
    def output(self, B: int) -> torch.Tensor:
        """(B,) fp32: log|c(x_b)|."""
        c, st = self.c, self.bind(B)
        po, fo = int(c._out_pairs[0, 0]), int(c._out_pairs[0, 1])
        o = st.off[po] + fo * B
        return st.arena[o : o + B]

    def stage(self, x: torch.Tensor, stream: int) -> None:
        """The (B, D) batch -> (D, B) int32, checked against the number of states (`HipCircuit._stage_input`)."""
        c = self.c
        B = int(x.shape[0])
        st = self.bind(B)
        _, xi = c._prepare_input(x)
        D = c.plan.num_variables
        x64 = None if st.leaf is None else st.leaf.x64
        if c.validate_inputs:
            capi.call("ck_stage_categories", xi.data_ptr(), st.xt.data_ptr(), B, D, c._num_states_dev().data_ptr(),
                      c._bad_input.data_ptr(), 1 if c._preclamp() else 0, None if x64 is None else x64.data_ptr(), stream)
        else:
            capi.call("ck_transpose_i64_to_i32", xi.data_ptr(), st.xt.data_ptr(), B, D, stream)
            if x64 is not None:
                x64.copy_(xi)

    def _args(self, st: SignedBinding, i: int) -> tuple:
        """(row offsets | table, its signs, folds, variables, batch, states) of layer i's input: blocks of the arena, or Embedding rows."""
        if self.kind[i] == "gather":
            t = st.tabs[i]
            lt = st.ltab[t.emb]
            return (None, lt.table.data_ptr(), lt.signs.data_ptr(), t.folds.data_ptr(), t.variables.data_ptr(), st.xt.data_ptr(),
                    self.c.layers[t.emb].num_states)
        return st.ro[i].data_ptr(), None, None, None, None, None, 0

    def _in_leaf(self, i: int) -> bool:
        return self.leaf is not None and i in self.leaf.levels

    def forward(self, B: int, stream: int) -> None:
        c, st = self.c, self.bind(B)
        a, sg = st.arena.data_ptr(), st.signs.data_ptr()
        for i, k in self.kind.items():
            l = c.layers[i]
            if k == "emb":  # the weight table (F, C + 1, 32) of this step's parameters, and its signed-log form
                if l._table is None or l._table.dtype != torch.float32:
                    l.prepare(stream, batched=False)  # (allocates the table; first call only)
                lt = st.ltab[i]
                in_region = self.leaf is not None and i == self.leaf.input_layer  # (the leaf launches read the linear table only)
                capi.call("ck_slse_tables", c.store[self.wname[i]].data_ptr(), l._table.data_ptr(), None if in_region else lt.table.data_ptr(),
                          None if in_region else lt.signs.data_ptr(), l.num_folds, l.num_states, stream)
            elif self._in_leaf(i):  # (the whole region with the launch of its first level)
                if i == self.leaf.levels[0]:
                    self._leaf_forward(st, B, stream)
            else:
                o = st.off[i]
                ro, *gather = self._args(st, i)
                capi.call("ck_slse_fwd", a, sg, ro, c.store[self.wname[i]].data_ptr(), a + 4 * o, sg + 4 * (o // 32),
                          l.num_folds, l.arity, B, l.num_output_units, *gather, stream)
        if c.validate_inputs and c._int_input and self.leaf is None:  # (the leaf launch checks the rows it reads: theirs are NaN)
            y = self.output(B)
            capi.call("ck_poison_outputs", y.data_ptr(), B, c._bad_input.data_ptr(), stream)

    def _leaf_forward(self, st: SignedBinding, B: int, stream: int) -> None:
        c, g, L = self.c, self.leaf, st.leaf
        emb = c.layers[g.input_layer]
        o = st.off[g.root]
        d = capi.LeafLaunch()
        d.table, d.table_scale, d.scope = emb._table.data_ptr(), L.scale.data_ptr(), L.scope.data_ptr()
        d.w_levels = (C.c_void_p * g.depth)(*[c.store[self.wname[j]].data_ptr() for j in g.levels])
        d.nodes, d.node_off, d.leaf_off = L.nodes.data_ptr(), L.node_off, g.leaf_off
        d.out, d.signs_out = st.arena.data_ptr() + 4 * o, st.signs.data_ptr() + 4 * (o // 32)
        d.work, d.n_seg, d.n_wg, d.waves, d.depth = L.work.data_ptr(), int(L.work.shape[0]), L.n_wg, 8, g.depth
        d.B, d.K, d.C, d.w_layout = B, 32, emb.num_states, capi.CK_W_ROWMAJOR
        d.signed_redo = d.keep_redo = L.redo.data_ptr()
        d.n_roots, d.root_tab = c.layers[g.root].num_folds, L.root_tab.data_ptr()
        d.xt, d.preclamped, d.D, d.x_rows, d.x_input = None, 0, c.plan.num_variables, L.x64.data_ptr(), -1
        d.bad_input = c._bad_input.data_ptr() if c.validate_inputs else None
        d.x_pairs = L.pairs
        d.keep_levels = (C.c_void_p * g.depth)(*[None if t is None else t.data_ptr() for t in L.keep])
        capi.call("ck_leaf_walk_fwd", C.byref(d), stream)

    def _leaf_backward(self, st: SignedBinding, B: int, stream: int) -> None:
        c, g, L = self.c, self.leaf, st.leaf
        emb = c.layers[g.input_layer]
        ga = st.garena.data_ptr()
        gout1 = ga + 4 * st.off[g.levels[0]]  # (F_1, B, 32) row-major: what ck_embedding_bwd scatters
        leaf_backward(g, unit_tabs=[la.unit_tab.data_ptr() for la in L.launches], tops=[la.top for la in L.launches],
                      works=[la.work.data_ptr() for la in L.launches], n_segs=[int(la.work.shape[0]) for la in L.launches],
                      gouts=[gout1 if G is None else G.data_ptr() for G in L.G],
                      w=[c.store[self.wname[j]].data_ptr() for j in g.levels], dw=[self.grads[self.wname[j]].data_ptr() for j in g.levels],
                      keep=[None if t is None else t.data_ptr() for t in L.keep], redo=L.redo.data_ptr(), table=emb._table.data_ptr(),
                      scale=L.scale.data_ptr(), x_rows=L.x64.data_ptr(), nodes=L.nodes.data_ptr(), scope=L.scope.data_ptr(), B=B,
                      Cn=emb.num_states, D=c.plan.num_variables, n_roots=c.layers[g.root].num_folds, n_wg=L.n_wg, waves=8, gin=ga,
                      gin_rowmajor=0, is_signed=1, gin_fold=L.gin_fold.data_ptr(), stream=stream)

    def backward(self, B: int, seed: float, stream: int) -> None:
        """Gradients of ``seed * sum_b log|c(x_b)|`` ADDED into `grads` (the Embedding weights': written)."""
        c, st = self.c, self.bind(B)
        a, sg, ga = st.arena.data_ptr(), st.signs.data_ptr(), st.garena.data_ptr()
        po, fo = int(c._out_pairs[0, 0]), int(c._out_pairs[0, 1])
        # (filled on every run, inside the recorded list: the lists of one binding at two global batches share this block)
        if c.layers[po].num_folds > 1:
            capi.call("ck_fill_f32", st.seed.data_ptr(), st.seed.numel(), 0.0, stream)
        capi.call("ck_fill_f32", st.seed.data_ptr() + 4 * fo * B, B, float(seed), stream)
        for i in reversed(list(self.kind)):
            l, k = c.layers[i], self.kind[i]
            if k == "emb":
                r = st.gfold[i]
                capi.call("ck_embedding_bwd", ga + 4 * st.off[r.reader], 1, r.fold.data_ptr(), r.order.data_ptr(), st.xt.data_ptr(),
                          l._scope(c.device).data_ptr(), l._table.data_ptr(), self.grads[self.wname[i]].data_ptr(), l.num_folds, B, 32,
                          l.num_states, stream)
            elif self._in_leaf(i):  # (the whole region when its root layer is reached)
                if i == self.leaf.root:
                    self._leaf_backward(st, B, stream)
            else:
                o = st.off[i]
                ro, *gather = self._args(st, i)
                gout, gout_off = (st.seed.data_ptr(), None) if i == po else (ga, st.gout_off[i].data_ptr())
                capi.call("ck_slse_bwd", a, sg, ro, c.store[self.wname[i]].data_ptr(), a + 4 * o, sg + 4 * (o // 32), gout, gout_off,
                          ga + 4 * o, self.grads[self.wname[i]].data_ptr(), l.num_folds, l.arity, B, l.num_output_units, *gather, stream)
