"""The fold graph of a circuit ``c`` as the queries of `HipSquaredCircuit` read it (cirkit_amd/squared.py, squared_sampling.py,
squared_posterior.py): who reads whom, which variables lie under a fold, the ancestry of a variable, and -- from those variables
alone -- the class of a fold for a set of integrated variables.  Built once per plan (`resolve_fold_index` once per layer) and
kept on the circuit; the module-level functions build one for a caller that only has a `Plan`."""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .plan import Plan, resolve_fold_index

OBSERVED, INTEGRATED, MIXED = 0, 1, 2


def fold_class(bits: int, mbits: int) -> int:
    """The class of a fold over the variables `bits` when the variables `mbits` are integrated: OBSERVED (disjoint), INTEGRATED
    (inside) or MIXED."""
    return OBSERVED if not bits & mbits else (INTEGRATED if not bits & ~mbits else MIXED)


def mask_bits(mask: np.ndarray) -> int:
    return sum(1 << int(v) for v in np.nonzero(mask)[0])


@dataclass
class PathLevel:
    """One ancestor of a variable: fold `fold` of layer `layer`, which reads the fold below it on the path in child slot
    `slot` and the `siblings` ``(layer, fold)`` in its other slots."""

    layer: int
    fold: int
    slot: int
    siblings: list[tuple[int, int]]


@dataclass
class PathPlan:
    var: int
    leaf: tuple[int, int]  # the input fold that reads the variable
    levels: list[PathLevel]  # root first

    def folds(self) -> set[tuple[int, int]]:
        return {self.leaf} | {(lv.layer, lv.fold) for lv in self.levels}


class FoldGraph:
    def __init__(self, plan: Plan) -> None:
        folds = [l.num_folds for l in plan.layers]
        self.plan = plan
        self.children = [None if l.inputs is None else resolve_fold_index(l.inputs, folds) for l in plan.layers]  # (F, H, 2) each
        self.top = tuple(int(v) for v in resolve_fold_index(plan.output, folds).reshape(-1, 2)[0])  # the output fold
        self.fold_base = np.concatenate([[0], np.cumsum(folds)])  # global fold id of a layer's fold 0
        self.readers: dict[tuple[int, int], list[tuple[int, int, int]]] = {}  # (layer, fold) -> the (layer, fold, slot) that read it
        self.bits: list[list[int]] = []  # per layer, per fold, the variables under it as the bits of an int
        self.leaves: dict[int, list[tuple[int, int]]] = {}  # variable -> the input folds that read it
        for i, (l, ch) in enumerate(zip(plan.layers, self.children)):
            if ch is None:
                self.bits.append([sum(1 << int(v) for v in row) for row in l.scope_idx])
                for f, row in enumerate(l.scope_idx):
                    for v in row:
                        self.leaves.setdefault(int(v), []).append((i, f))
                continue
            row_bits = []
            for f, row in enumerate(ch):
                b = 0
                for h, (p, g) in enumerate(row):
                    b |= self.bits[int(p)][int(g)]
                    self.readers.setdefault((int(p), int(g)), []).append((i, f, h))
                row_bits.append(b)
            self.bits.append(row_bits)
        self._paths: dict[int, PathPlan] = {}
        self._tree: list[int] | None = None

    @staticmethod
    def units(l) -> int:
        """The units of a layer's folds as their readers see them."""
        return l.num_input_units if l.type == "hadamard" else l.num_output_units

    def classes(self, mask: np.ndarray) -> list[np.ndarray]:
        mbits = mask_bits(mask)
        return [np.asarray([fold_class(b, mbits) for b in row], dtype=np.int8) for row in self.bits]

    def tree_order(self) -> list[int]:
        if self._tree is None:
            order: dict[int, None] = {}  # (first meeting first)
            stack = [self.top]
            while stack:
                p, f = stack.pop()
                if self.children[p] is None:
                    order.update((int(v), None) for v in self.plan.layers[p].scope_idx[f])
                else:
                    stack.extend((int(q), int(g)) for q, g in self.children[p][f][::-1])
            self._tree = list(order)
        return self._tree

    def path(self, var: int) -> PathPlan:
        var = int(var)
        if var in self._paths:
            return self._paths[var]
        leaves = self.leaves.get(var, [])
        if len(leaves) != 1:
            raise NotImplementedError(f"HipSquaredCircuit: variable {var} is read by {len(leaves)} input folds; sampling and all-state "
                                      "conditionals walk ONE path from the root to the variable (region graphs that are trees)")
        levels: list[PathLevel] = []
        cur = leaves[0]
        while cur != self.top:
            rd = self.readers.get(cur, [])
            if len(rd) != 1:
                raise NotImplementedError(f"HipSquaredCircuit: fold {cur[1]} of layer {cur[0]} above variable {var} has {len(rd)} readers; "
                                          "sampling and all-state conditionals walk ONE path from the root to the variable (region graphs "
                                          "that are trees; a DAG such as a QuadGraph or Poon-Domingos is not supported)")
            i, f, h = rd[0]
            levels.append(PathLevel(i, f, h, [(int(p), int(g)) for k, (p, g) in enumerate(self.children[i][f]) if k != h]))
            cur = (i, f)
        self._paths[var] = PathPlan(var, leaves[0], levels[::-1])
        return self._paths[var]

    def num_states(self, var: int) -> int:
        cfg = self.plan.layers[self.path(var).leaf[0]].config
        return int(cfg.get("num_states", cfg.get("num_categories", 0)))


def graph_of(plan: Plan, graph: FoldGraph | None = None) -> FoldGraph:
    return FoldGraph(plan) if graph is None else graph


def tree_order(plan: Plan, graph: FoldGraph | None = None) -> list[int]:
    """The variables in the order a depth-first walk of the fold tree below the output meets them.  Sampling in this order,
    every sibling of a fold on the path of the variable being drawn is entirely drawn or entirely still to draw."""
    return graph_of(plan, graph).tree_order()


def path_plan(plan: Plan, var: int, graph: FoldGraph | None = None) -> PathPlan:
    """The ancestry of a variable, root first.  ``NotImplementedError`` unless it is a path: one input fold reads the
    variable and every fold on the way up has exactly one reader, up to the output fold (a region graph that is a tree)."""
    return graph_of(plan, graph).path(var)


def scope_bits(plan: Plan, graph: FoldGraph | None = None) -> list[list[int]]:
    """Per layer, per fold, the variables under it as the bits of an int."""
    return graph_of(plan, graph).bits
