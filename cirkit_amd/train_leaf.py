"""The backward of a fused leaf region, shared by the fused step of `HipTrainer` (cirkit_amd/train_fused.py: Categorical -> dense ->
CP-T levels on linear tiles) and the signed-log circuit of `HipSquaredTrainer` (cirkit_amd/train_signed.py: Embedding -> CP-T
levels on signed linear tiles): one `ck_leaf_walk_bwd` per two levels, top first, then `ck_leaf_walk_bwd_redo` over the (root,
tile) units whose forward walk left the linear range.  The unit tables are `fusion.leaf_bwd_unit_tables`'."""

from __future__ import annotations

import ctypes as C
from typing import Sequence

from . import _capi as capi
from .fusion import SubtreeGroup


def leaf_backward(g: SubtreeGroup, *, unit_tabs: Sequence[int], tops: Sequence[int], works: Sequence[int], n_segs: Sequence[int],
                  gouts: Sequence[int], w: Sequence[int], dw: Sequence[int], keep: Sequence[int | None], redo: int, table: int,
                  scale: int, x_rows: int, nodes: int, scope: int, B: int, Cn: int, D: int, n_roots: int, n_wg: int, waves: int,
                  gin: int, gin_rowmajor: int, is_signed: int, gin_fold: int | None, stream: int) -> None:
    """Every argument but the counts is a device address.  Per launch k: its unit table, the level `tops[k]` of its P nodes, its
    work segments and where it leaves the gradient tiles of the level below its Q nodes (`gouts[k]`: what launch k + 1 reads; the
    last one holds level 1's).  Per level of `g.levels`: the weights `w`, their gradients `dw` and the kept tiles `keep` (None for
    the levels in between, which the launch recomputes).  `gin`: the gradient of the roots' outputs, row-major blocks
    (`gin_rowmajor`) or tile-native ones found through the unit table; `gin_fold`: per root the block of `gin` its gradient lies
    in, for the redo launch (None: the root's own)."""
    first = gin
    for k, top in enumerate(tops):
        d = capi.LeafBwdLaunch()
        d.unit_tab, d.work, d.n_seg, d.n_wg, d.B, d.waves = unit_tabs[k], works[k], n_segs[k], n_wg, B, waves
        d.C, d.D, d.leaf, d.is_signed = Cn, D, 1 if top == 2 else 0, is_signed
        d.gin, d.gin_rowmajor = gin, gin_rowmajor if k == 0 else 0
        d.y_p = keep[top - 1]  # (the level in between, top - 1, is recomputed by the launch)
        if top == 2:
            d.table, d.x_rows = table, x_rows
        else:
            d.y_c = keep[top - 3]
        d.w_p, d.w_q = w[top - 1], w[top - 2]
        d.dw_p, d.dw_q = dw[top - 1], dw[top - 2]
        d.gout = gouts[k]
        d.redo = redo
        capi.call("ck_leaf_walk_bwd", C.byref(d), stream)
        gin = gouts[k]
    # (root, tile) units whose forward walk left the linear range: in (signed) log space, by a launch in which every other wave exits
    depth = g.depth
    capi.call("ck_leaf_walk_bwd_redo", table, scale, x_rows, B, Cn, D, nodes, (C.c_int32 * (depth + 1))(*[int(v) for v in g.node_off]),
              g.leaf_off, scope, depth, (C.c_void_p * depth)(*w), (C.c_void_p * depth)(*dw), first, gin, redo, n_roots, gin_fold,
              is_signed, stream)
