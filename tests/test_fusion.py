"""Host-side schedules of the fused launches (cirkit_amd/fusion.py): CPU tests."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_backward_walk_segments_cover_every_tile_once_and_use_every_workgroup():
    """`balanced_segments` (the schedule of `ck_leaf_walk_bwd`): whatever form it picks -- whole roots cut into equal pieces
    dealt longest first, or the flat (root, wave round) list cut into equal stretches -- every (root, tile) is in exactly one
    segment, segments never straddle roots, workgroup g takes rows g, g + num_wg, ..., and at the north-star shape (196 nodes
    x 128 tiles, 8 waves) all 256 workgroups have work (whole roots would leave 60 idle)."""
    import numpy as np

    from cirkit_amd.fusion import balanced_segments

    for roots, tiles, wg, waves in [(196, 128, 256, 8), (49, 128, 256, 8), (196, 128, 256, 4), (49, 128, 256, 4), (3, 5, 256, 8),
                                    (1, 128, 256, 8), (392, 32, 256, 8), (7, 1000, 64, 8)]:
        seg = balanced_segments(roots, tiles, wg, waves=waves)
        assert seg.dtype == np.int32 and seg.shape[1] == 4
        cover = np.zeros((roots, tiles), dtype=np.int64)
        for r, t0, t1, _ in seg:
            assert 0 <= r < roots and 0 <= t0 <= t1 <= tiles
            cover[r, t0:t1] += 1
        assert (cover == 1).all(), (roots, tiles, wg, waves)
    seg = balanced_segments(196, 128, 256, waves=8)
    busy = {j % 256 for j, (_, t0, t1, _) in enumerate(seg) if t1 > t0}
    assert len(busy) == 256
    rounds = np.zeros(256)
    for j, (_, t0, t1, _) in enumerate(seg):
        rounds[j % 256] += -(-(t1 - t0) // 8)
    assert rounds.max() <= 13  # (12.25 on average)


def _restated_unit_tables(grp, n_roots, var_of_leaf, gin_block, leaves_from_nodes):
    """The row layout of `ck_leaf_walk_bwd`'s unit table as include/cirkit_hip.h words it, unit by unit: [fold of P's gradient
    tile, fold of P, of Q0, of Q1, of c0..c3, variables of the four leaves (leaf launch only), root of the region, 0, 0, 0]."""
    import numpy as np

    depth, out = grp.depth, []
    for top in range(depth, 0, -2):
        rows = []
        for t in range(n_roots):
            def node(level, k):
                return int(grp.nodes[grp.node_off[level] + t * 2 ** (depth - level) + k])

            for j in range(2 ** (depth - top)):
                p = node(top, j)
                if top < depth:
                    gin = node(top + 1, j // 2)  # the tile the launch above left for P's parent
                else:
                    gin = p if gin_block is None else int(gin_block[p])
                cs = [node(top - 2, 4 * j + i) for i in range(4)]
                vs = [0, 0, 0, 0]
                if top == 2:
                    leaves = [int(grp.nodes[grp.leaf_off + t * 2 ** depth + 4 * j + i]) for i in range(4)] if leaves_from_nodes else cs
                    vs = [int(var_of_leaf[f]) for f in leaves]
                rows.append([gin, p, node(top - 1, 2 * j), node(top - 1, 2 * j + 1), *cs, *vs, t, 0, 0, 0])
        out.append((np.asarray(rows, dtype=np.int32), top))
    return out


def test_leaf_bwd_unit_tables_match_the_recorded_digests_and_the_header_layout():
    """`leaf_bwd_unit_tables`, which both trainers call: (a) on the depth-4 region of cfg2_qt784 and on the depth-2 region of the
    (1, 3, 4) quad-tree image, byte for byte what `HipTrainer` built before the function existed (the `unit_tabs` digests of
    tests/golden/train_step_calls.json; no trainer before it built a depth-2 table of cfg2_qt784, whose two-level region the
    fused form refuses, so that group is held against the restatement alone); (b) entry by entry against a plain restatement
    of the header's row layout, on those groups and on a hand-made one -- depth 2, two roots, folds numbered out of order --
    under both settings of `gin_block` and `leaves_from_nodes`."""
    import importlib.util
    import json

    import numpy as np

    from cirkit_amd.fusion import SubtreeGroup, find_subtree_groups, leaf_bwd_unit_tables
    from cirkit_amd.layers import layer_from_spec
    from cirkit_amd.parameters import TensorStore
    from cirkit_amd.plan import resolve_fold_index
    from cirkit_amd.templates import image_data
    from test_host_logic import _setup

    spec = importlib.util.spec_from_file_location("record_train_calls", os.path.join(ROOT, "scripts", "record_train_calls.py"))
    rtc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rtc)
    with open(rtc.FIXTURE, encoding="utf-8") as f:
        recorded = json.load(f)["unit_tabs"]

    plan, _, _, layers, children, out_pairs = _setup("cfg2_qt784")
    groups = {d: find_subtree_groups(plan, layers, children, out_pairs, d)[0] for d in (4, 2)}
    small = image_data((1, 3, 4), "quad-tree-2", num_input_units=32, num_sum_units=32)
    store = TensorStore("cpu")
    slayers = [layer_from_spec(s, store, small.semiring) for s in small.layers]
    folds = [l.num_folds for l in slayers]
    schildren = [None if s.inputs is None else resolve_fold_index(s.inputs, folds) for s in small.layers]
    (sgrp,) = find_subtree_groups(small, slayers, schildren, resolve_fold_index(small.output, folds).reshape(-1, 2), 4)
    assert groups[4].depth == 4 and groups[2].depth == 2 and sgrp.depth == 2
    cases = [(groups[4], layers, "cfg2_qt784"), (groups[2], layers, None), (sgrp, slayers, "qt2_1x3x4")]
    for grp, ls, case in cases:
        n_roots, var_of_leaf = ls[grp.root].num_folds, ls[grp.input_layer].scope_idx[:, 0].astype(np.int64)
        got = leaf_bwd_unit_tables(grp, n_roots, var_of_leaf)
        assert [top for _, top in got] == list(range(grp.depth, 0, -2))
        if case is not None:
            assert [[top, rtc.digest(tab)] for tab, top in got] == recorded[case], case
        gin_block = np.arange(n_roots, dtype=np.int32)[::-1] * 3 + 5
        for gb, from_nodes in ((None, True), (gin_block, False), (gin_block, True), (None, False)):
            got = leaf_bwd_unit_tables(grp, n_roots, var_of_leaf, gin_block=gb, leaves_from_nodes=from_nodes)
            want = _restated_unit_tables(grp, n_roots, var_of_leaf, gb, from_nodes)
            for (a, ta), (b, tb) in zip(got, want):
                assert ta == tb and a.dtype == np.int32 and a.shape == b.shape and np.array_equal(a, b), (case, ta)
    # by hand: level 0 (8 table folds), level 1 (4), level 2 (the 2 roots), then the input folds behind the table folds
    nodes = np.asarray([5, 2, 7, 0, 3, 6, 1, 4,  3, 0, 2, 1,  1, 0,  6, 4, 0, 2, 7, 1, 5, 3], dtype=np.int32)
    hand = SubtreeGroup(input_layer=0, dense_layer=1, levels=[2, 3], nodes=nodes, node_off=[0, 8, 12], leaf_off=14)
    var_of_leaf = np.asarray([10, 11, 12, 13, 14, 15, 16, 17], dtype=np.int64)
    ((tab, top),) = leaf_bwd_unit_tables(hand, 2, var_of_leaf)
    assert top == 2 and tab.tolist() == [[1, 1, 3, 0, 5, 2, 7, 0, 16, 14, 10, 12, 0, 0, 0, 0], [0, 0, 2, 1, 3, 6, 1, 4, 17, 11, 15, 13, 1, 0, 0, 0]]
    ((tab, top),) = leaf_bwd_unit_tables(hand, 2, var_of_leaf, gin_block=np.asarray([40, 41], dtype=np.int32), leaves_from_nodes=False)
    assert tab.tolist() == [[41, 1, 3, 0, 5, 2, 7, 0, 15, 12, 17, 10, 0, 0, 0, 0], [40, 0, 2, 1, 3, 6, 1, 4, 13, 16, 11, 14, 1, 0, 0, 0]]


def test_interleave_8_apart_places_group_members_eight_apart_and_marks_holes():
    """`interleave_8_apart`: once the holes are dropped the result is a permutation of the members; members of a group sit 8
    apart inside a full stretch of 8 groups; a group shorter than the longest of its stretch leaves a hole (-1) where its member
    would be; a last stretch of fewer than 8 groups has its members that many apart (the callers' policies differ there)."""
    from cirkit_amd.fusion import interleave_8_apart

    def groups_of(sizes):
        it = iter(range(sum(sizes)))
        return [[next(it) for _ in range(n)] for n in sizes]

    regular = interleave_8_apart(groups_of([2] * 16))
    assert sorted(regular) == list(range(32)) and all(regular.index(2 * k + 1) - regular.index(2 * k) == 8 for k in range(16))
    short = interleave_8_apart(groups_of([2] * 7))  # one stretch of 7 groups: no hole, members 7 apart
    assert short == [0, 2, 4, 6, 8, 10, 12, 1, 3, 5, 7, 9, 11, 13]
    ragged = interleave_8_apart(groups_of([2, 2, 1, 2, 2, 2, 2, 2, 2]))
    assert [i for i, v in enumerate(ragged) if v < 0] == [10]  # (stretch 1, second members, third group)
    assert ragged == [0, 2, 4, 5, 7, 9, 11, 13, 1, 3, -1, 6, 8, 10, 12, 14, 15, 16]
    assert sorted(v for v in ragged if v >= 0) == list(range(17))
