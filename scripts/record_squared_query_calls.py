"""Record what the queries of `HipSquaredCircuit` plan on the host and issue on the device, case by case, into
tests/golden/squared_query_calls.json.

    python scripts/record_squared_query_calls.py [--section all|host|device] [--out tests/golden/squared_query_calls.json]

A section that is not recorded is kept from the file as it stands.

* `host` (no GPU): per plan `tree_order`, `scope_bits`, `path_plan` of every variable, and per mask or query of the case
  `fold_classes`, `mixed_plan` -- plain, with `path=` (the ancestry of one variable) and with `readers=` (the down folds of a query
  set) -- and `host_plan`: ints as they are, the kind / src / children arrays as a sha256.  tests/test_squared_query_calls.py
  rebuilds it on the CPU.
* `device` (MI355X): per case and batch size the entry points issued through `cirkit_amd._capi.call` by every query of the case, with
  their integer arguments (`tapped` of scripts/record_job_step_calls.py) -- never an address -- and per launch of the four squared
  entry points a sha256 (`digest` of scripts/record_train_calls.py) of every table it reads.  The host tables -- the level rows of
  `ck_squared_path_bwd`, the fold rows of `ck_squared_down_bwd`, the variable rows of `ck_squared_down_leaf` -- are read through the
  call's own host pointer, so nothing here depends on where the package keeps them; weight-pointer words and arguments are
  reduced to zero / non-zero, the address of an input table to (layer, byte offset into that layer's `_table`); arena offsets stay
  as they are.  The three device tables of `ck_squared_mixed_fwd` (kind, off, wfold) are found by their addresses among the launch
  records of the circuit: `mixed_launch_tables` is the one place that knows where those are kept, attributes of typed records or
  the string-keyed dicts of a commit from before them.  tests/test_gpu_squared_query_calls.py rebuilds every case and compares."""

from __future__ import annotations

import argparse
import contextlib
import ctypes
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
FIXTURE = os.path.join(ROOT, "tests", "golden", "squared_query_calls.json")

_spec = importlib.util.spec_from_file_location("record_train_calls", os.path.join(ROOT, "scripts", "record_train_calls.py"))
rtc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rtc)
tapped, digest = rtc.tapped, rtc.digest

GAUSS_MASKS = ([], list(range(16)), [0, 1, 4, 5, 2, 15])  # nothing, everything, an aligned 2 x 2 block plus two scattered variables


def _helpers():
    import squared_down_restatement as P
    import squared_marginal_restatement as R
    import squared_sampling_restatement as S

    return P, R, S


def _ids(mask) -> list:
    return np.nonzero(np.asarray(mask))[0].tolist()


# ---- the host section -----------------------------------------------------------------------------------------------------------
def host_cases() -> dict:
    """name -> (plan, masks for `fold_classes` / `mixed_plan`, (variable, mask of the others) for `path=`, (Q, I) for `host_plan`)."""
    P, R, S = _helpers()
    half = _ids(S.draw_cases()["conditional"][1])
    emb_masks = [_ids(m) for m in R.masks_4x4()] + [sorted(set(range(16)) - set(half))]
    out = {}
    for sp in ("cp-t", "cp"):
        out[f"tiny_{sp}"] = (R.tiny_case(sp)[0], [q + i for q, i in P.TINY_QUERIES], [(v, _ids(m)) for v, m in S.tiny_queries()], P.TINY_QUERIES)
    out["emb32"] = (R.emb32_case()[0], emb_masks, [(v, _ids(m)) for v, m in S.emb32_queries()] + _raster_steps(), P.EMB32_QUERIES)
    out["cat"] = (R.cat_case()[0], [sum(P.CAT_QUERY, [])], [(v, _ids(m)) for v, m in S.cat_queries()], [P.CAT_QUERY])
    out["gauss"] = (R.gauss_case()[0], [list(m) for m in GAUSS_MASKS], [], [])
    return out


def _raster_steps() -> list:
    """The (variable, still integrated) pairs of the sixteen steps of a sample in raster order: mixed siblings."""
    return [(v, list(range(v + 1, 16))) for v in range(16)]


def _mixed_record(mp) -> dict:
    return {"classes": [np.asarray(c).tolist() for c in mp.classes], "root": [int(v) for v in mp.root], "num_mixed": int(mp.num_mixed),
            "layers": [[int(m.layer), np.asarray(m.folds).tolist(), digest(m.kind), digest(m.src)] for m in mp.layers]}


def _path_record(pp) -> list:
    return [int(pp.var), list(pp.leaf), [[lv.layer, lv.fold, lv.slot, [list(s) for s in lv.siblings]] for lv in pp.levels]]


def record_host_case(plan, masks, steps, queries) -> dict:
    from cirkit_amd.squared import fold_classes, mixed_plan
    from cirkit_amd.squared_posterior import host_plan
    from cirkit_amd.squared_sampling import path_plan, scope_bits, tree_order

    D = plan.num_variables

    def mask_of(ids):
        m = np.zeros(D, dtype=bool)
        m[list(ids)] = True
        return m

    out: dict = {"tree_order": [int(v) for v in tree_order(plan)], "scope_bits": [[int(b) for b in row] for row in scope_bits(plan)]}
    paths = {v: path_plan(plan, v) for v in range(D)}
    out["paths"] = [_path_record(paths[v]) for v in range(D)]
    out["masks"] = [[ids, [np.asarray(c).tolist() for c in fold_classes(plan, mask_of(ids))], _mixed_record(mixed_plan(plan, mask_of(ids)))]
                    for ids in masks]
    out["steps"] = [[v, ids, _mixed_record(mixed_plan(plan, mask_of(ids + [v]), path=paths[v].folds()))] for v, ids in steps]
    out["queries"] = []
    for q, i in queries:
        dp = host_plan(plan, q, mask_of(q + i))
        out["queries"].append({
            "Q": list(q), "I": list(i), "qvars": [int(v) for v in dp.qvars], "down": sorted(list(d) for d in dp.down), "top": list(dp.top),
            "leaves": [list(lf) for lf in dp.leaves], "mixed": _mixed_record(dp.mixed),
            "layers": [[int(dl.layer), [int(f) for f in dl.folds], digest(dl.children)] for dl in dp.layers]})
    return json.loads(json.dumps(out))


def record_host() -> dict:
    return {name: record_host_case(*case) for name, case in host_cases().items()}


# ---- the device section ---------------------------------------------------------------------------------------------------------
def _get(o, name):
    return o[name] if isinstance(o, dict) else getattr(o, name)


def mixed_launch_tables(sq) -> dict:
    """device address -> tensor, for the kind / off / wfold tables of every mixed launch the circuit holds: those of the cached
    masks of `log_marginal`, of the steps of the cached orders, of the cached query sets."""
    plans = list(sq._cache.values()) + [dp.mixed for dp in sq._down_plans.values()]
    sm = getattr(sq, "_sampler", None)
    for op in (sm.orders.values() if sm is not None else ()):
        plans += [s.mixed for s in op.steps if s.mixed is not None]
    out = {}
    for mp in plans:
        for tb in mp.dev.values():
            for la in _get(tb, "launches"):
                for name in ("kind", "off", "wfold"):
                    t = _get(la, name)
                    out[t.data_ptr()] = t
    return out


def _host_words(ptr, rows: int, words: int) -> np.ndarray:
    if not ptr or rows * words == 0:
        return np.zeros((0, words), dtype=np.int64)
    return np.ctypeslib.as_array(ctypes.cast(int(ptr), ctypes.POINTER(ctypes.c_int64)), shape=(rows * words,)).reshape(rows, words).copy()


def _table_of(sq, address: int) -> list:
    """[layer of c, byte offset] of an address inside that layer's input table."""
    for i, layer in enumerate(sq.c.layers):
        t = getattr(layer, "_table", None)
        if t is not None and t.data_ptr() <= address < t.data_ptr() + t.numel() * t.element_size():
            return [i, int(address - t.data_ptr())]
    raise AssertionError("an input-table address outside every input table")


def _nz(a) -> int:
    return 0 if not a else 1


@contextlib.contextmanager
def table_tap(sq, tables: list):
    """Append, per call of one of the four squared entry points, [entry point, what its pointer arguments are reduced to ...,
    a digest per table it reads] to `tables`."""
    from cirkit_amd import _capi

    inner = _capi.call

    def call(name, *a):
        if name == "ck_squared_mixed_fwd":
            dev = mixed_launch_tables(sq)
            tables.append([name, _nz(a[0]), _nz(a[6]), _nz(a[7]), _nz(a[9])] + [digest(dev[a[k]]) for k in (3, 4, 8)])
        elif name == "ck_squared_path_bwd":
            rows = _host_words(a[3], a[5], _capi.CK_SQ_PATH_LEVEL_WORDS + 2 * a[6])
            rows[:, 4:6] = rows[:, 4:6] != 0
            tables.append([name, _nz(a[0]), _nz(a[4]), _nz(a[12]), _nz(a[14]), _nz(a[15]), _table_of(sq, a[7]), digest(rows)])
        elif name == "ck_squared_down_bwd":
            rows = _host_words(a[5], a[7], _capi.CK_SQ_DOWN_FOLD_WORDS + 3 * a[8])
            tables.append([name, _nz(a[0]), _nz(a[9]), _nz(a[10]), digest(rows)])
        elif name == "ck_squared_down_leaf":
            rows = _host_words(a[2], a[4], _capi.CK_SQ_DOWN_LEAF_WORDS)
            where = [_table_of(sq, int(p)) for p in rows[:, 0]]
            rows[:, 0] = 0
            tables.append([name, where, digest(rows)])
        return inner(name, *a)

    _capi.call = call
    try:
        yield
    finally:
        _capi.call = inner


def _emb32_queries(sq, x, B, few: bool = False, **kw) -> list:
    """(name, call) of the 32-unit case: every kind of query (`few`: one or two of each, those with mixed folds)."""
    P, R, S = _helpers()
    _, drawn, _, seed = S.draw_cases()["conditional"]
    xs = R.rows_of(16, 3, B, seed=23).to(sq.device)
    masks, states, sets = R.masks_4x4(), S.emb32_queries(), P.EMB32_QUERIES
    if few:
        masks, states, sets = masks[4:5], states[2::5][:2], sets[2:]
    out = [(f"log_marginal{_ids(m)}", lambda m=m: sq.log_marginal(x, torch.from_numpy(m), **kw)) for m in masks]
    out += [(f"state_log_marginals{v}{_ids(m)}", lambda v=v, m=m: sq.state_log_marginals(x, v, torch.from_numpy(m), **kw)) for v, m in states]
    out += [(f"query_log_marginals{q}{i}", lambda q=q, i=i: sq.query_log_marginals(x, q, i, return_log_evidence=True, **kw)) for q, i in sets]
    out += [("sample", lambda: sq.sample(B, seed=20250101, **kw)), ("sample_raster", lambda: sq.sample(B, seed=20250102, order=S.RASTER, **kw)),
            ("sample_conditional", lambda: sq.sample_conditional(xs, torch.from_numpy(drawn), seed=seed, **kw))]
    return out


def device_cases() -> dict:
    """name -> (builder of (circuit, [(batch size, [(query name, call)])]))."""
    from cirkit_amd.squared import HipSquaredCircuit

    P, R, S = _helpers()

    def tiny(sp, padded):
        def build(dev):
            plan, tensors, _ = R.tiny_case(sp)
            if padded:
                plan, tensors = R.pad_tiny_to_32(plan, tensors, sp)
            sq = HipSquaredCircuit(plan, tensors, device=dev)
            x = P.tiny_rows().to(dev)
            return sq, [(5, [(f"query_log_marginals{q}{i}", lambda q=q, i=i: sq.query_log_marginals(x, q, i, return_log_evidence=True))
                             for q, i in P.TINY_QUERIES])]
        return build

    def emb32(batches, rows_per_block=1, **kw):
        def build(dev):
            plan, tensors, _ = R.emb32_case()
            sq = HipSquaredCircuit(plan, tensors, device=dev, rows_per_block=rows_per_block)
            runs = []
            for B in batches:
                runs.append((B, _emb32_queries(sq, P.emb32_rows()[:B].to(dev), B, few=bool(kw) or rows_per_block != 1, **kw)))
            return sq, runs
        return build

    def cat(dev):
        plan, tensors, _ = R.cat_case()
        sq = HipSquaredCircuit(plan, tensors, device=dev)
        x = P.cat_rows().to(dev)
        q, i = P.CAT_QUERY
        return sq, [(3, [(f"query_log_marginals{q}{i}", lambda: sq.query_log_marginals(x, q, i))] +
                     [(f"state_log_marginals{v}{_ids(m)}", lambda v=v, m=m: sq.state_log_marginals(x, v, torch.from_numpy(m))) for v, m in S.cat_queries()])]

    def gauss(dev):
        plan, tensors, x = R.gauss_case()
        sq = HipSquaredCircuit(plan, tensors, device=dev)
        xg = x[:3].to(torch.float32).to(dev)
        xg[1, 7] = float("nan")  # (an absent entry: the float path of the cleaning)
        return sq, [(3, [(f"log_marginal{list(m)}", lambda m=m: sq.log_marginal(xg, list(m))) for m in GAUSS_MASKS])]

    out = {f"tiny_{sp}_{'k32' if padded else 'k3'}": tiny(sp, padded) for sp in ("cp-t", "cp") for padded in (False, True)}
    out.update(emb32=emb32((1, 33)), emb32_two_chunks=emb32((33,), rows_per_chunk=17), emb32_rows_per_block4=emb32((33,), rows_per_block=4),
               cat=cat, gauss=gauss)
    return out


def record_device_case(build, device) -> dict:
    """Per batch size of a case {query: {calls, tables, launch counters}}, on a fresh circuit, in the order of the case."""
    sq, runs = build(device)
    out = {}
    for B, queries in runs:
        rec = {}
        for name, call in queries:
            calls, tables = [], []
            with tapped(calls), table_tap(sq, tables):
                call()
            torch.cuda.synchronize()
            rec[name] = {"calls": calls, "tables": tables, "launches": [int(sq.last_launches), int(sq.last_mixed_launches), int(sq.last_down_launches)]}
        out[str(B)] = rec
    return json.loads(json.dumps(out))


def record_device(device) -> dict:
    return {name: record_device_case(build, device) for name, build in device_cases().items()}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", choices=("all", "host", "device"), default="all")
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    doc = {}
    if os.path.exists(args.out):
        with open(args.out, encoding="utf-8") as f:
            doc = json.load(f)
    if args.section in ("all", "host"):
        doc["host"] = record_host()
        print(f"host: {len(doc['host'])} plans", flush=True)
    if args.section in ("all", "device"):
        doc["device"] = record_device(torch.device("cuda:0"))
        for cid, c in doc["device"].items():
            print(f"device {cid}: {sum(len(q['calls']) for rec in c.values() for q in rec.values())} calls", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        json.dump(doc, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
