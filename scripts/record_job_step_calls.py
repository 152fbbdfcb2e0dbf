"""Record what the job form of the training step binds and records, case by case, into tests/golden/job_step_calls.json (MI355X).

    python scripts/record_job_step_calls.py [--out tests/golden/job_step_calls.json]

Per case (circuit, batch size) and mode (1: d theta to the flat gradient, 2: the optimizer in the job epilogues) the step is
bound and its program recorded; no step runs.  The fixture notes

* the calls: every entry point issued through `cirkit_amd._capi.call` while the program is recorded, with its count arguments
  (the int / int64 arguments of its signature: units, waves, hmax, block size, B, C; of the root launch's struct R, B, mode,
  n_wg, S; of a leaf backward launch's struct n_seg, n_wg, B, C, D, leaf, waves, gin_rowmajor, is_signed; whether a `TableOpt` was
  passed: scripts/record_train_calls.py) -- never an address;
* the tables: per job launch a sha256 over its device table read back to the host -- every field that is not a pointer byte for
  byte, every pointer (`<u8`) field reduced to zero / non-zero -- plus the pool's length and the number of extra blocks.

`launch_tables` is the one place that knows how a binding lists its launches: the `Launch` records of cirkit_amd/train_jobs.py,
or the positional tuples of a commit from before them, so that the script records the same fixture on either.
tests/test_gpu_job_step_calls.py rebuilds every case with the functions below and compares."""

from __future__ import annotations

import argparse
import contextlib
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "job_step_calls.json")

# case -> (image shape, region graph, input layer, batch sizes)
CASES = {
    "quadgraph_cat_3x4x4": ((3, 4, 4), "quad-graph", "categorical", (32, 150)),
    "pd_gauss_3x4x4": ((3, 4, 4), "poon-domingos", "gaussian", (32, 320)),  # 320 rows: 10 tiles, partial sums and tickets
    "pd_gauss_1x6x6": ((1, 6, 6), "poon-domingos", "gaussian", (320,)),  # backward levels of 560 sum jobs: the remainder layout
}
_TABLE_DTYPE = {"nsum": "NSUM_JOB_DTYPE", "input_bwd": "NSUM_JOB_DTYPE", "sum_fwd": "SUM_JOB_DTYPE", "sum_bwd": "SUM_JOB_DTYPE",
                "mix_fwd": "MIX_JOB_DTYPE", "mix_bwd": "MIX_JOB_DTYPE", "mix_params": "MIX_JOB_DTYPE", "gauss_bwd": "GAUSS_JOB_DTYPE",
                "cat_bwd": "CAT_JOB_DTYPE"}


def make_trainer(case: str, device):
    from cirkit_amd.initializers import init_plan_tensors
    from cirkit_amd.templates import image_data
    from cirkit_amd.training import HipTrainer

    shape, rg, il, _ = CASES[case]
    plan = image_data(shape, region_graph=rg, input_layer=il, num_input_units=64, num_sum_units=64, sum_product_layer="cp")
    return HipTrainer(plan, init_plan_tensors(plan, seed=4), device=device, lr=0.01, jobs=True)


@contextlib.contextmanager
def tapped(calls: list):
    """Append [entry point, count arguments ...] of every call through `_capi.call` to `calls`."""
    from cirkit_amd import _capi

    inner = _capi.call

    def call(name, *args):
        row = [name]
        for a, ty in zip(args, _capi.SIGNATURES[name]):
            if ty in (C.c_int, C.c_int64):
                row.append(int(a))
            elif isinstance(getattr(a, "_obj", None), _capi.RootLaunch):
                ra = a._obj
                row += [int(ra.R), int(ra.B), int(ra.mode), int(ra.n_wg), int(ra.S)]
            elif isinstance(getattr(a, "_obj", None), _capi.LeafBwdLaunch):
                d = a._obj
                row += [int(getattr(d, f)) for f in ("n_seg", "n_wg", "B", "C", "D", "leaf", "waves", "gin_rowmajor", "is_signed")]
            elif ty == C.POINTER(_capi.TableOpt):  # (ck_table_dense_bwd: with or without the optimizer epilogue)
                row.append(0 if a is None else 1)
        calls.append(row)
        return inner(name, *args)

    _capi.call = call
    try:
        yield
    finally:
        _capi.call = inner


def launch_tables(la):
    """(kind, {mode: device table}) of one launch of a binding; the root launch has no table."""
    if isinstance(la, tuple):  # (kind, tables, n, ...) -- input launches: (kind, layer, tables, n)
        if la[0] == "root":
            return "root", None
        return la[0], (la[2] if la[0] in ("input_bwd", "gauss_bwd", "cat_bwd") else la[1])
    return la.kind, la.tables


def table_digest(kind: str, table: torch.Tensor) -> str:
    from cirkit_amd import _capi

    dtype = getattr(_capi, _TABLE_DTYPE[kind])
    rows = table.cpu().numpy().view(np.dtype(dtype)).reshape(-1)
    h = hashlib.sha256()
    for name, ty in dtype:
        col = np.ascontiguousarray(rows[name])
        h.update((col != 0).astype(np.uint8).tobytes() if ty == "<u8" else col.tobytes())
    return h.hexdigest()


def record_case(tr, B: int, mode: int) -> dict:
    js = tr._jobs
    st = js.bind(B)
    calls: list = []
    with tapped(calls):
        prog = js._program(st, B, mode)
    torch.cuda.synchronize()
    tables = []
    for la in st["launches"]:
        kind, tabs = launch_tables(la)
        tables.append([kind, None if tabs is None else table_digest(kind, tabs.get(mode, tabs[1]))])
    return {"calls": calls, "num_ops": int(prog.num_ops), "tables": tables, "pool": int(st["pool"].numel()),
            "n_extra": int(getattr(js, "graph", js).n_extra)}


def record_all(device) -> dict:
    cases: dict = {}
    n_cu = None
    for case, (_, _, _, batches) in CASES.items():
        tr = make_trainer(case, device)
        n_cu = int(tr.circuit._n_cu)
        for B in batches:
            for mode in (1, 2):
                cases[f"{case}@{B}/mode{mode}"] = record_case(tr, B, mode)
        del tr
    return {"n_cu": n_cu, "cases": cases}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    doc = record_all(torch.device("cuda:0"))
    for cid, c in doc["cases"].items():
        print(f"{cid}: {len(c['calls'])} calls, {c['num_ops']} launches, {len(c['tables'])} job launches, pool {c['pool']}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        json.dump(doc, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
