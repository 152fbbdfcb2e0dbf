"""Record what the fused, the layer-wise and the signed squared training steps bind and issue, case by case, into
tests/golden/train_step_calls.json, and what `HipSquaredTrainer` binds and issues on its other paths into
tests/golden/squared_step_calls.json (MI355X).

    python scripts/record_train_calls.py [--section all|train|squared] [--out ...] [--out-squared ...]

Per case the fixture notes

* the calls: every entry point issued through `cirkit_amd._capi.call` during one `loss_and_grads`, one `step` and one
  `_backward(B, float(B), seed)` (fused), or one `loss_and_grads` (layer-wise, signed), with their count arguments -- `tapped` of
  scripts/record_job_step_calls.py, which also notes the counts of a `LeafBwdLaunch` and whether `ck_table_dense_bwd` got a
  `TableOpt` -- never an address;
* the tables: a sha256 over every host-built device table read back -- the unit tables of `ck_leaf_walk_bwd`, `gfold`, `var`,
  `fold_order`, the work segments, the tail fold table (96-byte rows) and its levels, both softmax-backward job tables (88-byte
  rows), the four tables of every shared-children entry -- every pointer (`<u8`) field reduced to zero / non-zero;
* shapes (`G`, `dws`), `flags` and the sorted `need_zero`.

The `squared` section (SQUARED_CASES) notes per case and batch size the calls of one `loss_and_grads` (the first case: also of
one `step` and of one `loss_and_grads(global_batch=2 B)`), each the first -- eager -- call of its (part, B, global batch,
optimizer) key on a fresh trainer, and for c and for Z the weight-pool layout (per layer: offset, shape, `direct`), the per-layer
scratch shapes and digests of the `ro` tables of the Hadamard layers that have a backward launch of their own; for a signed c digests of `ro`, `gout_off`, the gather tables and
`gfold` / order.  `squared_state` reads them from the records of cirkit_amd/train_reverse.py and cirkit_amd/train_signed.py or
from the dicts and tuples of a commit from before them.

`trainer_state` is the one place that knows where a `HipTrainer` keeps this: the records of cirkit_amd/train_fused.py and the
binding dataclass of cirkit_amd/training.py, or the string-keyed dicts of a commit from before them, so that the script records
the same fixture on either.  tests/test_gpu_train_step_calls.py rebuilds every case with the functions below and compares;
tests/test_fusion.py compares `fusion.leaf_bwd_unit_tables` on the CPU with the `unit_tabs` digests, which depend on no device."""

from __future__ import annotations

import argparse
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "train_step_calls.json")
SQUARED_FIXTURE = os.path.join(GOLDEN, "squared_step_calls.json")

_spec = importlib.util.spec_from_file_location("record_job_step_calls", os.path.join(ROOT, "scripts", "record_job_step_calls.py"))
rjs = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rjs)
tapped = rjs.tapped

TAIL_DTYPE = [("w", "<u8"), ("gout", "<u8"), ("dw_part", "<u8"), ("child", "<u8", 4), ("gchild", "<u8", 4), ("H", "<i4"), ("Ko", "<i4")]
SOFTMAX_JOB_DTYPE = [("w", "<u8"), ("dw", "<u8"), ("dtheta", "<u8"), ("rows", "<i8"), ("len", "<i4"), ("first", "<i4"),
                     ("part_stride", "<i8"), ("n_part", "<i4"), ("reserved", "<i4"), ("theta", "<u8"), ("m1", "<u8"), ("m2", "<u8"),
                     ("w_out", "<u8")]

# fused: case -> (image shape or golden plan, depth of the leaf region, batch sizes, CK_TAIL_BWD)
# (1, 8, 8) is the smallest image accepted with a region of four levels (tail: two layers; (1, 4, 8), whose tail is the root layer
# alone, is refused: "layers outside the leaf region and the tail"), (1, 3, 4) the smallest accepted with two ((1, 2, 4) is
# refused likewise).  cfg2_qt784: the unit tables tests/test_fusion.py rebuilds on the CPU.
FUSED_CASES = {
    "qt2_1x8x8": ((1, 8, 8), 4, (32, 150, 320), None),
    "qt2_1x3x4": ((1, 3, 4), 2, (32, 150, 320), None),
    "qt2_1x8x8_layerwise_tail": ((1, 8, 8), 4, (150,), "0"),
    "cfg2_qt784": ("cfg2_qt784", 4, (32,), None),
}
# layer-wise: golden plans (quadgraph: shared children -- flags 1 and 2, the temporary and the gather; quadgraph, pd_gauss and
# the Tucker plan hold mixing layers), batch sizes 5 and 64
LAYERWISE_CASES = ("cfg1_rbt8", "quadgraph_6x6_k4", "pd_gauss_6x6_k4", "quadgraph_6x6_tucker_k4", "quadtree_4x4_kron_k3")
LAYERWISE_BATCHES = (5, 64)
SIGNED_ROWS = 300
# squared: case -> (plan of c, plan of Z or None: built by `squared_partition_plan`, `signed`, seed of the tensors, CK_SLSE_LEAF,
# batch sizes, whether a `step` and a `loss_and_grads` at twice the global batch are recorded too)
SQUARED_CASES = {
    "complex_emb_k4": ("sos_4x4_c_k4", "sos_4x4_z_k4", False, None, None, (5, 64), True),  # Embedding backward in two launches
    "complex_emb_k32": ("cfg5_sos_c_k32", "cfg5_sos_z_k32", False, None, None, (33,), False),  # `ck_embedding_bwd` in one
    "real_categorical": ("sq_cat_qt4x4_k5", None, None, 6, None, (5, 64), False),
    "real_gaussian": ("sq_gauss_qt4x4_k4", None, None, 8, None, (5, 64), False),
    "signed_layers": ("cfg5_sos_c_k32", "cfg5_sos_z_k32", True, None, "0", (33,), False),  # no leaf region
}


def digest(t, dtype=None) -> str:
    """sha256 of a table read back to the host; `dtype`: its record layout, whose `<u8` fields count as zero / non-zero."""
    a = np.ascontiguousarray(t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t))
    h = hashlib.sha256()
    if dtype is None:
        h.update(str(a.dtype).encode() + repr(tuple(a.shape)).encode() + a.tobytes())
        return h.hexdigest()
    rows = a.view(np.dtype(dtype)).reshape(-1)
    for field in dtype:
        col = np.ascontiguousarray(rows[field[0]])
        h.update((col != 0).astype(np.uint8).tobytes() if field[1] == "<u8" else col.tobytes())
    return h.hexdigest()


def _plan(src):
    from cirkit_amd.plan import Plan
    from cirkit_amd.templates import image_data

    if isinstance(src, str):
        return Plan.load(os.path.join(GOLDEN, src))
    return image_data(src, "quad-tree-2", num_input_units=32, num_sum_units=32)


def make_fused(case: str, device):
    """The fused trainer of a case, built under the case's CK_TAIL_BWD (read again when a batch size is bound: `tail_env`)."""
    from cirkit_amd.initializers import init_plan_tensors
    from cirkit_amd.training import HipTrainer

    src, depth, _, _ = FUSED_CASES[case]
    plan = _plan(src)
    with tail_env(case):
        tr = HipTrainer(plan, init_plan_tensors(plan, seed=4), device=device, lr=0.01, fused=True)
    assert tr.fused and trainer_state(tr, None)["group"].depth == depth, case
    return tr


class tail_env:
    def __init__(self, case: str) -> None:
        self.value = FUSED_CASES[case][3]

    def __enter__(self):
        self.old = os.environ.get("CK_TAIL_BWD")
        if self.value is not None:
            os.environ["CK_TAIL_BWD"] = self.value

    def __exit__(self, *exc):
        if self.value is not None:
            if self.old is None:
                del os.environ["CK_TAIL_BWD"]
            else:
                os.environ["CK_TAIL_BWD"] = self.old


def make_layerwise(case: str, device):
    from cirkit_amd.initializers import init_plan_tensors
    from cirkit_amd.training import HipTrainer

    plan = _plan(case)
    return HipTrainer(plan, init_plan_tensors(plan, seed=4), device=device, lr=0.01, fused=False, jobs=False)


def make_signed(device):
    from cirkit_amd.initializers import init_plan_tensors
    from cirkit_amd.training_squared import HipSquaredTrainer

    plan_c, plan_z = _plan("cfg5_sos_c_k32"), _plan("cfg5_sos_z_k32")
    tensors = {k: np.where(v == 0, np.float32(1e-2), v).astype(np.float32) for k, v in init_plan_tensors(plan_c).items()}
    tr = HipSquaredTrainer(plan_c, tensors, plan_z=plan_z, device=device, signed=True)
    assert tr._signed is not None and tr._signed.leaf is not None
    return tr


class _env:
    """One environment variable set (None: left alone) for the length of a block."""

    def __init__(self, name: str, value: str | None) -> None:
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.get(self.name)
        if self.value is not None:
            os.environ[self.name] = self.value

    def __exit__(self, *exc):
        if self.value is not None:
            if self.old is None:
                del os.environ[self.name]
            else:
                os.environ[self.name] = self.old


def make_squared(case: str, device):
    from cirkit_amd.initializers import init_plan_tensors
    from cirkit_amd.training_squared import HipSquaredTrainer

    src_c, src_z, signed, seed, leaf, _, _ = SQUARED_CASES[case]
    plan_c = _plan(src_c)
    tensors = init_plan_tensors(plan_c) if seed is None else init_plan_tensors(plan_c, seed=seed)
    # (the counter-based generator emits a few exact zeros: log 0)
    tensors = {k: np.where(v == 0, np.float32(1e-2), v).astype(np.float32) for k, v in tensors.items()}
    with _env("CK_SLSE_LEAF", leaf):  # (read once, at construction)
        tr = HipSquaredTrainer(plan_c, tensors, plan_z=None if src_z is None else _plan(src_z), device=device, signed=signed)
    assert (tr._signed is not None) == bool(signed) and (tr._signed is None or tr._signed.leaf is None), case
    return tr


def _get(o, name):
    return o[name] if isinstance(o, dict) else getattr(o, name)


def trainer_state(tr, B: int | None) -> dict:
    """What a `HipTrainer` holds for batch size B (None: what does not depend on it), under one set of names."""
    out: dict = {}
    if tr.fused:
        fz = tr._fused_step.tables if hasattr(tr, "_fused_step") else tr._fz
        out.update({k: _get(fz, k) for k in ("group", "launches", "fold_order", "gfold", "var")})
    if B is None:
        return out
    st = tr._bwd[B]
    out.update({k: _get(st, k) for k in ("flags", "need_zero", "dws")})
    out["shared"] = {j: [_get(sh, k) for k in ("row_off", "cptr", "clist", "coff")] for j, sh in _get(st, "shared").items()}
    if tr.fused:
        if isinstance(st, dict):  # per_B[B], its "tail_bwd" entry and the (key, (table, blocks)) softmax entries
            fb = tr._fz["per_B"][B]
            tail = fb["tail_bwd"]["tabs"]
            jobs = {k: (None if fb.get(k) is None else fb[k][1][0]) for k in ("sm_jobs", "sm_jobs_opt")}
        else:
            fb = st.fused
            tail = fb.tail
            jobs = {k: (None if getattr(fb, k) is None else getattr(fb, k).table) for k in ("sm_jobs", "sm_jobs_opt")}
        out.update(work=_get(fb, "work"), G=_get(fb, "G"), **jobs)
        out["tail"] = None if tail is None else (_get(tail, "folds"), _get(tail, "levels"))
    return out


def _fields(v, names: tuple) -> tuple:
    """A positional tuple as it is, a record by the names of its fields."""
    return tuple(v) if isinstance(v, tuple) else tuple(getattr(v, n) for n in names)


def squared_state(tr, B: int) -> dict:
    """What a `HipSquaredTrainer` holds at batch size B under one set of names: "c" / "z": the state of a layer-wise reverse list
    (`pool`, per layer `scratch`: {name: tensor or flag}); "signed": the binding of the signed-log circuit (`ro`, `gout_off`,
    `tabs`: (folds, variables, Embedding layer), `gfold`: (fold table, reader layer, order), `launches`: (unit table, top, work))."""
    import dataclasses

    def reverse(bwd, rows):
        st = (getattr(bwd, "bind", None) or bwd._bind)(rows)
        scratch = _get(st, "scratch")
        per_layer = []
        for i in range(len(bwd.c.layers)):
            sc = scratch[i]
            per_layer.append(dict(sc) if isinstance(sc, dict) else
                             {f.name: getattr(sc, f.name) for f in dataclasses.fields(sc) if getattr(sc, f.name) is not None})
        # (a layer whose reader's launch does its part -- an absorbed Hadamard layer, the first half of a TensorDot pair -- has no
        #  scratch of its own beyond its slice of the pool)
        return {"pool": _get(st, "pool"), "scratch": per_layer, "skip": set(bwd._skip)}

    out: dict = {"z": reverse(tr._bwd_z, 1)}
    if tr._signed is None:
        out["c"] = reverse(tr._bwd_c, B)
        return out
    st = tr._signed.bind(B)
    leaf = _get(st, "leaf") if (not isinstance(st, dict) or "leaf" in st) else None
    out["signed"] = {
        "ro": dict(_get(st, "ro")), "gout_off": dict(_get(st, "gout_off")),
        "tabs": {i: _fields(v, ("folds", "variables", "emb")) for i, v in _get(st, "tabs").items()},
        "gfold": {i: _fields(v, ("fold", "reader", "order")) for i, v in _get(st, "gfold").items()},
        "launches": None if leaf is None else [_fields(v, ("unit_tab", "top", "work")) for v in _get(leaf, "launches")],
    }
    return out


def unit_table_digests(tr) -> list:
    return [[int(top), digest(tab)] for tab, top in trainer_state(tr, None)["launches"]]


def record_fused(tr, case: str, B: int) -> dict:
    """One `loss_and_grads`, one `step`, one `_backward` with a seed at batch size B; then the tables they were issued over."""
    D = tr.plan.num_variables
    x = torch.randint(0, 256, (B, D), generator=torch.Generator().manual_seed(B)).to(tr.device)
    seed = torch.full((B,), -0.5 / B, dtype=torch.float32, device=tr.device)
    calls: dict = {"loss_and_grads": [], "step": [], "seeded_backward": []}
    with tail_env(case):
        with tapped(calls["loss_and_grads"]):
            tr.loss_and_grads(x)
        with tapped(calls["step"]):
            tr.step(x)
        with tapped(calls["seeded_backward"]), torch.cuda.device(tr.device):
            tr._forward(x)
            tr._backward(B, float(B), seed)
    torch.cuda.synchronize()
    st = trainer_state(tr, B)
    tail = st["tail"]
    return {
        "calls": calls, "gfold": digest(st["gfold"]), "var": digest(st["var"]), "fold_order": digest(st["fold_order"]),
        "work": [digest(w) for w in st["work"]], "G": [list(g.shape) for g in st["G"]],
        "tail": None if tail is None else [digest(tail[0], TAIL_DTYPE), digest(tail[1])],
        "sm_jobs": digest(st["sm_jobs"], SOFTMAX_JOB_DTYPE), "sm_jobs_opt": digest(st["sm_jobs_opt"], SOFTMAX_JOB_DTYPE),
    }


def _input(tr, B: int) -> torch.Tensor:
    from cirkit_amd.layers import HipGaussianLayer

    D, g = tr.plan.num_variables, torch.Generator().manual_seed(B)
    if any(isinstance(l, HipGaussianLayer) for l in tr.circuit.layers):
        return torch.rand((B, D), generator=g).to(tr.device)
    return torch.randint(0, 2, (B, D), generator=g).to(tr.device)


def record_layerwise(tr, B: int) -> dict:
    calls: list = []
    with tapped(calls):
        tr.loss_and_grads(_input(tr, B))
    torch.cuda.synchronize()
    st = trainer_state(tr, B)
    return {
        "calls": calls, "flags": sorted([int(j), int(f)] for j, f in st["flags"].items()), "need_zero": sorted(int(p) for p in st["need_zero"]),
        "dws": [[str(k), list(v.shape)] for k, v in st["dws"].items()],
        "shared": sorted([int(j), [digest(t) for t in tabs]] for j, tabs in st["shared"].items()),
    }


def record_signed(tr) -> dict:
    D = tr._signed.c.plan.num_variables
    x = torch.randint(0, 256, (SIGNED_ROWS, D), generator=torch.Generator().manual_seed(6)).to(tr._signed.c.device)
    calls: list = []
    with tapped(calls):
        tr.loss_and_grads(x)
    torch.cuda.synchronize()
    st = squared_state(tr, SIGNED_ROWS)["signed"]
    return {
        "calls": calls, "unit_tabs": [[int(top), digest(tab)] for tab, top, _ in st["launches"]],
        "work": [digest(work) for _, _, work in st["launches"]],
        "gfold": sorted([int(i), digest(gfold), digest(order)] for i, (gfold, _, order) in st["gfold"].items()),
    }


def _squared_input(tr, B: int) -> torch.Tensor:
    from cirkit_amd.layers import HipEmbeddingLayer, HipGaussianLayer

    D, g = tr.plan_c.num_variables, torch.Generator().manual_seed(B)
    if any(isinstance(l, HipGaussianLayer) for l in tr.c.layers):
        return torch.rand((B, D), generator=g).to(tr.device)
    states = min([l.num_states for l in tr.c.layers if isinstance(l, HipEmbeddingLayer)] or [2])
    return torch.randint(0, states, (B, D), generator=g).to(tr.device)


def _reverse_record(st: dict) -> dict:
    """Pool layout, scratch shapes and `ro` digests of one layer-wise reverse list."""
    pool = st["pool"]
    layout, shapes, ro = [], [], []
    for i, sc in enumerate(st["scratch"]):
        if "direct" in sc and "dw" in sc:  # (a sum / TensorDot layer: a slice of the pool, or the tensor's own gradient)
            off = None if sc["direct"] else (sc["dw"].data_ptr() - pool.data_ptr()) // 4
            layout.append([i, off, list(sc["dw"].shape), bool(sc["direct"])])
        if i in st["skip"]:
            continue
        shapes.append([i, sorted([k, list(v.shape)] for k, v in sc.items() if isinstance(v, torch.Tensor))])
        if "ro" in sc:
            ro.append([i, digest(sc["ro"])])
    return {"pool": int(pool.numel()), "layout": layout, "scratch": shapes, "ro": ro}


def record_squared(tr, case: str, B: int) -> dict:
    """The first call of each (part, B, global batch, optimizer) key at batch size B, then the state they were issued over."""
    x = _squared_input(tr, B)
    calls: dict = {"loss_and_grads": []}
    with tapped(calls["loss_and_grads"]):
        tr.loss_and_grads(x)
    if SQUARED_CASES[case][6]:
        calls["step"], calls["loss_and_grads_2B"] = [], []
        with tapped(calls["step"]):
            tr.step(x)
        with tapped(calls["loss_and_grads_2B"]):
            tr.loss_and_grads(x, global_batch=2 * B)
    torch.cuda.synchronize()
    st = squared_state(tr, B)
    out = {"calls": calls, "z": _reverse_record(st["z"])}
    if "c" in st:
        out["c"] = _reverse_record(st["c"])
    else:
        sg = st["signed"]
        assert sg["launches"] is None
        out["signed"] = {
            "ro": sorted([int(i), digest(t)] for i, t in sg["ro"].items()),
            "gout_off": sorted([int(i), digest(t)] for i, t in sg["gout_off"].items()),
            "tabs": sorted([int(i), digest(folds), digest(variables), int(emb)] for i, (folds, variables, emb) in sg["tabs"].items()),
            "gfold": sorted([int(i), digest(gfold), int(reader), digest(order)] for i, (gfold, reader, order) in sg["gfold"].items()),
        }
    return out


def record_all_squared(device) -> dict:
    cases, n_cu = {}, None
    for case, cfg in SQUARED_CASES.items():
        tr = make_squared(case, device)
        n_cu = int(tr.c._n_cu)
        for B in cfg[5]:
            cases[f"{case}@{B}"] = record_squared(tr, case, B)
        del tr
    return {"n_cu": n_cu, "squared": cases}


def record_all(device) -> dict:
    fused, unit_tabs, layerwise = {}, {}, {}
    n_cu = None
    for case, (_, _, batches, _) in FUSED_CASES.items():
        tr = make_fused(case, device)
        n_cu = int(tr.circuit._n_cu)
        unit_tabs[case] = unit_table_digests(tr)
        for B in batches:
            fused[f"{case}@{B}"] = record_fused(tr, case, B)
        del tr
    for case in LAYERWISE_CASES:
        tr = make_layerwise(case, device)
        for B in LAYERWISE_BATCHES:
            layerwise[f"{case}@{B}"] = record_layerwise(tr, B)
        del tr
    return {"n_cu": n_cu, "unit_tabs": unit_tabs, "fused": fused, "layerwise": layerwise, "signed": record_signed(make_signed(device))}


def _write(doc: dict, path: str) -> None:
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w", encoding="utf-8") as f:
        json.dump(doc, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", choices=("all", "train", "squared"), default="all")
    ap.add_argument("--out", default=FIXTURE)
    ap.add_argument("--out-squared", default=SQUARED_FIXTURE)
    args = ap.parse_args()
    if args.section in ("all", "squared"):
        doc = record_all_squared(torch.device("cuda:0"))
        for cid, c in doc["squared"].items():
            print(f"squared {cid}: {sum(len(v) for v in c['calls'].values())} calls", flush=True)
        _write(doc, args.out_squared)
    if args.section == "squared":
        return
    doc = record_all(torch.device("cuda:0"))
    for kind in ("fused", "layerwise"):
        for cid, c in doc[kind].items():
            calls = c["calls"]
            print(f"{kind} {cid}: {sum(len(v) for v in calls.values()) if isinstance(calls, dict) else len(calls)} calls", flush=True)
    print(f"signed: {len(doc['signed']['calls'])} calls", flush=True)
    _write(doc, args.out)


if __name__ == "__main__":
    main()
