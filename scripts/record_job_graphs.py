"""Record the job graph of the training step's job form, case by case, into tests/golden/job_graphs.json (no device needed).

    python scripts/record_job_graphs.py [--out tests/golden/job_graphs.json] [--dump CASE PATH]

The job graph (cirkit_amd/job_graph.py) is what `JobStep` derives from a folded plan before anything is bound: the sum,
mixing and sum-of-blocks jobs with their block lists, levels and gradient lists, the root, the input layers' gradient lists.
This script writes it in a canonical form -- plain lists and ints, in job order -- in full for three small circuits, as counts
and a sha256 for the larger ones, plus the reason strings of the plans that do not take the job form.
tests/test_job_graph.py rebuilds every case with the functions below and compares.

The script runs unchanged on a commit from before the job graph was a module of its own: there it builds the layers on the CPU
and calls `JobStep._analyse` through a stand-in for the trainer (`legacy_graph`).  Job fields are read through one accessor
(`get`) that takes a dict or a record.  `--dump` writes the full canonical form of one case, for diffing when a hash differs."""

from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "job_graphs.json")

K64 = dict(num_input_units=64, num_sum_units=64, sum_product_layer="cp")
# case -> (plan source, switches): a template call `(image shape, keyword arguments)` or the name of a golden plan
FULL = {
    "quadgraph_cat_3x4x4": (((3, 4, 4), dict(region_graph="quad-graph", input_layer="categorical")), {}),
    "pd_gauss_3x4x4": (((3, 4, 4), dict(region_graph="poon-domingos", input_layer="gaussian")), {}),
    "quadtree_cat_3x4x4": (((3, 4, 4), dict(region_graph="quad-tree-2", input_layer="categorical")), {}),
}
DIGEST = {
    "quadgraph_cat_8x8": (((1, 8, 8), dict(region_graph="quad-graph", input_layer="categorical")), {}),
    "pd_gauss_8x8": (((1, 8, 8), dict(region_graph="poon-domingos", input_layer="gaussian")), {}),
    "quadtree_cat_8x8": (((1, 8, 8), dict(region_graph="quad-tree-2", input_layer="categorical")), {}),
    "quadgraph_6x6_k64": ("quadgraph_6x6_k64", {}),
    "pd_gauss_6x6_k64": ("pd_gauss_6x6_k64", {}),
    "cfg4_pd784": ("cfg4_pd784", {}),  # the only plan with forward NSUM jobs and the collapsed dense x mixing pair
    "pd_gauss_6x6_k64[fold_mix_bwd=False]": ("pd_gauss_6x6_k64", dict(fold_mix_bwd=False)),  # mixing jobs with a backward launch
    "quadtree4_cat_8x8[max_list=2]": (((1, 8, 8), dict(region_graph="quad-tree-4", input_layer="categorical")), dict(max_list=2)),
}
REFUSED = {
    "cfg2_qt784": ("cfg2_qt784", {}),
    "quadgraph_6x6[use_mixing_weights=False]": (((1, 6, 6), dict(region_graph="quad-graph", input_layer="categorical",
                                                                  use_mixing_weights=False)), {}),
    "quadgraph_6x6[sum_weight_activation=sigmoid]": (((1, 6, 6), dict(region_graph="quad-graph", input_layer="categorical",
                                                                       sum_weight_activation="sigmoid")), {}),
    "quadgraph_6x6[num_classes=3]": (((1, 6, 6), dict(region_graph="quad-graph", input_layer="categorical", num_classes=3)), {}),
}


def make_plan(source):
    from cirkit_amd.plan import Plan
    from cirkit_amd.templates import image_data

    if isinstance(source, str):
        return Plan.load(os.path.join(GOLDEN, source))
    shape, kw = source
    return image_data(tuple(shape), **K64, **kw)


def cpu_circuit(plan):
    """(layers, children, out_pairs, is_complex) of a plan as `HipCircuit` derives them, on the CPU: the parameter values do
    not matter to the job graph, so every tensor is zeros of its shape."""
    from cirkit_amd.layers import layer_from_spec
    from cirkit_amd.parameters import TensorStore
    from cirkit_amd.plan import resolve_fold_index

    store = TensorStore("cpu")
    for name, (shape, dt) in plan.tensors.items():
        store.set(name, torch.zeros(tuple(shape), dtype=torch.complex64 if "complex" in dt else torch.float32))
    layers = [layer_from_spec(s, store, plan.semiring) for s in plan.layers]
    folds = [l.num_folds for l in layers]
    children = [None if s.inputs is None else resolve_fold_index(s.inputs, folds) for s in plan.layers]
    out_pairs = resolve_fold_index(plan.output, folds).reshape(-1, 2)
    return layers, children, out_pairs, plan.semiring == "complex-lse-sum"


def legacy_graph(plan, layers, children, out_pairs, is_complex, param_ops, max_list, fold_mix_bwd):
    """`JobStep._analyse` of a commit where the analysis is a method: through stand-ins for the circuit and the trainer."""
    from cirkit_amd import train_jobs as tj

    saved = tj.MAX_LIST, tj.FOLD_MIX_BWD
    tj.MAX_LIST, tj.FOLD_MIX_BWD = max_list, fold_mix_bwd
    try:
        js = tj.JobStep.__new__(tj.JobStep)
        js.c = SimpleNamespace(layers=layers, _children=children, _out_pairs=out_pairs, _complex=is_complex)
        js.tr = SimpleNamespace(plan=plan, _PARAM_OPS=param_ops, circuit=js.c)
        why = js._analyse()
    finally:
        tj.MAX_LIST, tj.FOLD_MIX_BWD = saved
    return js if why is None else why


def job_graph(source, **switches):
    """The job graph of a case, or the reason its plan does not take the job form; switches: `max_list`, `fold_mix_bwd`."""
    from cirkit_amd.training import HipTrainer

    plan = make_plan(source)
    args = (plan, *cpu_circuit(plan), HipTrainer._PARAM_OPS)
    try:
        from cirkit_amd.job_graph import build_job_graph
    except ImportError:
        from cirkit_amd import train_jobs as tj

        return legacy_graph(*args, switches.get("max_list", tj.MAX_LIST), switches.get("fold_mix_bwd", True))
    return build_job_graph(*args, **{"fold_mix_bwd": True, **switches})


def get(j, key, default=None):
    """A field of a job: a key of a dict or an attribute of a record; `default` where the key is absent or the field None."""
    v = j.get(key) if isinstance(j, dict) else getattr(j, key, None)
    return default if v is None else v


def _blocks(lst) -> list:
    return [list(x) for x in lst]


def canonical(g) -> dict:
    """The job graph as plain lists and ints, in job order."""
    mix_index = {id(r): n for n, r in enumerate(g.mix_jobs)}
    sums = []
    for j in g.sum_jobs:
        mx, ga = get(j, "mix"), get(j, "gather")
        sums.append({"layer": get(j, "layer"), "fold": get(j, "fold"), "ins": _blocks(get(j, "ins")), "out": list(get(j, "out")),
                     "gx": list(get(j, "gx")), "w": list(get(j, "w")), "theta": list(get(j, "theta")), "lf": get(j, "lf"),
                     "lb": get(j, "lb"), "g": _blocks(get(j, "g")), "gather": None if ga is None else list(ga),
                     "mix": None if mx is None else [mix_index[id(get(mx, "job"))], get(mx, "h"), _blocks(get(mx, "partners")),
                                                     bool(get(mx, "writer"))]})
    mixes = []
    for r in g.mix_jobs:
        d = {"layer": get(r, "layer"), "fold": get(r, "fold"), "slots": [_blocks(s) for s in get(r, "slots")], "H": get(r, "H"),
             "S": get(r, "S"), "out": list(get(r, "out")), "gx0": get(r, "gx0"), "w": list(get(r, "w")),
             "theta": list(get(r, "theta")), "lf": get(r, "lf"), "folded": bool(get(r, "folded", False))}
        if not d["folded"]:
            d["g"], d["lb"] = _blocks(get(r, "g")), get(r, "lb")
        mixes.append(d)
    root = g.root
    rmix = get(root, "mix")
    return {
        "sum_jobs": sums, "mix_jobs": mixes,
        "nsum_jobs": [{"ins": _blocks(get(j, "ins")), "out": list(get(j, "out")), "lf": get(j, "lf")} for j in g.nsum_jobs],
        "gsum_jobs": [{"ins": _blocks(get(j, "ins")), "out": list(get(j, "out")), "lb": get(j, "lb")} for j in g.gsum_jobs],
        "root": {"folds": [{"layer": get(s, "layer"), "fold": get(s, "fold"), "ins": _blocks(get(s, "ins")),
                            "theta": list(get(s, "theta"))} for s in get(root, "folds")],
                 "mix": None if rmix is None else {"layer": get(rmix, "layer"), "kids": [list(k) for k in get(rmix, "kids")],
                                                   "theta": list(get(rmix, "theta"))},
                 "gx0": get(root, "gx0"), "zero": get(root, "zero")},
        "input_g": {str(i): {"first": get(ig, "first"), "lists": [_blocks(lst) for lst in get(ig, "lists")], "lb": get(ig, "lb")}
                    for i, ig in g.input_g.items()},
        "inputs": list(g.inputs), "cat": sorted(g.cat), "gathered": sorted(g.gathered),
        "gauss": {str(i): [{"mean": list(get(r, "mean")), "sd": list(get(r, "sd")), "ss": bool(get(r, "ss", False)),
                            "vmin": get(r, "vmin"), "vmax": get(r, "vmax")} for r in recs] for i, recs in g.gauss.items()},
        "n_extra": g.n_extra,
    }


def uncovered(canon: dict) -> list[int]:
    """Input layers whose parameters no job epilogue updates."""
    return [i for i in canon["inputs"] if str(i) not in canon["gauss"] and i not in canon["cat"]]


def digest(canon: dict) -> dict:
    text = json.dumps(canon, sort_keys=True, separators=(",", ":"))
    mixes = canon["mix_jobs"]
    return {"sum_jobs": len(canon["sum_jobs"]), "mix_jobs": len(mixes), "folded_mix_jobs": sum(1 for r in mixes if r["folded"]),
            "nsum_jobs": len(canon["nsum_jobs"]), "gsum_jobs": len(canon["gsum_jobs"]), "root_folds": len(canon["root"]["folds"]),
            "n_extra": canon["n_extra"], "sha256": hashlib.sha256(text.encode()).hexdigest()}


def case_canonical(name: str) -> dict:
    source, switches = {**FULL, **DIGEST}[name]
    g = job_graph(source, **switches)
    if isinstance(g, str):
        raise SystemExit(f"{name}: the plan does not take the job form: {g}")
    return canonical(g)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FIXTURE)
    ap.add_argument("--dump", nargs=2, metavar=("CASE", "PATH"), help="write the full canonical form of one case to PATH")
    args = ap.parse_args()
    if args.dump:
        with open(args.dump[1], "w", encoding="utf-8") as f:
            json.dump(case_canonical(args.dump[0]), f, indent=1, sort_keys=True)
            f.write("\n")
        return
    doc: dict = {"full": {}, "digest": {}, "refused": {}}
    for name in list(FULL) + list(DIGEST):
        canon = case_canonical(name)
        if uncovered(canon):
            raise SystemExit(f"{name}: input layers {uncovered(canon)} are covered by no job epilogue (the fixture has no such case)")
        d = digest(canon)
        if name in FULL:
            doc["full"][name] = canon
        doc["digest"][name] = d
        print(f"{name}: {d}", flush=True)
    for name, (source, switches) in REFUSED.items():
        why = job_graph(source, **switches)
        if not isinstance(why, str):
            raise SystemExit(f"{name}: expected a refusal")
        doc["refused"][name] = why
        print(f"{name}: {why}")
    with open(args.out, "w", encoding="utf-8") as f:
        json.dump(doc, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
