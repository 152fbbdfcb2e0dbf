"""Record which entry points `HipCircuit` issues, case by case, into tests/golden/launch_lists.json (MI355X).

    python scripts/record_launch_lists.py [--out tests/golden/launch_lists.json]

Every launch of the package goes through `cirkit_amd._capi.call`; a wrapper around it notes the entry-point names.  Per
case (fixture plan, batch size, constructor arguments): the names and `num_ops` of `_record(bd, with_ll=False)` and
`_record(bd, with_ll=True)`, `bd.direct`, `bd.params_at_end`, the (layer, kernel) rows of `profile_kernels(x, iters=1)` and
the names it issued.  tests/test_gpu_launch_lists.py rebuilds every case with the functions below and compares.

The script also counts which branch of the layer dispatch every layer of every case takes and prints the branches no case
reaches.  It carries its own copy of the branch order (`branch_of_layers`), so that it runs unchanged on any commit.
"""

from __future__ import annotations

import argparse
import contextlib
import glob
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "launch_lists.json")

BATCH = 64
LARGE_BATCH = 4096  # one 32-row tile per CU and more: the persistent leaf launch is on
LARGE = ("cfg2_qt784", "cfg4_pd784", "cfg5_sos_c_k32")
VARIED = ("cfg2_qt784", "cfg4_pd784", "cfg5_sos_c_k32", "cfg5_sos_z_k32")
VARIANTS = {
    "fuse=False": {"fuse": False},
    "dense_on_table=False": {"dense_on_table": False},
    "fuse_regions=False": {"fuse_regions": False},
    "signed_real=False,complex_linear=False": {"signed_real": False, "complex_linear": False},
    "validate_inputs=False": {"validate_inputs": False},
    "direct_input=False": {"direct_input": False},
    "cache_params=True": {"cache_params": True},
}
BRANCHES = ("first tail layer", "later tail layer", "skipped", "TensorDot", "fused group", "tabulated dense", "Embedding gather",
            "batched leftover", "CP block / lone leftover", "region", "Gaussian product", "constant", "data input", "plain layer")
_REFUSALS = (ValueError, TypeError, NotImplementedError)  # what a constructor that does not take a plan raises
_HOST_ERRORS = _REFUSALS + (AttributeError, KeyError, IndexError)  # (never a device error: those end the run)


def plan_names() -> list[str]:
    """Every fixture plan: a .json with the .npz of its arrays beside it."""
    names = [os.path.basename(p)[:-5] for p in sorted(glob.glob(os.path.join(GOLDEN, "*.json")))]
    return [n for n in names if os.path.exists(os.path.join(GOLDEN, n + ".npz"))]


def load_plan(name: str):
    """(plan, tensors): the literal parameter values of the golden file where it has some, else the initialiser's."""
    from cirkit_amd.initializers import init_plan_tensors
    from cirkit_amd.plan import Plan

    plan = Plan.load(os.path.join(GOLDEN, name))
    lit = {}
    if os.path.exists(os.path.join(GOLDEN, name + "_golden.npz")):
        with np.load(os.path.join(GOLDEN, name + "_golden.npz")) as z:
            lit = {k[2:]: z[k] for k in z.files if k.startswith("w_")}
    return plan, (lit if lit else init_plan_tensors(plan))


def all_cases(names: list[str]) -> list[tuple[str, str, int, str]]:
    """(case id, plan, batch size, variant) of every case, in recording order."""
    out = [(f"{n}@{BATCH}", n, BATCH, "") for n in names]
    out += [(f"{n}@{LARGE_BATCH}", n, LARGE_BATCH, "") for n in LARGE]
    out += [(f"{n}@{BATCH}[{v}]", n, BATCH, v) for n in VARIED for v in VARIANTS]
    return out


@contextlib.contextmanager
def tapped(names: list[str]):
    """Append the name of every entry point called through `_capi.call` to `names`."""
    from cirkit_amd import _capi

    inner = _capi.call

    def call(name, *args):
        names.append(name)
        return inner(name, *args)

    _capi.call = call
    try:
        yield
    finally:
        _capi.call = inner


def build_circuit(plan_name: str, variant: str, device):
    from cirkit_amd.circuit import HipCircuit

    plan, tensors = load_plan(plan_name)
    return HipCircuit(plan, tensors, device=device, **VARIANTS.get(variant, {}))


def batch_for(hc, B: int):
    """A valid batch: state 0 of every discrete variable, 0.0 of every continuous one."""
    if not hc.plan.num_variables:
        return None
    return torch.zeros((B, hc.plan.num_variables), dtype=torch.float32 if hc._float_input else torch.int64, device=hc.device)


def record_case(hc, B: int) -> dict:
    """What the fixture holds for one circuit at one batch size."""
    out: dict = {}
    bd = hc._bind(B)
    for key, with_ll in (("forward", False), ("forward_ll", True)):
        names: list[str] = []
        with tapped(names):
            prog = hc._record(bd, with_ll=with_ll)
        out[key] = names
        out[key + "_num_ops"] = int(prog.num_ops)
        prog.close()
    out["direct"] = bool(bd.direct)
    out["params_at_end"] = bool(bd.params_at_end)
    names = []
    try:
        with tapped(names):
            rows = hc.profile_kernels(batch_for(hc, B), iters=1)
        out["profile_rows"] = [[int(r["layer"]), str(r["kernel"])] for r in rows]
    except _HOST_ERRORS as e:
        out["profile_rows"] = None
        out["profile_error"] = type(e).__name__
    out["profile_names"] = names
    return out


def branch_of_layers(hc) -> list[str]:
    """The dispatch branch every layer takes in a forward (the order of `HipCircuit._enqueue_layers_` when this fixture was
    first recorded); a circuit on the complex linear-tile path has its own launch list and takes none."""
    from cirkit_amd.layers import HipConstantValueLayer, HipInputLayer

    if hc._clin is not None:
        return []
    out, pending = [], []
    for i, l in enumerate(hc.layers):
        ch = hc._children[i]
        if pending and ch is not None and {int(p) for p in np.unique(ch[..., 0])} & set(pending):
            pending = []
        if hc._tail and i in hc._tail:
            if i == hc._tail[0]:
                pending = []
            out.append("first tail layer" if i == hc._tail[0] else "later tail layer")
        elif i in hc._virtual or i in hc._td_first:
            out.append("skipped")
        elif i in hc._td_had or i in hc._td_pair:
            out.append("TensorDot")
        elif i in hc._group_of_root:
            out.append("fused group")
        elif i in hc._tdense:
            out.append("tabulated dense")
        elif i in hc._emb_gather:
            out.append("Embedding gather")
        elif i in hc._cp_leftover and i not in hc._cp_blocks and not hc._complex and (
                not pending or hc.layers[pending[0]].num_output_units == l.num_output_units):
            pending.append(i)
            out.append("batched leftover")
        elif i in hc._cp_blocks or i in hc._cp_leftover:
            out.append("CP block / lone leftover")
        elif i in hc._regions:
            out.append("region")
        elif i in hc._input_prod:
            out.append("Gaussian product")
        elif isinstance(l, HipConstantValueLayer):
            out.append("constant")
        elif isinstance(l, HipInputLayer):
            out.append("data input")
        else:
            out.append("plain layer")
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    device = torch.device("cuda:0")
    accepted, refused = [], {}
    for n in plan_names():
        try:
            build_circuit(n, "", device)
            accepted.append(n)
        except _REFUSALS as e:
            refused[n] = type(e).__name__
    taken = dict.fromkeys(BRANCHES, 0)
    cases = {}
    for cid, n, B, v in all_cases(accepted):
        hc = build_circuit(n, v, device)
        cases[cid] = record_case(hc, B)
        for b in branch_of_layers(hc):
            taken[b] += 1
        print(f"{cid}: {cases[cid]['forward_num_ops']} / {cases[cid]['forward_ll_num_ops']} launches, direct={cases[cid]['direct']}, "
              f"params_at_end={cases[cid]['params_at_end']}, {len(cases[cid]['profile_rows'] or [])} profile rows", flush=True)
        del hc
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        json.dump({"cases": cases, "refused": refused}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("refused with default arguments:", refused or "none")
    print("layers per branch:", taken)
    print("branches never taken:", [b for b, k in taken.items() if k == 0] or "none")


if __name__ == "__main__":
    main()
