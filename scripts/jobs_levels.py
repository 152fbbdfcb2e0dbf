#!/usr/bin/env python3
"""Per-launch table of the job form of a training step (cirkit_amd/train_jobs.py): kind, units, jobs, splits, list lengths and
the launch's time when it is issued alone (HIP events, 20 repetitions after the whole step has run once).
    python scripts/jobs_levels.py [B] [config]      config 6: QuadGraph CP K = 64 (the reference's learning notebook); 4: BASELINE config 4"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cirkit_amd import _capi as capi  # noqa: E402

if os.environ.get("CK_LIB"):  # a lab build of the library
    capi._LIB_PATH = os.environ["CK_LIB"]
from cirkit_amd.initializers import init_plan_tensors  # noqa: E402
from cirkit_amd.templates import image_data  # noqa: E402
from cirkit_amd.training import HipTrainer  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
cfg = int(sys.argv[2]) if len(sys.argv) > 2 else 6
if cfg == 4:
    plan = image_data((1, 28, 28), "poon-domingos", input_layer="gaussian", num_input_units=64, sum_product_layer="cp", num_sum_units=64)
    x = torch.randn(B, 784).cuda()
else:
    plan = image_data((1, 28, 28), "quad-graph", input_layer="categorical", num_input_units=64, sum_product_layer="cp", num_sum_units=64)
    x = torch.randint(0, 256, (B, 784)).cuda()
tr = HipTrainer(plan, init_plan_tensors(plan), device="cuda:0", lr=0.01, jobs=True)
js = tr._jobs
for _ in range(3):
    tr.step(x)
torch.cuda.synchronize()
st = js.bind(B)
bd = tr.circuit._bind(B)
MODE = int(os.environ.get("MODE", "2"))  # 2: the optimizer inside the epilogues (what `step` runs on one rank); 1: d theta only
stream = torch.cuda.current_stream().cuda_stream
DTYPES = {"nsum": capi.NSUM_JOB_DTYPE, "input_bwd": capi.NSUM_JOB_DTYPE, "sum_fwd": capi.SUM_JOB_DTYPE, "sum_bwd": capi.SUM_JOB_DTYPE,
          "mix_fwd": capi.MIX_JOB_DTYPE, "mix_bwd": capi.MIX_JOB_DTYPE, "gauss_bwd": capi.GAUSS_JOB_DTYPE, "cat_bwd": capi.CAT_JOB_DTYPE}
total = 0.0
print(f"{'launch':10s} {'units':>6s} {'jobs':>6s} {'split':>5s} {'n_in':>9s} {'n_g':>9s} {'us':>8s}")
for la in st["launches"]:  # (`Launch` records; `JobStep._issue` knows each kind's entry point -- an input_bwd launch includes its layer's backward)
    what, n = la.kind, la.n
    if what == "mix_params":
        continue
    fn = lambda la=la: js._issue(la, bd, st, B, MODE, stream)
    if what == "root":
        desc = (1, 1, 1, "", "")
    else:
        t = la.tables.get(MODE, la.tables[1]).cpu().numpy().view(np.dtype(DTYPES[what])).reshape(-1)
        n_g = f"{t['n_g'].mean():.1f}/{t['n_g'].max()}" if "n_g" in t.dtype.names else ""
        if what in ("cat_bwd", "gauss_bwd"):
            desc = (n, n, 1, "", n_g)
        elif what in ("nsum", "input_bwd"):
            desc = (n, n, 1, f"{t['n_in'].mean():.1f}/{t['n_in'].max()}", "")
        elif what.startswith("sum"):
            desc = (n, int((t["split"] == 0).sum()), int(t["n_split"].max()), f"{t['n_in'].mean():.1f}/{t['n_in'].max()}", n_g)
            what = what + (f"/{la.param}w" if what == "sum_bwd" else "")
        else:
            ns = int(t["n_split"][0])
            desc = (n, n // ns, ns, f"H{t['H'].mean():.1f}/{t['H'].max()} S{t['S'].max()}", n_g)
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(20):
        fn()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / 20
    total += us
    print(f"{what:10s} {desc[0]:6d} {desc[1]:6d} {desc[2]:5d} {desc[3]:>9s} {desc[4]:>9s} {us:8.1f}")
print(f"sum of the job launches {total:.0f} us  ({len(st['launches'])} launches; the recorded step has {js.num_launches(B, MODE)})")
