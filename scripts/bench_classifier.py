#!/usr/bin/env python3
"""Classification throughput (`HipClassifier`, `HipClassifierTrainer`, DESIGN.md section 11 "Classification") on a
class-conditional QuadTree-2 circuit over 28 x 28 images: Categorical-256 inputs, K = 32, C = 10 classes, 4096 rows;
following scripts/bench_soft_evidence.py's protocol.

    python scripts/bench_classifier.py [--reps 20] [--warmup 5] [--rows 4096]

HIP events around each timed call after `--warmup` untimed ones; the median is reported.  Timed: `predict_log_proba` (the
fused forward + the class head), the trainer's `step` (layer-wise forward, head, reverse launch list, Adam), and
`ck_class_head` alone on the root block the forward left (seed + statistics, as the step runs it); and, for scale,
`HipTrainer(fused=False, jobs=False).step` on the same template with num_classes=1 (a code path this feature leaves as it
was).  Prints one JSON line.
"""

from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cirkit_amd.classification import HipClassifierTrainer  # noqa: E402
from cirkit_amd.initializers import init_plan_tensors  # noqa: E402
from cirkit_amd.templates import image_data  # noqa: E402
from cirkit_amd.training import HipTrainer  # noqa: E402


def _time(fn, reps: int, warmup: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", type=int, default=4096)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, C = args.rows, 10
    kw = dict(input_layer="categorical", num_input_units=32, sum_product_layer="cp", num_sum_units=32)
    plan = image_data((1, 28, 28), "quad-tree-2", num_classes=C, **kw)
    g = torch.Generator().manual_seed(2)
    x = torch.randint(0, 256, (B, 784), generator=g).to(dev)
    y = torch.randint(0, C, (B,), generator=g).to(dev)
    tr = HipClassifierTrainer(plan, init_plan_tensors(plan), device=dev, lr=0.01, generative_weight=0.3)
    clf = tr.classifier()
    t_pred = _time(lambda: clf.predict_log_proba(x), args.reps, args.warmup)
    t_step = _time(lambda: tr.step(x, y), args.reps, args.warmup)
    # the head alone, as the step runs it: on the root block of the last forward, seed into the root's gradient view
    c = tr.circuit
    bd, st = c._bind(B), tr._bind_backward(B)
    po, fo = int(c._out_pairs[0, 0]), int(c._out_pairs[0, 1])
    block, view = bd.views[po][fo], st.gviews[po][fo]
    t_head = _time(lambda: tr._head.run(block, labels=y, w_gen=0.3, w_disc=1.0, inv_gb=1.0 / B, seed=view, stats=True,
                                        bad_flag=c._bad_input), args.reps, args.warmup)
    stats = tr.loss_and_grads(x, y).cpu().numpy()
    tr.check_inputs()
    scalar = image_data((1, 28, 28), "quad-tree-2", num_classes=1, **kw)
    base = HipTrainer(scalar, init_plan_tensors(scalar), device=dev, lr=0.01, fused=False, jobs=False)
    t_base = _time(lambda: base.step(x), args.reps, args.warmup)
    row = {"circuit": "quad-tree-2 28x28 categorical-256 K=32", "C": C, "B": B, "predict_log_proba_ms": round(t_pred, 4),
           "classifier_step_ms": round(t_step, 4), "class_head_ms": round(t_head, 4),
           "class_head_GBps": round(2 * block.numel() * 4 / t_head / 1e6, 1),
           "scalar_layerwise_step_ms": round(t_base, 4), "live_rows": int(stats[2]), "accuracy": round(float(stats[4] / max(stats[3], 1)), 4)}
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
