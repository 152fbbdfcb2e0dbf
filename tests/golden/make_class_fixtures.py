"""Generator of the classification fixture (run where the reference is installed; CIRKIT_REFERENCE points at its checkout):

    python tests/golden/make_class_fixtures.py

On the committed plan `plan_quadgraph_1x4x4_cp_nc3` (image_data((1, 4, 4), "quad-graph", "cp", num_classes=3): a mixing root
of three units) it compiles the same symbolic circuit with the reference, loads the closed-form parameters of
`init_plan_tensors(plan, seed=0)`, and records the losses of notebooks/generative-vs-discriminative-circuit.ipynb
(`MNISTClassifier.generative_loss` with marginalize=False, `MNISTClassifier.discriminative_loss`) on one batch together with
every parameter gradient of the reference's own `loss.backward()` for each of the two.  The reference runs in fp64
(`circuit.double()`, as the y_f64 fixtures of make_fixtures.py): the discriminative gradient is the difference of two
generative-sized ones (entries of 1e-3 against 7e-2 here), so two fp32 autograd passes that round the output gradient
differently already differ by 2e-6 of the LARGER scale -- noise that would hide what the fixture is there to pin.

    tests/golden/quadgraph_1x4x4_cp_nc3_class_grads.npz: x, y, gen_loss, dis_loss, gg_<tensor>, gd_<tensor> (fp64)
"""
from __future__ import annotations

import os

import numpy as np
import torch

import make_fixtures as mf  # (puts the reference and the repository on sys.path)
from make_fixtures import HERE, PipelineContext, _fp64_copy, _load_closed_form, data_modalities, plan_from_torch_circuit

from cirkit_amd.plan import Plan  # noqa: E402

NAME = "plan_quadgraph_1x4x4_cp_nc3"
OUT = "quadgraph_1x4x4_cp_nc3_class_grads.npz"


def generative_loss(log_probs, labels):  # the notebook's, marginalize=False
    return -torch.mean(log_probs[torch.arange(log_probs.shape[0]), labels])


def discriminative_loss(log_probs, labels):  # the notebook's
    target = log_probs[torch.arange(log_probs.shape[0]), labels]
    return -torch.mean(target - torch.logsumexp(log_probs, dim=1))


def main():
    sc = data_modalities.image_data((1, 4, 4), "quad-graph", input_layer="categorical", num_input_units=3,
                                    sum_product_layer="cp", num_sum_units=3, num_classes=3)
    cc = PipelineContext(backend="torch", semiring="lse-sum", fold=True, optimize=True).compile(sc)
    plan, tensors = plan_from_torch_circuit(cc)
    committed = Plan.load(os.path.join(HERE, NAME))
    assert [l.type for l in plan.layers] == [l.type for l in committed.layers] and dict(plan.tensors) == dict(committed.tensors)
    with torch.no_grad():
        _load_closed_form(plan, tensors)
    g = torch.Generator().manual_seed(17)
    x = torch.randint(0, 256, (24, 16), generator=g)
    y = torch.randint(0, 3, (24,), generator=g)
    order = [id(p) for p in cc.parameters()]
    names = {order.index(id(p)): k for k, t in tensors.items() for p in cc.parameters() if p.data_ptr() == t.data_ptr()}
    assert len(names) == len(tensors)
    cc = _fp64_copy(cc)  # (parameters in the same order)
    extra = {"x": x.numpy().astype(np.int16), "y": y.numpy().astype(np.int64)}
    torch.set_grad_enabled(True)
    try:
        for tag, fn in (("g", generative_loss), ("d", discriminative_loss)):
            for p in cc.parameters():
                p.grad = None
            out = cc(x)
            assert out.shape == (24, 1, 3)
            loss = fn(out[:, 0, :], y)
            loss.backward()
            extra["gen_loss" if tag == "g" else "dis_loss"] = np.array(loss.item())
            for i, p in enumerate(cc.parameters()):
                assert p.dtype == torch.float64
                extra[f"g{tag}_{names[i]}"] = p.grad.numpy().copy()
    finally:
        torch.set_grad_enabled(False)
    np.savez_compressed(os.path.join(HERE, OUT), **extra)
    print(OUT, {k: (v.shape, float(np.abs(v).max())) for k, v in extra.items()})


if __name__ == "__main__":
    assert mf.REF
    main()
