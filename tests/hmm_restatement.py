"""The forward algorithm of a chain plan in fp64 torch: what `cirkit_amd.hmm.HipHMM.log_prob` is tested against
(tests/test_hmm.py pins it to the reference's recorded outputs)."""
import numpy as np
import torch

from cirkit_amd.hmm import chain_of


def log_emissions(plan, tensors, x):
    """(F, B, K) fp64 log emissions of the input layer at x (B, D); zeros where an entry is missing (-1, or NaN)."""
    layer = next(l for l in plan.layers if l.inputs is None)
    raw = {n: torch.as_tensor(np.asarray(tensors[g.nodes[0].config["tensor"]]), dtype=torch.float64) for n, g in layer.params.items()}
    xv = torch.as_tensor(np.asarray(x))[:, layer.scope_idx[:, 0]].T  # (F, B)
    if layer.type == "gaussian":
        xv = xv.double()
        missing = torch.isnan(xv)
        mean, sd = raw["mean"][:, None, :], (1e-5 + (1.0 - 1e-5) * torch.sigmoid(raw["stddev"]))[:, None, :]
        e = torch.distributions.Normal(mean, sd).log_prob(torch.where(missing, torch.zeros_like(xv), xv)[..., None])
    else:
        missing = xv < 0
        idx = torch.where(missing, torch.zeros_like(xv), xv).long()
        if layer.type == "categorical":
            table = torch.log_softmax(raw["probs"], dim=-1)  # (F, K, C)
            e = torch.gather(table.transpose(1, 2), 1, idx[..., None].expand(-1, -1, table.shape[1]))
        else:
            n = float(layer.config["total_count"])
            e = torch.distributions.Binomial(n, probs=torch.sigmoid(raw["probs"])[:, None, :]).log_prob(idx[..., None].double())
    return torch.where(missing[..., None], torch.zeros_like(e), e)


def hmm_log_prob(plan, tensors, x, integrate_vars=()):
    """(B,) fp64: v_s = logsumexp_i(log W_s[o, i] + v_{s-1}[i] + e_s[i]) along `chain_of(plan)`, unit 0 of the last step."""
    x = torch.as_tensor(np.asarray(x)).clone()
    if len(integrate_vars):
        x[:, list(integrate_vars)] = float("nan") if x.is_floating_point() else -1
    e = log_emissions(plan, tensors, x)
    v = torch.zeros_like(e[0])
    for s in chain_of(plan):
        g = plan.layers[s.layer].params["weight"]
        w = torch.as_tensor(np.asarray(tensors[g.nodes[0].config["tensor"]]), dtype=torch.float64)[0]  # (Ko, K) logits
        v = torch.logsumexp(torch.log_softmax(w, dim=-1)[None] + (v + e[s.fold])[:, None, :], dim=-1)
    return v[:, 0]
