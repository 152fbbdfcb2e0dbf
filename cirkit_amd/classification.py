"""Classification with class-conditional circuits: `HipClassifier` (inference) and `HipClassifierTrainer` (training).

`templates.image_data(..., num_classes=C)` builds a circuit whose root fold has C units, unit c being ``log p(x | y = c)``.
The reference trains and queries such a circuit in torch on its ``(B, 1, C)`` output
(notebooks/generative-vs-discriminative-circuit.ipynb: the class-conditional NLL, the cross-entropy
``log p(x | y) - logsumexp_c log p(x | c)``, prediction with missing pixels through ``IntegrateQuery``,
cirkit/backend/torch/queries.py:19-184).  Here that step is ONE kernel, the class head `ck_class_head`
(cirkit_amd/csrc/ck_class.hip; DESIGN.md section 11, "Classification"):

    j_bc = l_bc + pi_c        e_b = logsumexp_c j_bc = log p(x_b)        q_bc = j_bc - e_b = log p(y = c | x_b)
    L = -(1 / gB) sum_b (w_gen gen_b + w_disc disc_b),   gen_b = j_{b,y_b} | e_b,   disc_b = q_{b,y_b} | 0   (labelled | y_b = -1)

It reads the root fold's block where the forward left it and writes the posterior, the prediction, the six fp64 statistics
and -- for training -- the seed dL/dl straight into the root's gradient view, from where the layer-wise reverse launch list
of `HipTrainer` runs unchanged (its kernels are shape-generic in the root's unit count).

Out of scope: the fused and job forms of the training step (they keep refusing a root of several units; the classifier
trainer never asks them), squared circuits, several output folds, label smoothing.
"""

from __future__ import annotations

from typing import Mapping

import numpy as np
import torch

from . import _capi as capi
from .distributed import all_reduce_sum as _all_reduce_sum, world_size as _world_size
from .plan import Plan, resolve_fold_index
from .training import HipTrainer

STATS = ("sum_gen", "sum_disc", "live", "labelled", "correct", "dead")  # the six statistics, in the head's order


def num_classes(plan: Plan) -> int:
    """The number of classes of a class-conditional plan (the units of its one output fold); raises for plans the class
    head does not serve.  Host only: nothing is allocated."""
    if plan.semiring != "lse-sum":
        raise NotImplementedError(f"classification needs a circuit under the real lse-sum semiring, not {plan.semiring!r} "
                                  "(squared circuits are out of scope)")
    out = resolve_fold_index(plan.output, [l.num_folds for l in plan.layers]).reshape(-1, 2)
    if len(out) != 1:
        raise NotImplementedError(f"classification needs a single output fold whose units are the classes; this plan has {len(out)}")
    return int(plan.layers[int(out[0, 0])].num_output_units)


def normalise_log_prior(log_prior, C: int) -> np.ndarray | None:
    """The user's unnormalised log prior as the normalised fp32 vector the head reads (log-softmax in fp64 on the host;
    -inf entries -- impossible classes -- stay -inf); None (uniform) stays None."""
    if log_prior is None:
        return None
    p = np.asarray(log_prior.detach().cpu() if hasattr(log_prior, "detach") else log_prior, dtype=np.float64).reshape(-1)
    if p.shape[0] != C:
        raise ValueError(f"log_prior holds {p.shape[0]} entries, the circuit has {C} classes")
    if np.isnan(p).any() or np.isposinf(p).any():
        raise ValueError("log_prior holds a NaN or +inf entry")
    if not np.isfinite(p).any():
        raise ValueError("log_prior is -inf everywhere: no class is possible")
    m = p.max()
    return (p - (m + np.log(np.exp(p - m).sum()))).astype(np.float32)


def _check_weights(w_gen: float, w_disc: float) -> tuple[float, float]:
    w_gen, w_disc = float(w_gen), float(w_disc)
    if not (np.isfinite(w_gen) and np.isfinite(w_disc)) or w_gen < 0.0 or w_disc < 0.0:
        raise ValueError(f"generative_weight and discriminative_weight must be finite and non-negative, got {w_gen}, {w_disc}")
    return w_gen, w_disc


def check_labels(y: torch.Tensor, B: int) -> torch.Tensor:
    """Labels are an int64 tensor of B entries (values are checked on the device: -1 = unlabelled, else 0 .. C-1)."""
    if not isinstance(y, torch.Tensor) or y.dtype != torch.int64:
        raise ValueError(f"labels must be a torch.int64 tensor, got {getattr(y, 'dtype', type(y))}")
    if y.dim() != 1 or y.shape[0] != B:
        raise ValueError(f"labels must have shape ({B},), got {tuple(y.shape)}")
    return y


class ClassHead:
    """The device side of `ck_class_head` for one circuit: the prior, the statistics and their scratch."""

    def __init__(self, C: int, log_prior: np.ndarray | None, device: torch.device) -> None:
        self.C, self.device = int(C), device
        self.prior = None if log_prior is None else torch.from_numpy(log_prior).to(device)
        self.stats = torch.zeros(capi.CK_CLASS_NUM_STATS, dtype=torch.float64, device=device)
        self._partials = torch.empty(capi.CK_CLASS_MAX_BLOCKS * capi.CK_CLASS_NUM_STATS, dtype=torch.float64, device=device)

    def run(self, block: torch.Tensor, *, labels: torch.Tensor | None = None, w_gen: float = 1.0, w_disc: float = 1.0,
            inv_gb: float = 1.0, seed: torch.Tensor | None = None, log_post: torch.Tensor | None = None,
            log_evid: torch.Tensor | None = None, pred: torch.Tensor | None = None, stats: bool = False,
            bad_flag: torch.Tensor | None = None, stream: int | None = None) -> None:
        """`block`: the root fold's (B, stride) fp32 block; `seed` its gradient view of the same shape."""
        B, stride = int(block.shape[0]), int(block.shape[1])
        if block.dtype != torch.float32 or block.stride(1) != 1 or block.stride(0) != stride:
            raise ValueError("the class head reads a contiguous (B, stride) float32 block")
        if seed is not None and (tuple(seed.shape) != (B, stride) or not seed.is_contiguous()):
            raise ValueError("the seed is the root's (B, stride) gradient view")
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        capi.call("ck_class_head", block.data_ptr(), B, self.C, stride, ptr(labels), ptr(self.prior), w_gen, w_disc, inv_gb,
                  ptr(seed), ptr(log_post), ptr(log_evid), ptr(pred), ptr(self.stats) if stats else None,
                  ptr(self._partials) if stats else None, ptr(bad_flag), stream)


class HipClassifier:
    """Inference with a class-conditional circuit: ``log p(x | c)``, ``log p(c | x)``, ``argmax_c``, ``log p(x)`` and the
    scoring statistics, all with missing features where asked (`integrate_vars` and sentinel entries exactly as in
    `HipCircuit.forward`).  It owns a default `HipCircuit` (fused forward, unit padding as `HipCircuit` chooses); the head
    reads the first C units of the root's block, whatever its padded width.  One class (C = 1) is a valid edge."""

    def __init__(self, plan: Plan, tensors: Mapping[str, object], *, device: str | torch.device = "cuda:0", log_prior=None,
                 _classes: int | None = None, _prior: np.ndarray | None = None) -> None:
        # (`_classes`, `_prior`: `HipClassifierTrainer.classifier()` over a plan it padded -- the classes are the user's -- and
        #  with the trainer's prior as it was normalised, bit for bit)
        C = num_classes(plan) if _classes is None else int(_classes)
        prior = normalise_log_prior(log_prior, C) if _prior is None else _prior
        from .circuit import HipCircuit

        self.circuit = HipCircuit(plan, tensors, device=device)
        self.device = self.circuit.device
        self.num_classes = C
        self._head = ClassHead(C, prior, self.device)
        self._bad_label = torch.zeros(1, dtype=torch.int32, device=self.device)

    def _root(self, x: torch.Tensor, integrate_vars) -> torch.Tensor:
        """The root fold's (B, stride) block of one forward (a view of the arena)."""
        c = self.circuit
        if integrate_vars is not None:
            x = c._apply_integration_mask(x.to(self.device), integrate_vars)
        bd = c._run(x)
        p, f = int(c._out_pairs[0, 0]), int(c._out_pairs[0, 1])
        return bd.views[p][f]

    def class_log_likelihoods(self, x: torch.Tensor, integrate_vars=None) -> torch.Tensor:
        """``(B, C)``: ``log p(x_b | y = c)``."""
        return self._root(x, integrate_vars)[:, : self.num_classes].clone()

    def _query(self, x: torch.Tensor, integrate_vars, what: str) -> torch.Tensor:
        with torch.cuda.device(self.device):
            block = self._root(x, integrate_vars)
            B = int(block.shape[0])
            shape, dtype = {"log_post": ((B, self.num_classes), torch.float32), "log_evid": ((B,), torch.float32),
                            "pred": ((B,), torch.int64)}[what]
            out = torch.empty(shape, dtype=dtype, device=self.device)
            self._head.run(block, **{what: out})
        return out

    def predict_log_proba(self, x: torch.Tensor, integrate_vars=None) -> torch.Tensor:
        """``(B, C)``: ``log p(y = c | x_b)`` (NaN rows where ``log p(x_b)`` is not finite)."""
        return self._query(x, integrate_vars, "log_post")

    def predict(self, x: torch.Tensor, integrate_vars=None) -> torch.Tensor:
        """``(B,)`` int64: the most probable class, the lowest on ties (-1 where ``log p(x_b)`` is not finite)."""
        return self._query(x, integrate_vars, "pred")

    def log_evidence(self, x: torch.Tensor, integrate_vars=None) -> torch.Tensor:
        """``(B,)``: ``log p(x_b) = logsumexp_c (log p(x_b | c) + log p(c))``."""
        return self._query(x, integrate_vars, "log_evid")

    def score(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """The six fp64 statistics of a labelled batch (`STATS`: sums of the generative and discriminative terms, live /
        labelled / correct / dead rows) as a device tensor.  A label outside [-1, C) makes its row dead and
        `check_score_labels()` raise."""
        y = check_labels(y, int(x.shape[0])).to(self.device)
        with torch.cuda.device(self.device):
            self._head.run(self._root(x, None), labels=y, stats=True, bad_flag=self._bad_label)
        return self._head.stats.clone()

    def check_score_labels(self) -> None:
        """Raise ``IndexError`` if a `score` call since the last check held a label outside [-1, C) (a device read)."""
        if int(self._bad_label.item()) != 0:
            self._bad_label.zero_()
            raise IndexError(f"a batch held a label outside [-1, {self.num_classes})")


class HipClassifierTrainer(HipTrainer):
    """Training of a class-conditional circuit on ``L = -(1 / gB) sum_b (w_gen gen_b + w_disc disc_b)`` (module
    docstring): ``generative_weight=1, discriminative_weight=0`` is the class-conditional maximum likelihood of the
    reference's notebook, ``0, 1`` (the default) its cross-entropy; rows labelled -1 are unlabelled and contribute
    ``log p(x_b)`` to the generative term only (semi-supervised).

    A layer-wise `HipTrainer` (``fused=False, jobs=False``): the layer-wise forward, the class head writing the seed into
    the root's gradient view, the reverse launch list from there; flat buffers, optimizer, `gradients()`, `parameters()`,
    `skipped_steps` and the data-parallel reduction are the base trainer's.  A label outside [-1, C) is treated like an
    out-of-range category: the step changes nothing and `check_inputs()` reports it."""

    def __init__(self, plan: Plan, tensors: Mapping[str, object], *, device: str | torch.device = "cuda:0", lr: float = 0.01,
                 optimizer: str = "adam", betas: tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 generative_weight: float = 0.0, discriminative_weight: float = 1.0, log_prior=None,
                 pad_units: bool = False) -> None:
        C = num_classes(plan)
        self.generative_weight, self.discriminative_weight = _check_weights(generative_weight, discriminative_weight)
        prior = normalise_log_prior(log_prior, C)
        super().__init__(plan, tensors, device=device, lr=lr, optimizer=optimizer, betas=betas, eps=eps, pad_units=pad_units,
                         fused=False, jobs=False)
        self.num_classes = C
        self._log_prior = prior
        self._head = ClassHead(C, prior, self.device)

    # -- one step ------------------------------------------------------------------------------------------
    def loss_and_grads(self, x: torch.Tensor, y: torch.Tensor, *, global_batch: int | None = None) -> torch.Tensor:
        """Forward, class head, backward; gradients land in ``self.grads``.  Returns the six fp64 statistics of this
        shard (`STATS`) as a device tensor -- the head's own buffer, overwritten by the next call (clone it to keep it).
        ``global_batch``: see `TrainerSurface._global_batch`."""
        B = int(x.shape[0])
        labels = check_labels(y, B).to(self.device)
        gB = self._global_batch(B, global_batch)
        with torch.cuda.device(self.device):
            self._grads_current = True
            self.circuit._run(x)  # the layer-wise forward: every activation stays in the arena
            bd = self.circuit._bind(B)
            po, fo = int(self.circuit._out_pairs[0, 0]), int(self.circuit._out_pairs[0, 1])
            block = bd.views[po][fo]

            def seed(view: torch.Tensor, stream: int) -> None:
                self._head.run(block, labels=labels, w_gen=self.generative_weight, w_disc=self.discriminative_weight,
                               inv_gb=1.0 / gB, seed=view, stats=True, bad_flag=self.circuit._bad_input, stream=stream)

            self._backward(B, gB, seed)
        return self._head.stats

    def step(self, x: torch.Tensor, y: torch.Tensor, *, global_batch: int | None = None) -> torch.Tensor:
        """One optimisation step on this rank's shard; returns the six statistics (before the update; summed over the
        ranks when there are several).  Nothing is read back."""
        stats = self.loss_and_grads(x, y, global_batch=global_batch)
        alone = _world_size() <= 1
        # a bad label raised the circuit's own input flag (the head's bad_flag): the policy of an out-of-range category
        self._reduce_and_apply(self.circuit._bad_input, alone, latch=True)
        if not alone:
            _all_reduce_sum(stats)
        return stats

    def check_inputs(self) -> None:
        """Raise ``IndexError`` if a batch since the last check held a label outside [-1, C) or a category out of range;
        the steps on such batches changed nothing."""
        try:
            super().check_inputs()
        except IndexError as e:
            raise IndexError(f"{e}, or a label outside [-1, {self.num_classes})") from None

    def classifier(self) -> HipClassifier:
        """A `HipClassifier` over this trainer's parameter store: it sees every update without being rebuilt."""
        return HipClassifier(self.plan, self.circuit.store, device=self.device, _classes=self.num_classes, _prior=self._log_prior)
