"""The job graph of the job form of the training step (cirkit_amd/train_jobs.py), built from a folded plan without a device:
which SUM / MIX / sum-of-blocks jobs exist, the blocks they read and write, their forward and backward levels, the gradient
list of every job and input fold -- or the reason the plan does not take the job form.  tests/golden/job_graphs.json pins it.

A block is `("a", layer, fold)` -- a fold of a layer's activation -- or `("x", n)` -- the n-th extra block of a binding."""
from __future__ import annotations

import os
from dataclasses import dataclass, field

from . import _capi as capi
from .layers import HipCategoricalLayer, HipCPTLayer, HipGaussianLayer, HipHadamardLayer, HipSumLayer, HipTuckerLayer
from .plan import resolve_fold_index

MAX_LIST = 4  # a product of more blocks than this is materialised by an NSUM job
K = 64
FOLD_MIX_BWD = os.environ.get("CK_JOBS_FOLD_MIX", "1") != "0"  # (lab switch: 0 keeps a backward launch per mixing level)


@dataclass(slots=True)
class MixJob:
    """One fold of a mixing layer over H slots of S blocks each.  `folded`: the sum jobs under it do its backward (no `g`, `lb`)."""
    layer: int
    fold: int
    slots: list
    H: int
    S: int
    out: tuple
    gx0: int  # the first of its H gradient blocks ("x", gx0 + h)
    w: tuple
    theta: tuple
    lf: int
    folded: bool = False
    g: list | None = None
    lb: int | None = None


@dataclass(slots=True)
class MixRef:
    """The folded mixing fold a sum job serves: slot `h`, the other factors of that slot, whether the job leaves d w[:, h]."""
    job: MixJob
    h: int
    partners: list
    writer: bool


@dataclass(slots=True)
class SumJob:
    """One fold of a dense / CP-T layer: out = W . exp(sum of `ins`), backward one gradient block `gx` from the list `g`."""
    layer: int
    fold: int
    ins: list
    out: tuple
    gx: tuple
    w: tuple  # ("layer", i, fold) | ("node", i, node, fold): where the evaluated weight lives
    theta: tuple  # (tensor, fold)
    lf: int
    gather: tuple | None = None  # the (layer, fold) of a gathered Categorical layer the job reads the table of
    mix: MixRef | None = None
    g: list | None = None
    lb: int | None = None


@dataclass(slots=True)
class BlockSum:
    """out = the sum of `ins`: a kept product (forward, level `lf`) or a gradient list several jobs share (backward, `lb`)."""
    ins: list
    out: tuple | None
    lf: int | None = None
    lb: int | None = None


@dataclass(slots=True)
class ScalarFold:
    layer: int
    fold: int
    ins: list
    theta: tuple


@dataclass(slots=True)
class FinalMix:
    layer: int
    kids: list
    theta: tuple


@dataclass(slots=True)
class Root:
    folds: list[ScalarFold]  # in the order the final mixing layer reads them
    mix: FinalMix | None
    gx0: int
    zero: int  # (a block nobody writes)


@dataclass(slots=True)
class GaussFold:
    mean: tuple
    sd: tuple
    ss: bool  # stddev = scaled_sigmoid(tensor)
    vmin: float
    vmax: float


@dataclass(slots=True)
class InputGrad:
    """The gradient lists of an input layer's folds; `first`: the extra blocks they are gathered into (-1: its folds are jobs)."""
    first: int
    lists: list
    lb: int


@dataclass(slots=True)
class JobGraph:
    sum_jobs: list[SumJob] = field(default_factory=list)
    mix_jobs: list[MixJob] = field(default_factory=list)
    nsum_jobs: list[BlockSum] = field(default_factory=list)
    gsum_jobs: list[BlockSum] = field(default_factory=list)
    root: Root | None = None
    inputs: list[int] = field(default_factory=list)
    gauss: dict[int, list[GaussFold]] = field(default_factory=dict)  # Gaussian layers whose folds are backward jobs
    cat: set[int] = field(default_factory=set)  # Categorical layers whose folds are backward jobs
    gathered: set[int] = field(default_factory=set)  # Categorical layers never evaluated: their readers gather table rows
    input_g: dict[int, InputGrad] = field(default_factory=dict)
    n_extra: int = 0


def _expr(g, j: int, f: int):
    """The value of fold f of node j of a parameter graph as a nested tuple (op, node, fold, *operands)."""
    n = g.nodes[j]
    if n.op == "tensor":
        return ("tensor", j, f, n.config["tensor"])
    folds = [m.num_folds for m in g.nodes]
    kids = []
    for fi in n.inputs:
        pr = resolve_fold_index(fi, [folds[i] if i in fi.ids else 0 for i in range(max(fi.ids) + 1)]).reshape(-1, 2)
        kids.append(_expr(g, int(pr[f, 0]), int(pr[f, 1])))
    return (n.op, j, f, *kids)


def _out_expr(g, f: int):
    folds = [m.num_folds for m in g.nodes]
    pr = resolve_fold_index(g.output, [folds[i] if i in g.output.ids else 0 for i in range(max(g.output.ids) + 1)]).reshape(-1, 2)
    return _expr(g, int(pr[f, 0]), int(pr[f, 1]))


def _is_softmax_of_tensor(g, e) -> bool:
    return (e[0] == "softmax" and e[3][0] == "tensor" and int(g.nodes[e[1]].config["dim"]) == len(g.nodes[e[1]].shape) - 1)


class _NotJobForm(Exception):
    """The plan does not take the job form: the message is the reason `JobStep.why` reports."""


def build_job_graph(plan, layers, children, out_pairs, is_complex: bool, param_ops, *, max_list: int = MAX_LIST,
                    fold_mix_bwd: bool = FOLD_MIX_BWD) -> JobGraph | str:
    """The job graph of a plan over its `layers` (children, out_pairs: as `HipCircuit` resolves them), or why it has none."""
    if is_complex or len(out_pairs) != 1:
        return "needs a real circuit with one output"
    b = _Builder(plan, layers, children, (int(out_pairs[0, 0]), int(out_pairs[0, 1])), param_ops, max_list)
    try:
        b.forward_jobs()
        b.root()
        b.gathered_categoricals()
        if fold_mix_bwd:
            b.fold_mixing()
        b.gradient_lists()
        b.backward_levels()
        b.input_gradients()
    except _NotJobForm as e:
        return str(e)
    return b.g


class _Builder:
    """The state the phases of `build_job_graph` share."""

    def __init__(self, plan, layers, children, out, param_ops, max_list: int) -> None:
        self.plan, self.layers, self.children, self.out, self.param_ops, self.max_list = plan, layers, children, out, param_ops, max_list
        self.g = JobGraph()
        self.vals: dict[tuple[int, int], list] = {}  # (layer, fold) -> the blocks whose sum is its value
        self.producer: dict[tuple, SumJob | MixJob | BlockSum] = {}  # block -> the job that writes it (forward)
        self.gsrc: dict[tuple, list] = {}  # block -> the gradient blocks (or ("ref", kept product)) it receives
        self.used: set[tuple[str, int]] = set()  # (tensor, fold)s that some job differentiates
        self.scalars: dict[tuple[int, int], ScalarFold] = {}
        self.final_mix: FinalMix | None = None
        self.writer: dict[tuple, SumJob | MixJob | BlockSum] = {}  # gradient block -> the job that writes it (backward)

    # ---- shared helpers ---------------------------------------------------------------------------------------------------
    def extra(self, n: int = 1) -> int:
        first = self.g.n_extra
        self.g.n_extra += n
        return first

    def try_claim(self, theta) -> bool:
        fresh = theta not in self.used
        self.used.add(theta)
        return fresh

    def claim(self, name: str, fold: int) -> tuple:
        if not self.try_claim((name, fold)):
            raise _NotJobForm(f"tensor {name} is shared")
        return (name, fold)

    def feed(self, blocks, gid) -> None:
        for x in blocks:
            self.gsrc.setdefault(x, []).append(gid)

    def level_of(self, blocks) -> int:
        return 1 + max((self.producer[x].lf if x in self.producer else 0) for x in blocks)

    def gather(self, ch_f) -> list:
        return [x for p, q in ch_f for x in self.vals[(int(p), int(q))]]

    def shorten(self, lst: list, out: tuple | None = None) -> list:
        """More than `max_list` blocks: one NSUM job materialises their sum; every member's gradient is the sum's."""
        if len(lst) <= self.max_list:
            return lst
        out = out or ("x", self.extra())
        job = BlockSum(list(lst), out, lf=self.level_of(lst))
        self.g.nsum_jobs.append(job)
        self.producer[out] = job
        self.feed(lst, ("ref", out))
        return [out]

    def add_sum(self, i: int, f: int, ins: list, w: tuple, theta: tuple) -> None:
        job = SumJob(i, f, ins, ("a", i, f), ("x", self.extra()), w, theta, self.level_of(ins))
        self.g.sum_jobs.append(job)
        self.producer[job.out] = self.writer[job.gx] = job
        self.feed(ins, job.gx)

    def add_mix(self, i: int, f: int, slots: list, out: tuple, w: tuple, theta: tuple) -> None:
        S = max(len(s) for s in slots)
        if any(len(s) != S for s in slots):  # uniform slot length: longer products are kept
            slots = [self.shorten(s) if len(s) > 1 else s for s in slots]
            S = max(len(s) for s in slots)
            if any(len(s) != S for s in slots):
                raise NotImplementedError("mixing slots that are products of different numbers of blocks")
        H = len(slots)
        job = MixJob(i, f, slots, H, S, out, self.extra(H), w, theta, self.level_of([x for s in slots for x in s]))
        self.g.mix_jobs.append(job)
        self.producer[out] = job
        for h, s in enumerate(slots):  # (a folded mixing fold writes no gradient block: nobody looks its entries up)
            self.feed(s, ("x", job.gx0 + h))
            self.writer[("x", job.gx0 + h)] = job

    # ---- 1. forward jobs, layer by layer ----------------------------------------------------------------------------------
    def forward_jobs(self) -> None:
        for i, (spec, l) in enumerate(zip(self.plan.layers, self.layers)):
            if isinstance(l, HipCategoricalLayer) and type(l) is HipCategoricalLayer:
                self.categorical(i, l)
            elif isinstance(l, HipGaussianLayer):
                self.gaussian(i, l)
            elif isinstance(l, HipHadamardLayer):
                for f in range(l.num_folds):  # (a short product is virtual: it is the list)
                    self.vals[(i, f)] = self.shorten(self.gather(self.children[i][f]), ("a", i, f))
            elif isinstance(l, (HipSumLayer, HipCPTLayer)) and not isinstance(l, HipTuckerLayer):
                self.sum_layer(i, spec, l)
            else:
                raise _NotJobForm(f"layer {i}: layer type {spec.type!r}")
        # (tensor folds nobody reads keep a zero gradient: the flat gradient buffer starts as zeros and only claimed folds are written)

    def categorical(self, i: int, l) -> None:
        if l.num_output_units != K or l.probs is None or l.probs.softmax_source() is None:
            raise _NotJobForm(f"layer {i}: Categorical layers need 64 units and probs = softmax(tensor)")
        name = l.probs.graph.nodes[0].config["tensor"]
        for f in range(l.num_folds):
            self.vals[(i, f)] = [("a", i, f)]
            self.claim(name, f)
        self.g.inputs.append(i)
        if l.scope_idx.shape[1] == 1 and ((l.num_categories + 1) * 65 + 1280) * 4 + (2 * 16 * ((l.num_categories + 16) // 16) + 4100) * 4 <= 160 * 1024:
            self.g.cat.add(i)  # its folds' backward (+ optimizer + next table) is one launch of jobs (`ck_jobs_cat_bwd`)

    def gaussian(self, i: int, l) -> None:
        if l.num_output_units != K or l.log_partition is not None or (set(l.mean.ops) | set(l.stddev.ops)) - self.param_ops:
            raise _NotJobForm(f"layer {i}: Gaussian layers need 64 units, no log-partition and plain parameters")
        for f in range(l.num_folds):
            self.vals[(i, f)] = [("a", i, f)]
        self.g.inputs.append(i)
        # mean = a tensor, stddev = a tensor or its scaled sigmoid (what the templates build): the fold's backward is a job of
        # its own (`ck_jobs_gauss_bwd`) reading its gradient list; anything else takes the layer-wise launches
        recs = []
        for f in range(l.num_folds):
            em, es = _out_expr(l.mean.graph, f), _out_expr(l.stddev.graph, f)
            ss = es[0] == "scaled_sigmoid"
            et = es[3] if ss else es
            if em[0] != "tensor" or et[0] != "tensor" or l.scope_idx.shape[1] != 1:
                return
            cfg = l.stddev.graph.nodes[es[1]].config if ss else {}
            recs.append(GaussFold((em[3], em[2]), (et[3], et[2]), ss, float(cfg.get("vmin", 0.0)), float(cfg.get("vmax", 1.0))))
        if all(self.try_claim(r.mean) and self.try_claim(r.sd) for r in recs):
            self.g.gauss[i] = recs

    def sum_layer(self, i: int, spec, l) -> None:
        ch, F = self.children[i], l.num_folds
        Ki, Ko = l.num_input_units, l.num_output_units
        prod = l._mode == capi.CK_SUM_PROD or l.arity == 1
        if Ko == 1 and Ki == K and prod and l.weight.softmax_source() is not None:
            name = l.weight.graph.nodes[0].config["tensor"]
            for f in range(F):
                theta = self.claim(name, f)
                self.scalars[(i, f)] = ScalarFold(i, f, self.shorten(self.gather(ch[f])), theta)
        elif Ko == 1 and Ki == 1 and l._mixing and l.weight.mixing_softmax_source() is not None and F == 1 and i == self.out[0]:
            theta = self.claim(l.weight.graph.nodes[0].config["tensor"], 0)
            kids = [(int(p), int(q)) for p, q in ch[0]]
            if any(k not in self.scalars for k in kids) or len(set(kids)) != len(kids):
                raise _NotJobForm("the final mixing layer must read distinct scalar sum folds")
            self.final_mix = FinalMix(i, kids, theta)
        elif Ki == K and Ko == K and l._mixing and l.weight.mixing_softmax_source() is not None:
            if l.arity > 16:
                raise _NotJobForm(f"layer {i}: a mixing layer over more than 16 slots")
            name = l.weight.graph.nodes[0].config["tensor"]
            for f in range(F):
                theta = self.claim(name, f)
                self.add_mix(i, f, [self.vals[(int(p), int(q))] for p, q in ch[f]], ("a", i, f), ("layer", i, f), theta)
                self.vals[(i, f)] = [("a", i, f)]
        elif Ki == K and Ko == K and prod and l.weight.softmax_source() is not None:
            name = l.weight.graph.nodes[0].config["tensor"]
            for f in range(F):
                theta = self.claim(name, f)
                self.add_sum(i, f, self.shorten(self.gather(ch[f])), ("layer", i, f), theta)
                self.vals[(i, f)] = [("a", i, f)]
        elif Ki == K and Ko == K and l._mode == capi.CK_SUM_CAT and l.arity > 1 and not l._mixing:
            if l.arity > 16:
                raise _NotJobForm(f"layer {i}: more than 16 slots")
            for f in range(F):
                self.mixing_or_collapsed_fold(i, f, l)
                self.vals[(i, f)] = [("a", i, f)]
        else:
            raise _NotJobForm(f"layer {i}: a {spec.type} layer of {Ki} -> {Ko} units, arity {l.arity}, weight {l.weight.ops}")

    def mixing_or_collapsed_fold(self, i: int, f: int, l) -> None:
        """A mixing weight, or a dense weight times a mixing weight (the collapsed pair: a MIX job feeding a SUM job)."""
        g = l.weight.graph
        e = _out_expr(g, f)
        slots = [self.vals[(int(p), int(q))] for p, q in self.children[i][f]]
        if e[0] == "mixing_weight" and _is_softmax_of_tensor(g, e[3]):
            sm = e[3]
            self.add_mix(i, f, slots, ("a", i, f), ("node", i, sm[1], sm[2]), self.claim(sm[3][3], sm[3][2]))
        elif e[0] == "matmul" and _is_softmax_of_tensor(g, e[3]) and e[4][0] == "mixing_weight" and _is_softmax_of_tensor(g, e[4][3]):
            sd, sm = e[3], e[4][3]
            if not self.try_claim((sd[3][3], sd[3][2])) or not self.try_claim((sm[3][3], sm[3][2])):
                raise _NotJobForm(f"tensors of layer {i} are shared")
            mid = ("x", self.extra())
            self.add_mix(i, f, slots, mid, ("node", i, sm[1], sm[2]), (sm[3][3], sm[3][2]))
            self.add_sum(i, f, [mid], ("node", i, sd[1], sd[2]), (sd[3][3], sd[3][2]))
        else:
            raise _NotJobForm(f"layer {i}: weight parameterisation {l.weight.ops}")

    # ---- 2. the root: the scalar folds in the order the final mixing layer reads them ----------------------------------------
    def root(self) -> None:
        if self.final_mix is not None:
            order = self.final_mix.kids
            if set(order) != set(self.scalars):
                raise _NotJobForm("scalar sum folds outside the final mixing layer")
        else:
            if len(self.scalars) != 1 or self.out not in self.scalars:
                raise _NotJobForm("the circuit must end in a scalar sum fold or a final mixing layer over scalar sum folds")
            order = [self.out]
        if len(order) > 16:
            raise _NotJobForm("more than 16 scalar folds under the final mixing layer")
        g0 = self.extra(len(order))
        self.g.root = Root([self.scalars[k] for k in order], self.final_mix, g0, self.extra())
        for r, sc in enumerate(self.g.root.folds):
            self.feed(sc.ins, ("x", g0 + r))
            self.writer[("x", g0 + r)] = BlockSum([], None, lb=0)  # (the root is backward level 0)
        if not self.g.sum_jobs:
            raise _NotJobForm("no 64-unit sum layer")

    # ---- 3. a Categorical layer whose folds are only read by sum jobs, each as the job's single input, is never evaluated:
    #         those jobs gather the rows of its log-probability table themselves ---------------------------------------------
    def gathered_categoricals(self) -> None:
        g = self.g
        other = [j.ins for j in g.sum_jobs if len(j.ins) != 1] + [s for j in g.mix_jobs for s in j.slots]
        other += [j.ins for j in g.nsum_jobs] + [sc.ins for sc in g.root.folds]
        spoiled = {x[1] for blocks in other for x in blocks if x[0] == "a"}
        g.gathered = {i for i in g.cat if i not in spoiled and i != self.out[0]}
        for j in g.sum_jobs:
            x = j.ins[0]
            if len(j.ins) == 1 and x[0] == "a" and x[1] in g.gathered:
                j.gather = (x[1], x[2])

    # ---- 4. a mixing fold whose every factor is the output of a sum job that nobody else reads has no backward launch: each
    #         of those sum jobs forms its own gradient from the MIXING fold's gradient list (ck_sum_job.mix_out), and one job
    #         per slot leaves d w[:, h]; the softmax behind the coefficients is differentiated by one launch for all such folds
    #         at the end ----------------------------------------------------------------------------------------------------
    def fold_mixing(self) -> None:
        sum_of = {j.out: j for j in self.g.sum_jobs}
        for r in self.g.mix_jobs:
            ok = r.S <= 4
            for h, sl in enumerate(r.slots):
                for x in sl:
                    if x not in sum_of or self.gsrc.get(x) != [("x", r.gx0 + h)] or sum_of[x].mix is not None:
                        ok = False
            if not ok:
                continue
            r.folded = True
            for h, sl in enumerate(r.slots):
                for k, x in enumerate(sl):
                    sum_of[x].mix = MixRef(r, h, [y for y in sl if y is not x], k == 0)

    # ---- 5. gradient lists: expand references to kept products, then materialise lists that several readers share ----------
    def sources(self, x, memo: dict) -> tuple:
        if x not in memo:
            out: list = []
            for gsid in self.gsrc.get(x, []):
                out += list(self.sources(gsid[1], memo)) if gsid[0] == "ref" else [gsid]
            memo[x] = tuple(out)
        return memo[x]

    def gradient_lists(self) -> None:
        g = self.g
        self.live = g.sum_jobs + [r for r in g.mix_jobs if not r.folded]  # the jobs with a backward launch
        memo: dict[tuple, tuple] = {}
        readers: dict[tuple, int] = {}
        gof = {id(j): j.mix.job.out if isinstance(j, SumJob) and j.mix else j.out for j in self.live}  # whose gradient list a job reads
        wanted = list(gof.values()) + [("a", i, f) for i in g.inputs for f in range(self.layers[i].num_folds)]
        for x in wanted:
            readers[self.sources(x, memo)] = readers.get(self.sources(x, memo), 0) + 1
        shared: dict[tuple, tuple] = {}
        for lst, n in readers.items():
            if len(lst) >= 3 and n >= 2:
                shared[lst] = ("x", self.extra())
                g.gsum_jobs.append(BlockSum(list(lst), shared[lst]))
                self.writer[shared[lst]] = g.gsum_jobs[-1]
        self.grad_list = lambda x: [shared[memo[x]]] if memo[x] in shared else list(memo[x])
        for j in self.live:
            j.g = self.grad_list(gof[id(j)])
            if not j.g:
                raise _NotJobForm(f"layer {j.layer} fold {j.fold} feeds nothing")

    # ---- 6. backward levels: the root is level 0; a job follows the writers of its gradient list -----------------------------
    def lb(self, j) -> int:
        if j.lb is None:
            j.lb = 1 + max(self.lb(self.writer[gsid]) for gsid in (j.ins if isinstance(j, BlockSum) else j.g))
        return j.lb

    def backward_levels(self) -> None:
        for j in self.live + self.g.gsum_jobs:
            self.lb(j)

    # ---- 7. the gradient of every input-layer fold, gathered into a contiguous (F, B, 64) block per layer for its backward ----
    def input_gradients(self) -> None:
        g = self.g
        for i in g.inputs:
            Fi = self.layers[i].num_folds
            first = -1 if (i in g.gauss or i in g.cat) else self.extra(Fi)
            lists = [self.grad_list(("a", i, f)) for f in range(Fi)]
            if any(not lst for lst in lists):
                raise _NotJobForm(f"input layer {i} has a fold nobody reads")
            g.input_g[i] = InputGrad(first, lists, 1 + max(self.lb(self.writer[gsid]) for lst in lists for gsid in lst))
