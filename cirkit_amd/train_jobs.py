"""The training step as LEVEL launches over JOBS, for circuits made of 64-unit dense / CP-T / mixing / Hadamard layers.

The reference trains by autograd through its layer-by-layer forward (notebooks/learning-a-circuit.ipynb cell 18 over
layers/inner.py:126-127, 266-273, optimized.py:171-178, semiring.py:383-408, parameters/nodes.py:764-772, 847-862).  This
module is the host side of cirkit_amd/csrc/ck_jobs.hip: it turns a folded plan into

* SUM jobs -- one fold of a dense / CP-T layer (64 -> 64 units): input = the sum of a list of blocks (a Hadamard product in
  log space: the product layers are never evaluated, their folds are LISTS), output one block, backward one gradient block;
* MIX jobs -- one fold of a mixing layer over H slots (each a list of blocks); a collapsed Sum -> Sum pair (a MatMul weight,
  nodes.py:802-805) is evaluated as what it was before the reference's optimizer collapsed it: a MIX job feeding a SUM job;
* NSUM jobs -- products that are kept (more than `MAX_LIST` factors) and gradients that several jobs read;
* the ROOT launch -- scalar sum folds + the final mixing layer + the log-likelihood sum + their backward;

orders them in levels (one launch per kind and level), and records the whole step -- parameter prologue, input layers, forward
levels, root, backward levels, input-layer backward -- as ONE native launch list per batch size (`ck_program`).  Every gradient
block has one writer; readers add the blocks of their list.  Parameter gradients leave the job epilogues as d theta (the softmax
behind every weight is differentiated by the workgroup that holds dW).  `HipTrainer` owns the buffers, the optimizer and the
collective; `JobStep(trainer).why` says why a plan does not take this form (then the layer-wise launch list runs).

The jobs, their lists and levels: cirkit_amd/job_graph.py (no device needed); how a level's jobs are cut into the units of a
launch: cirkit_amd/job_layout.py; this module binds both to a batch size (`_Tables`) and issues the launches."""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import _capi as capi
from .job_graph import K, MixJob, SumJob, build_job_graph
from .job_layout import mix_split, sum_layout
from .layers import HipCategoricalLayer


@dataclass(slots=True)
class Launch:
    """One launch of a bound step, in issue order."""
    kind: str  # nsum | sum_fwd | mix_fwd | root | sum_bwd | mix_bwd | mix_params | gauss_bwd | cat_bwd | input_bwd
    tables: dict[int, torch.Tensor] | None = None  # mode -> the device job table (forward launches: mode 1 only)
    n: int = 1  # units (rows of the table)
    param: int = 0  # sum_bwd: waves per workgroup; mix_fwd / mix_bwd: the largest H; cat_bwd: the layer's categories
    layer: int = -1  # the input layer of a gauss_bwd / cat_bwd / input_bwd launch

    def table(self, mode: int) -> int:
        return self.tables.get(mode, self.tables[1]).data_ptr()


class _Tables:
    """The binding context of one batch size: block addresses, the pool of block lists, the device table of every launch."""

    def __init__(self, js: JobStep, bd, B: int) -> None:
        self.g, self.tr, self.c, self.bd, self.B = js.graph, js.tr, js.c, bd, B
        self.dev, self.n_cu, self.tiles, self.blk = self.c.device, self.c._n_cu, (B + 31) // 32, B * K
        self.keep: list[torch.Tensor] = []
        self.extra = self.zeros(max(1, self.g.n_extra) * self.blk)
        self.x0 = self.extra.data_ptr()
        self.pool: list[int] = []
        self.folded = [r for r in self.g.mix_jobs if r.folded]
        offs = np.cumsum([0] + [K * r.H for r in self.folded])
        mix_dw = self.zeros(max(1, int(offs[-1])))  # d w of the folded mixing folds, left by the sum jobs under them
        self.mix_dw = {id(r): mix_dw.data_ptr() + 4 * int(o) for r, o in zip(self.folded, offs)}

    def zeros(self, n: int, dtype=torch.float32) -> torch.Tensor:
        self.keep.append(torch.zeros(n, dtype=dtype, device=self.dev))
        return self.keep[-1]

    def addr(self, x) -> int:
        if x[0] == "a":
            v = self.bd.views[x[1]]
            return v.data_ptr() + x[2] * self.B * v.shape[2] * 4
        return self.x0 + x[1] * self.blk * 4

    def put(self, blocks) -> tuple[int, int]:
        off = len(self.pool)
        self.pool.extend(self.addr(x) for x in blocks)
        return off, len(blocks)

    def weight_ptr(self, w) -> int:
        if w[0] == "layer":
            t, fold = self.c.layers[w[1]]._w, w[2]
        else:  # the evaluated softmax node of a parameter graph that `prepare` evaluates node by node
            t, fold = self.c.layers[w[1]].weight._last_outs[w[2]], w[3]
        return t.data_ptr() + fold * (t.numel() // t.shape[0]) * 4

    def param_ptrs(self, theta) -> tuple[int, int, int, int]:
        """(theta, m1, m2, d theta) of a tensor fold: what every table's parameter columns hold."""
        name, fold = theta
        m1, m2 = self.tr._moments.get(name, (None, None))
        return tuple(0 if t is None else t.data_ptr() + fold * (t.numel() // t.shape[0]) * 4
                     for t in (self.c.store[name], m1, m2, self.tr.grads[name]))

    def weight_cols(self, j) -> dict:
        """The weight and parameter columns of a sum / mixing table row."""
        th, m1, m2, dth = self.param_ptrs(j.theta)
        w = self.weight_ptr(j.w)
        return dict(w=w, w_out=w, theta=th, m1=m1, m2=m2, dtheta=dth)

    def upload(self, kind: str, tab: np.ndarray, both_modes: bool, **kw) -> Launch:
        """The launch over the DEVICE copy of a job table -- for the backward launches one copy per mode (1: d theta to the
        flat gradient, 2: the optimizer's update in the epilogue)."""
        out = {}
        for mode in ((1, 2) if both_modes else (1,)):
            if both_modes:
                tab["mode"] = mode
            out[mode] = torch.from_numpy(tab.view(np.uint8).reshape(len(tab), -1).copy()).to(self.dev)
        self.keep.extend(out.values())
        return Launch(kind, out, len(tab), **kw)

    def fill_splits(self, rows: np.ndarray, rows_per: int, fields: dict) -> None:
        """The table rows of one job: `fields` in each, the row range of its own."""
        for k, v in fields.items():
            rows[k] = v
        rows["split"], rows["n_split"], rows["mode"] = np.arange(len(rows)), len(rows), 1
        rows["row0"] = rows["split"] * rows_per
        rows["row1"] = np.minimum(self.B, rows["row0"] + rows_per)

    def sum_table(self, jobs: list[SumJob], backward: bool) -> Launch:
        B = self.B
        splits, waves = sum_layout(len(jobs), self.tiles, self.n_cu, backward)
        rows_of = [-(-self.tiles // s) * 32 for s in splits]  # (a job's pieces: whole 32-row tiles, as equal as they come)
        first_unit = np.cumsum([0] + [-(-B // rp) for rp in rows_of])
        n_units = int(first_unit[-1])
        tab = np.zeros(n_units, dtype=np.dtype(capi.SUM_JOB_DTYPE))
        part = tick = None
        if backward and n_units > len(jobs):
            part, tick = self.zeros(n_units * 4096), self.zeros(len(jobs), torch.int32)
        for n, j in enumerate(jobs):
            u0, u1 = int(first_unit[n]), int(first_unit[n + 1])
            f = self.weight_cols(j)
            if j.gather is not None:  # the input is a Categorical fold: the pool entry is its table, rows picked by the batch column
                gl, gf = self.c.layers[j.gather[0]], j.gather[1]
                f["C"], f["xrow"] = gl.num_categories, self.bd.xt_i.data_ptr() + int(gl.scope_idx[gf, 0]) * B * 4
                f["in_off"], f["n_in"] = len(self.pool), 1
                self.pool.append(gl._table.data_ptr() + gf * (gl.num_categories + 1) * K * 4)
            else:
                f["in_off"], f["n_in"] = self.put(j.ins)
            f["g_off"], f["n_g"] = self.put(j.g) if backward else (0, 0)
            f["out"], f["gx"] = self.addr(j.out), self.addr(j.gx)
            if backward and j.mix is not None:
                mj = j.mix.job
                f["partner_off"], f["n_partner"] = self.put(j.mix.partners)
                f["mix_out"], f["mix_w"], f["mix_h"], f["mix_H"] = self.addr(mj.out), self.weight_ptr(mj.w), j.mix.h, mj.H
                f["mix_dw"] = self.mix_dw[id(mj)] if j.mix.writer else 0
            if part is not None and u1 - u0 > 1:
                f["part"], f["ticket"] = part.data_ptr() + u0 * 4096 * 4, tick.data_ptr() + n * 4
            self.fill_splits(tab[u0:u1], rows_of[n], f)
        return self.upload("sum_bwd" if backward else "sum_fwd", tab, backward, param=waves)

    def mix_table(self, jobs: list[MixJob], backward: bool) -> Launch:
        hmax = max(j.H for j in jobs)
        hpad = 2 if hmax <= 2 else 4 if hmax <= 4 else 8 if hmax <= 8 else 16
        ns, rows_per = mix_split(len(jobs), self.B, self.n_cu, backward, int(os.environ.get("CK_MIX_FWD_WG", "8")))
        tab = np.zeros(len(jobs) * ns, dtype=np.dtype(capi.MIX_JOB_DTYPE))
        part = tick = None
        if backward and ns > 1:
            part, tick = self.zeros(len(jobs) * ns * K * hpad), self.zeros(len(jobs), torch.int32)
        for n, j in enumerate(jobs):
            f = self.weight_cols(j)
            f["in_off"], _ = self.put([x for s in j.slots for x in s])
            f["g_off"], f["n_g"] = self.put(j.g) if backward else (0, 0)
            f["out"], f["gx"], f["H"], f["S"] = self.addr(j.out), self.addr(("x", j.gx0)), j.H, j.S
            if part is not None:
                f["part"], f["ticket"] = part.data_ptr() + n * ns * K * hpad * 4, tick.data_ptr() + n * 4
            self.fill_splits(tab[n * ns:(n + 1) * ns], rows_per, f)
        return self.upload("mix_bwd" if backward else "mix_fwd", tab, backward, param=hmax)

    def mix_params_table(self) -> Launch:
        """The coefficients of the mixing folds without a backward launch: one launch for all of them."""
        tab = np.zeros(len(self.folded), dtype=np.dtype(capi.MIX_JOB_DTYPE))
        for r, j in zip(tab, self.folded):
            for k, v in self.weight_cols(j).items():
                r[k] = v
            r["part"], r["H"], r["mode"] = self.mix_dw[id(j)], j.H, 1
        return self.upload("mix_params", tab, True)

    def nsum_table(self, kind: str, items: list[tuple[list, int]], **kw) -> Launch:
        tab = np.zeros(len(items), dtype=np.dtype(capi.NSUM_JOB_DTYPE))
        for r, (ins, out) in zip(tab, items):
            r["in_off"], r["n_in"] = self.put(ins)
            r["out"] = out
        return self.upload(kind, tab, False, **kw)

    def gauss_table(self, i: int) -> Launch:
        l = self.c.layers[i]
        mean, stddev, _ = l._vals
        tab = np.zeros(len(self.g.gauss[i]), dtype=np.dtype(capi.GAUSS_JOB_DTYPE))
        for f, (r, rec, lst) in enumerate(zip(tab, self.g.gauss[i], self.g.input_g[i].lists)):
            r["th_mean"], r["m1_mean"], r["m2_mean"], r["dmean"] = self.param_ptrs(rec.mean)
            r["th_sd"], r["m1_sd"], r["m2_sd"], r["dsd"] = self.param_ptrs(rec.sd)
            r["mean"], r["stddev"] = mean.data_ptr() + f * K * 4, stddev.data_ptr() + f * K * 4
            r["x"] = self.bd.xt.data_ptr() + int(l.scope_idx[f, 0]) * self.B * 4
            r["mean_out"] = 0 if r["mean"] == r["th_mean"] else r["mean"]
            r["sd_out"] = r["stddev"]
            r["g_off"], r["n_g"] = self.put(lst)
            r["vmin"], r["vmax"], r["has_ss"], r["mode"] = rec.vmin, rec.vmax, 1 if rec.ss else 0, 1
        return self.upload("gauss_bwd", tab, True, layer=i)

    def cat_table(self, i: int) -> Launch:
        l = self.c.layers[i]
        name = l.probs.graph.nodes[0].config["tensor"]
        tab = np.zeros(l.num_folds, dtype=np.dtype(capi.CAT_JOB_DTYPE))
        for f, (r, lst) in enumerate(zip(tab, self.g.input_g[i].lists)):
            r["theta"], r["m1"], r["m2"], r["dtheta"] = self.param_ptrs((name, f))
            r["table"] = l._table.data_ptr() + f * (l.num_categories + 1) * K * 4
            r["x"] = self.bd.xt_i.data_ptr() + int(l.scope_idx[f, 0]) * self.B * 4
            r["theta_out"], r["table_out"] = r["theta"], r["table"]
            r["g_off"], r["n_g"] = self.put(lst)
            r["mode"] = 1
        return self.upload("cat_bwd", tab, True, layer=i, param=l.num_categories)

    def input_table(self, i: int) -> Launch:
        ig = self.g.input_g[i]
        if i in self.g.gauss or i in self.g.cat:
            return self.gauss_table(i) if i in self.g.gauss else self.cat_table(i)
        return self.nsum_table("input_bwd", [(lst, self.x0 + (ig.first + f) * self.blk * 4) for f, lst in enumerate(ig.lists)], layer=i)

    def launches(self) -> list[Launch]:
        """Every launch in issue order: per level the kept products / shared gradients, the sum jobs, the mixing jobs."""
        g = self.g

        def by_level(jobs: list, key: str) -> dict[int, list]:
            out: dict[int, list] = {}
            for j in jobs:
                out.setdefault(getattr(j, key), []).append(j)
            return out

        def level_launches(nsum: dict, sums: dict, mixes: dict, inputs: dict, backward: bool) -> list[Launch]:
            out = []
            for lv in sorted(set(nsum) | set(sums) | set(mixes) | set(inputs)):
                if lv in nsum:
                    out.append(self.nsum_table("nsum", [(j.ins, self.addr(j.out)) for j in nsum[lv]]))
                if lv in sums:
                    out.append(self.sum_table(sums[lv], backward))
                if lv in mixes:
                    out.append(self.mix_table(mixes[lv], backward))
                out += [self.input_table(i) for i in inputs.get(lv, [])]
            return out

        bi: dict[int, list[int]] = {}
        for i, ig in g.input_g.items():
            bi.setdefault(ig.lb, []).append(i)
        out = level_launches(by_level(g.nsum_jobs, "lf"), by_level(g.sum_jobs, "lf"), by_level(g.mix_jobs, "lf"), {}, False)
        out.append(Launch("root"))
        out += level_launches(by_level(g.gsum_jobs, "lb"), by_level(g.sum_jobs, "lb"),
                              by_level([r for r in g.mix_jobs if not r.folded], "lb"), bi, True)
        return out + ([self.mix_params_table()] if self.folded else [])

    def root(self, opt) -> dict[int, capi.RootLaunch]:
        """The root launch's arguments per mode (after every table: its lists close the pool, which is uploaded here)."""
        c, bd, B, root = self.c, self.bd, self.B, self.g.root
        R = len(root.folds)
        rin = np.zeros((2, R), dtype=np.int32)
        ptrs = np.zeros((6, R), dtype=np.uint64)  # w, dtheta, theta, m1, m2, w_out
        S_root = max(len(sc.ins) for sc in root.folds)
        for r, sc in enumerate(root.folds):  # (lists of one length: shorter ones are padded with the block of zeros)
            rin[0, r], rin[1, r] = self.put(list(sc.ins) + [("x", root.zero)] * (S_root - len(sc.ins)))
            w = c.layers[sc.layer]._w.data_ptr() + sc.fold * K * 4
            th, m1, m2, dth = self.param_ptrs(sc.theta)
            ptrs[:, r] = (w, dth, th, m1, m2, w)
        rin_d = torch.from_numpy(rin).to(self.dev)
        ptrs_d = torch.from_numpy(ptrs.view(np.int64)).to(self.dev)
        n_wg = int(max(1, min(64, B // 4)))  # (a row per wave up to 256 rows: the launch is a chain of row-long round trips)
        rpart, rtick, self.seed = self.zeros(n_wg * 1042), self.zeros(1, torch.int32), self.zeros(B)
        self.pool_d = torch.from_numpy(np.asarray(self.pool, dtype=np.uint64).view(np.int64)).to(self.dev)
        self.keep.extend([rin_d, ptrs_d, self.pool_d])
        po, fo = int(c._out_pairs[0, 0]), int(c._out_pairs[0, 1])
        validate = c.validate_inputs and c._int_input
        out = {}
        for mode in (1, 2):
            ra = out[mode] = capi.RootLaunch()
            ra.pool, ra.in_off, ra.n_in = self.pool_d.data_ptr(), rin_d[0].data_ptr(), rin_d[1].data_ptr()
            ra.w, ra.dtheta_w, ra.theta_w = ptrs_d[0].data_ptr(), ptrs_d[1].data_ptr(), ptrs_d[2].data_ptr()
            ra.m1_w, ra.m2_w, ra.w_out = ptrs_d[3].data_ptr(), ptrs_d[4].data_ptr(), ptrs_d[5].data_ptr()
            ra.out = bd.views[po][fo].data_ptr()
            ra.gx, ra.seed, ra.ll = self.x0 + root.gx0 * self.blk * 4, self.seed.data_ptr(), bd.ll.data_ptr()
            ra.part, ra.ticket = rpart.data_ptr(), rtick.data_ptr()
            if root.mix is not None:
                ra.theta_c, ra.m1_c, ra.m2_c, ra.dtheta_c = self.param_ptrs(root.mix.theta)
                ra.c = ra.c_out = c.layers[root.mix.layer]._w.data_ptr()
            # mode 1: the circuit's own flag (latched after the step by the trainer); mode 2: `ck_opt_tick` has moved it into
            # the optimizer state's skip_now by the time the root launch runs
            ra.opt = opt.ptr if mode == 2 else None
            ra.bad_flag = opt.skip_now_ptr if mode == 2 else (c._bad_input.data_ptr() if validate else None)
            ra.seed_const, ra.R, ra.B, ra.mode, ra.n_wg, ra.S = 0.0, R, B, mode, n_wg, S_root
        return out


class JobStep:
    """Structure (independent of the batch size: `graph`) + per-batch-size bindings of the job form of a training step."""

    def __init__(self, trainer) -> None:
        self.tr = trainer
        c = self.c = trainer.circuit
        self._bound: dict[int, dict] = {}
        self._own_state = None  # the store's state after this object's last in-place update (fused optimizer)
        g = build_job_graph(trainer.plan, c.layers, c._children, c._out_pairs, c._complex, trainer._PARAM_OPS)
        self.why, self.graph = (g, None) if isinstance(g, str) else (None, g)
        self.sum_jobs, self.mix_jobs = ([], []) if self.graph is None else (self.graph.sum_jobs, self.graph.mix_jobs)

    def _uncovered(self) -> list[int]:
        """Input layers whose parameters no job epilogue updates (their gradients go to the flat buffer; the fused step runs
        the optimizer on their tensors' ranges and re-evaluates their parameter graphs at its start)."""
        return [i for i in self.graph.inputs if i not in self.graph.gauss and i not in self.graph.cat]

    def opt_counters(self) -> tuple[int, int]:
        """(steps taken, steps dropped) of the trainer's device clock, which the job epilogues advance (a device read)."""
        return self.tr.opt_counters()

    # ---- binding ----------------------------------------------------------------------------------------------------------
    def _drop(self, B: int) -> None:  # (the recorded programs of a binding hold its pointers)
        for pr in self._bound.pop(B)["prog"].values():
            pr.close()

    def bind(self, B: int) -> dict:
        c = self.c
        bd = c._bind(B)
        st = self._bound.get(B)
        if st is not None and st["serial"] == bd.serial and st["store_version"] == c.store.version:
            return st
        if st is not None:  # (a rebuilt circuit binding: the recorded lists point at its old staging copies and [sum, count] pair)
            self._drop(B)
        with torch.cuda.device(c.device):
            c._enqueue_params(torch.cuda.current_stream(c.device).cuda_stream)  # (allocates every derived-parameter buffer the tables point at)
            torch.cuda.synchronize(c.device)
        t = _Tables(self, bd, B)
        launches = t.launches()
        root = t.root(self.tr._opt_state())  # (last: its lists close the pool)
        st = {"serial": bd.serial, "store_version": c.store.version, "keep": t.keep, "launches": launches, "root": root,
              "pool": t.pool_d, "seed": t.seed, "seed_value": None, "extra": t.extra, "x0": t.x0, "prog": {}, "dT": {}}
        while len(self._bound) >= 4:
            self._drop(next(iter(self._bound)))
        self._bound[B] = st
        return st

    # ---- the launch list ----------------------------------------------------------------------------------------------------
    def _program(self, st: dict, B: int, mode: int):
        prog = st["prog"].get(mode)
        if prog is None:
            bd = self.c._bind(B)
            prog = st["prog"][mode] = capi.Program.record(lambda: self._enqueue(bd, st, B, mode, 0))
        return prog

    def _issue(self, la: Launch, bd, st: dict, B: int, mode: int, stream: int) -> None:
        """One launch of a binding: the one place that knows each kind's entry point and arguments (mode 2: the optimizer
        state goes to the backward launches' epilogues)."""
        if la.kind == "root":
            return capi.call("ck_jobs_root", C.byref(st["root"][mode]), stream)
        pool, blk = st["pool"].data_ptr(), B * K
        opt = self.tr._opt_state().ptr if mode == 2 else None
        entry, args = {
            "nsum": ("ck_jobs_nsum", (pool, blk)), "input_bwd": ("ck_jobs_nsum", (pool, blk)),
            "sum_fwd": ("ck_jobs_sum64_fwd", (pool,)), "sum_bwd": ("ck_jobs_sum64_bwd", (pool, opt, la.param)),
            "mix_fwd": ("ck_jobs_mix_fwd", (pool, la.param)), "mix_bwd": ("ck_jobs_mix_bwd", (pool, la.param, blk, opt)),
            "mix_params": ("ck_jobs_mix_params", (opt,)), "gauss_bwd": ("ck_jobs_gauss_bwd", (pool, B, opt)),
            "cat_bwd": ("ck_jobs_cat_bwd", (pool, B, la.param, opt)),
        }[la.kind]
        capi.call(entry, la.table(mode), la.n, *args, stream)
        if la.kind == "input_bwd":  # (its gathered gradient block goes through the layer-wise trainer's launches)
            self._input_backward(la.layer, bd, st, B, stream)

    def _enqueue(self, bd, st: dict, B: int, mode: int, stream: int) -> None:
        """mode 1: parameters, forward, backward with d theta into the trainer's flat gradient (the optimizer launch and the
        collective follow outside).  mode 2 (one rank): the optimizer runs in the job epilogues -- `ck_opt_tick` first, the
        parameter graphs of the layers no epilogue covers re-evaluated, and the optimizer on their tensors at the end."""
        tr, c = self.tr, self.c
        opt = tr._opt_state().ptr if mode == 2 else None
        validate = c.validate_inputs and c._int_input
        if mode == 2:
            capi.call("ck_opt_tick", opt, c._bad_input.data_ptr() if validate else None, tr._bad_seen.data_ptr() if validate else None, stream)
            for i in self._uncovered():  # their parameter graphs, as every forward of the reference evaluates them
                idx = c._jobs_of_layer.get(i)
                if idx:
                    c._batch.subset(idx).launch(stream)
                else:
                    c.layers[i].prepare(stream, batched=False)
        else:
            c._enqueue_params(stream)  # every parameter graph, once per step (parameters/parameter.py:180-188)
        D = c.plan.num_variables
        for i in self.graph.inputs:
            if i in self.graph.gathered:
                continue  # (its consumers read the table)
            l = c.layers[i]
            l.launch_input(bd.xt if l.wants_float_input else bd.xt_i, D, bd.views[i], B, stream)
        for la in st["launches"]:
            self._issue(la, bd, st, B, mode, stream)
        if mode == 2:  # the tensors of the layers no epilogue covers: the optimizer on their ranges of the flat buffers
            for i in self._uncovered():
                for name in self._tensors_of(i):
                    t, g = c.store[name], tr.grads[name]
                    m1, m2 = tr._moments.get(name, (None, None))
                    capi.call("ck_opt_step_range", t.data_ptr(), g.data_ptr(), None, None if m1 is None else m1.data_ptr(),
                              None if m2 is None else m2.data_ptr(), t.numel(), opt, stream)

    def _tensors_of(self, i: int) -> list[str]:
        l = self.c.layers[i]
        names: list[str] = []
        for p in l.params.values():
            for n in p.graph.nodes:
                if n.op == "tensor" and n.config["tensor"] not in names:
                    names.append(n.config["tensor"])
        return names

    def _input_backward(self, i: int, bd, st: dict, B: int, stream: int) -> None:
        """The backward of input layer i over its gathered (F, B, 64) gradient -- the launches of the layer-wise trainer."""
        tr, c = self.tr, self.c
        l = c.layers[i]
        g = st["x0"] + self.graph.input_g[i].first * B * K * 4
        dev = c.device
        if isinstance(l, HipCategoricalLayer):
            dT = st["dT"].get(i)
            if dT is None:
                dT = st["dT"][i] = torch.zeros((l.num_folds, l.num_categories + 1, K), dtype=torch.float32, device=dev)
            capi.call("ck_categorical_bwd", g, None, bd.xt_i.data_ptr(), l._scope(dev).data_ptr(), dT.data_ptr(), l.num_folds, B, K,
                      l.num_categories, 0, None, stream)
            name = l.probs.graph.nodes[0].config["tensor"]
            capi.call("ck_param_log_table_bwd", l._table.data_ptr(), dT.data_ptr(), tr.grads[name].data_ptr(), l.num_folds, K,
                      l.num_categories, 0, stream)
        else:  # a Gaussian layer with parameter graphs the job epilogue does not know
            mean, stddev, _ = l._vals
            dm = st["dT"].get((i, "m"))
            if dm is None:
                dm = st["dT"][(i, "m")] = torch.zeros_like(mean)
                st["dT"][(i, "s")] = torch.zeros_like(stddev)
            ds = st["dT"][(i, "s")]
            capi.call("ck_gaussian_bwd", g, bd.xt.data_ptr(), l._scope(dev).data_ptr(), mean.data_ptr(), stddev.data_ptr(), dm.data_ptr(),
                      ds.data_ptr(), l.num_folds, B, K, stream)
            for name in self._tensors_of(i):  # (the parameter backward ADDS into the tensors' gradients)
                t = tr.grads[name]
                capi.call("ck_fill_f32", t.data_ptr(), t.numel(), 0.0, stream)
            l.mean.backward(dm, tr.grads, stream)
            l.stddev.backward(ds, tr.grads, stream)

    # ---- one step -------------------------------------------------------------------------------------------------------------
    def _launch(self, x: torch.Tensor, gB: float, mode: int) -> torch.Tensor:
        c = self.c
        B = int(x.shape[0])
        st = self.bind(B)
        bd = c._bind(B)
        with torch.cuda.device(c.device):
            stream = torch.cuda.current_stream(c.device).cuda_stream
            if mode == 2:
                self.tr._opt_state()
                if self._own_state != c.store.state():
                    # somebody else changed a parameter since this object last derived them: all graphs, once
                    c._enqueue_params(stream)
            prog = self._program(st, B, mode)
            if st["seed_value"] != -1.0 / gB:
                capi.call("ck_fill_f32", st["seed"].data_ptr(), B, -1.0 / gB, stream)
                st["seed_value"] = -1.0 / gB
            xf, xi = c._prepare_input(x)
            c._stage_input(bd, xf, xi, stream)
            prog.launch(stream)
            if mode == 2:
                c.store.touch()
                self._own_state = c.store.state()
        return bd.ll

    def loss_and_grads(self, x: torch.Tensor, gB: float) -> torch.Tensor:
        """Forward + backward of ``-(1 / gB) sum_b log p(x_b)`` over the recorded launch list; the parameter gradients land in
        the trainer's flat buffer; returns the circuit's [sum log p, rows] pair (device, overwritten by the next call at this
        batch size)."""
        return self._launch(x, gB, 1)

    def step(self, x: torch.Tensor, gB: float) -> torch.Tensor:
        """One optimisation step with the optimizer inside the job epilogues (a single rank: no gradient leaves the launch
        that computed it, so there is nothing a collective could reduce)."""
        return self._launch(x, gB, 2)

    def num_launches(self, B: int, mode: int = 2) -> int:
        st = self.bind(B)
        return self._program(st, B, mode).num_ops
