"""The reverse half of the parameter graphs, kernel by kernel and then graph by graph.

Part one calls every backward entry point `HipParameter.backward` and the trainers drive -- `ck_param_softmax_bwd`,
`ck_param_softmax_bwd_strided`, `ck_param_softmax_bwd_batch` (job lists, parted gradients, the optimizer epilogue behind
`ck_opt_tick`), `ck_param_log_table_bwd`, `ck_param_unary_bwd`, `ck_param_scaled_sigmoid_bwd`, `ck_param_mixing_weight_bwd`,
`ck_param_scatter_add_folds`, `ck_axpy_f32`, `ck_param_reduce_bwd`, `ck_param_outer_sum_bwd`, `ck_param_gaussian_product_ms_bwd`,
`ck_param_gaussian_product_logz_bwd` -- through the C ABI on raw buffers, against the fp64 run of
tests/param_backward_restatement.py, on both sides of every shape or value boundary of the kernels.  Part two runs
`HipParameter.evaluate` / `backward` over graphs against the oracle's `eval_param` in fp64 under torch autograd.

Memory.  Every output lives between guard words of a NaN bit pattern no kernel produces (`_Guarded`): the guards must be
untouched; with accumulate = 0 every owned word must be written; with accumulate = 1 the output is pre-filled with a random
prior and must come out as prior + gradient.  In part two every entry of `grads` carries a random prior.

Tolerance (the convention of tests/test_gpu_param_prologue.py).  The yardstick of a case is the error of the SAME restated
function (graphs: `eval_param` under autograd) run in fp32 by torch on the CPU against its fp64 run, on the case's own inputs,
the accumulate step included; the GPU must be within 4 x that, with a floor of 1e-6.  Errors are relative to max|row| of the
fp64 result (the line of the reduced axis; entrywise kernels: to |prior| + |gradient| of the entry itself, sums of a line: to the
sum of the |addends|); the log-table gradient is compared absolutely.  Nothing in a bar comes from what the GPU returns, no entry
is left out, and a non-finite reference entry must be matched exactly.  `ck_param_scatter_add_folds` and `ck_axpy_f32` have
derived bounds instead: m 2^-24 (|prior| + sum|addends|) for a destination receiving m addends in any order, and one fp32 ulp
of the fp64 a x + y.  Every case prints `PARAM-BWD <kernel> <case> err yard ratio` (ratio = err / max(yard, floor / 4): a case
passes iff ratio <= 4); the worst per kernel are in LAB_NOTES.md, "Parameter backward"."""
import numpy as np
import pytest
import torch

import param_backward_restatement as R
from guarded_buffers import NAN_BITS, NEG_INF, _Guarded, _logits, _stream
from prologue_restatement import log_table

pytestmark = pytest.mark.gpu

FLOOR = 1e-6
WORST: dict[str, tuple] = {}
CASES = [0]
ACC = [0, 1]


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    for kernel in sorted(WORST):
        r, case, err, yard = WORST[kernel]
        print(f"\nPARAM-BWD-WORST {kernel}: ratio {r:.3f} (err {err:.3e}, yardstick {yard:.3e}) at {case}")
    print(f"\nPARAM-BWD-CASES {CASES[0]}")


def _call(dev, name, *args):
    """The entry point on the current stream, then a synchronize.  A host tensor among `args` is copied to the device and kept
    alive until the launch has finished; its pointer is what the entry point receives."""
    from cirkit_amd import _capi as capi

    held = [a.contiguous().to(dev) if isinstance(a, torch.Tensor) else a for a in args]
    capi.call(name, *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in held], _stream(dev))
    torch.cuda.synchronize()


def _report(kernel, case, err, yard, bound=None):
    """One case: `err` against 4 x `yard` with the floor (or against the derived `bound`, which then plays the bar's part)."""
    err, yard = float(err), float(yard)
    ratio = err / max(yard, FLOOR / 4) if bound is None else 4 * err / bound
    print(f"PARAM-BWD {kernel} {case} err {err:.3e} yard {yard:.3e} ratio {ratio:.3f}")
    CASES[0] += 1
    if kernel not in WORST or ratio > WORST[kernel][0]:
        WORST[kernel] = (ratio, case, err, yard)
    if bound is None:
        assert err <= max(4 * yard, FLOOR), f"{kernel} {case}: error {err:.3e} above 4 x the fp32 yardstick {yard:.3e} (floor {FLOOR})"
    else:
        assert err <= bound, f"{kernel} {case}: error {err:.3e} above the derived bound {bound:.3e}"


def _row_scale(ref, dim=-1):
    """max|row| of the fp64 result along `dim` over its finite entries (1 where that is 0: the error is then absolute)."""
    a = torch.where(torch.isfinite(ref), ref.abs(), torch.zeros_like(ref)).amax(dim=dim, keepdim=True)
    return torch.where(a > 0, a, torch.ones_like(a))


def _check(kernel, case, got, ref, yard, scale):
    """got (fp32, from the GPU) against ref (fp64) with the fp32 yardstick run `yard`; `scale` (from fp64 values only, broadcast
    to ref; None: absolute).  Non-finite reference entries are matched exactly; every other entry is compared."""
    got, yard = got.double().reshape(ref.shape), yard.double().reshape(ref.shape)
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), f"{kernel} {case}: NaN where the reference has none (or the reverse)"
    inf = torch.isinf(ref)
    assert torch.equal(got[inf], ref[inf]), f"{kernel} {case}: an infinite reference entry is not matched"
    assert bool(torch.isfinite(got[fin]).all()), f"{kernel} {case}: non-finite where the reference is finite"
    assert bool(torch.isfinite(yard[fin]).all()), f"{kernel} {case}: the fp32 yardstick run is not finite where the fp64 run is"
    if not bool(fin.any()):
        return _report(kernel, case, 0.0, 0.0)
    s = torch.ones_like(ref) if scale is None else scale.expand_as(ref)
    s = torch.where(s > 0, s, torch.ones_like(s))
    err = ((got - ref).abs() / s)[fin].max()
    y = ((yard - ref).abs() / s)[fin].max()
    _report(kernel, case, err, y)


def _output(dev, shape, acc, g):
    """(guarded output, fp32 prior or None): pre-filled with a random prior when the kernel is to add."""
    o = _Guarded(int(np.prod(shape)), dev)
    prior = None
    if acc:
        prior = torch.randn(tuple(shape), generator=g)
        o.out.copy_(prior.reshape(-1))
    return o, prior


def _d(x):
    return None if x is None else x.double()


# ------------------------------------------------------------------------------------------------- ck_param_softmax_bwd
SM_LENS = [1, 2, 31, 32, 33, 63, 64, 65, 128, 257, 1000]


def _dw(shape, fam, g):
    dw = torch.randn(shape, generator=g)
    if fam == "spike":  # one entry of every row 1e6 times the others: the cancellation in dw - dot
        col = torch.randint(shape[-1], (shape[0], 1), generator=g)
        dw.scatter_(1, col, dw.gather(1, col) * 1e6)
    return dw


@pytest.mark.parametrize("ln", SM_LENS)
def test_softmax_bwd_rows(hip_device, ln):
    """One wave per row, four rows per workgroup, lanes striding the row: rows on both sides of a workgroup (4 / 5), one
    lane's worth and more (len 63 / 64 / 65), several passes (257, 1000)."""
    g = torch.Generator().manual_seed(100 + ln)
    for rows in ([1, 3, 4, 5, 257] if ln in (1, 32, 33, 65, 1000) else [1, 5]):
        for fam in ("normal", "spread", "neginf", "const"):
            w = torch.softmax(_logits((rows, ln), fam, g), -1)
            for dfam in ("normal", "spike"):
                dw = _dw((rows, ln), dfam, g)
                for acc in ACC:
                    o, prior = _output(hip_device, (rows, ln), acc, g)
                    _call(hip_device, "ck_param_softmax_bwd", w, dw, o.out.data_ptr(),
                          rows, ln, acc)
                    got = o.read().view(rows, ln)
                    ref = R.softmax_bwd_rows(w.double(), dw.double(), _d(prior))
                    dead = w == 0
                    want0 = prior[dead] if acc else torch.zeros(int(dead.sum()))
                    assert torch.equal(got[dead], want0), "an entry with w == 0 does not have gradient exactly 0"
                    _check("softmax_bwd", f"len={ln} rows={rows} {fam} dw={dfam} acc={acc}", got, ref, R.softmax_bwd_rows(w, dw, prior),
                           _row_scale(ref))


# ---------------------------------------------------------------------------------------- ck_param_softmax_bwd_strided
@pytest.mark.parametrize("log_space", [0, 1])
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 5, 1), (2, 7, 3), (1, 33, 65), (5, 2, 300), (300, 3, 1)])
def test_softmax_bwd_strided(hip_device, shape, log_space):
    """A thread per (outer, inner) pair walking the axis: inner = 1 and not, more than one workgroup of lines (5 x 300, 300)."""
    outer, ln, inner = shape
    g = torch.Generator().manual_seed(outer * 1000 + ln * 10 + log_space)
    for fam in ("normal", "neginf"):
        x = _logits((outer, inner, ln), fam, g).transpose(1, 2).contiguous()  # (outer, len, inner), the axis in the middle
        y = torch.log_softmax(x, 1) if log_space else torch.softmax(x, 1)
        dy = torch.randn(shape, generator=g)
        for acc in ACC:
            o, prior = _output(hip_device, shape, acc, g)
            _call(hip_device, "ck_param_softmax_bwd_strided", y, dy, o.out.data_ptr(),
                  outer, ln, inner, log_space, acc)
            got = o.read().view(shape)
            ref = R.softmax_bwd_strided(y.double(), dy.double(), log_space, _d(prior))
            if not acc:
                dead = torch.isinf(x)
                assert torch.equal(got[dead], dy[dead] if log_space else torch.zeros(int(dead.sum()))), "dx at a -inf logit"
            _check("log_softmax_bwd_strided" if log_space else "softmax_bwd_strided", f"{shape} {fam} acc={acc}", got, ref,
                   R.softmax_bwd_strided(y, dy, log_space, prior), _row_scale(ref, 1))


# ------------------------------------------------------------------------------------------ ck_param_softmax_bwd_batch
JOB_DTYPE = np.dtype([("w", "<u8"), ("dw", "<u8"), ("dtheta", "<u8"), ("rows", "<i8"), ("len", "<i4"), ("first", "<i4"),
                      ("part_stride", "<i8"), ("n_part", "<i4"), ("reserved", "<i4"),
                      ("theta", "<u8"), ("m1", "<u8"), ("m2", "<u8"), ("w_out", "<u8")])  # ck_softmax_bwd_job of include/cirkit_hip.h


class _BwdJob:
    """One job of `ck_param_softmax_bwd_batch` with its own inputs and a guarded `dtheta`; n_part > 1: `dw` is n_part slots
    `stride` floats apart, the gaps between the slots filled with the NaN pattern."""

    def __init__(self, dev, rows, ln, g, n_part=0, fam="normal", theta=None):
        self.rows, self.len, self.n_part = rows, ln, n_part
        self.theta0 = _logits((rows, ln), fam, g) if theta is None else theta
        self.w = torch.softmax(self.theta0, -1)
        self.w_d = self.w.to(dev)
        self.dev = dev
        self.stride = rows * ln + 96 if n_part > 1 else 0
        self.dtheta = _Guarded(rows * ln, dev)
        self.theta = self.m1 = self.m2 = self.w_out = None
        self.new_dw(g)

    def new_dw(self, g, row_scale=None):
        rows, ln = self.rows, self.len
        n = max(self.n_part, 1)
        self.slots = torch.randn(n, rows, ln, generator=g)
        if row_scale is not None:
            self.slots = self.slots * row_scale.view(1, rows, 1)
        if self.n_part > 1:
            buf = torch.full((n * self.stride,), NAN_BITS, dtype=torch.int32).view(torch.float32).clone()
            for p in range(n):
                buf[p * self.stride:p * self.stride + rows * ln] = self.slots[p].reshape(-1)
            self.dw_d = buf.to(self.dev)
        else:
            self.dw_d = self.slots[0].contiguous().to(self.dev)
        self.dtheta.bits.fill_(NAN_BITS)

    def with_opt(self, adam, alias_w):
        """The optimizer epilogue on this job: logits, moments (Adam) and the next softmax -- into `w` itself, as the trainer
        does, or into an output of its own."""
        n = self.rows * self.len
        self.theta = _Guarded(n, self.dev)
        self.theta.out.copy_(self.theta0.reshape(-1))
        if adam:
            self.m1, self.m2 = _Guarded(n, self.dev), _Guarded(n, self.dev)
            self.m1.out.zero_()
            self.m2.out.zero_()
        self.w_out = None if alias_w else _Guarded(n, self.dev)
        self.alias_w = alias_w
        return self

    def dW(self, dtype):
        """The gradient the kernel differentiates: the sum of the slots in `dtype`."""
        return self.slots.to(dtype).sum(0)

    def check_dtheta(self, case, w=None):
        w = self.w if w is None else w
        got = self.dtheta.read().view(self.rows, self.len)
        ref = R.softmax_bwd_rows(w.double(), self.dW(torch.float64))
        _check("softmax_bwd_batch", case, got, ref, R.softmax_bwd_rows(w, self.dW(torch.float32)), _row_scale(ref))
        return got


def _launch_jobs(dev, jobs, opt_ptr=None):
    """first_block as the trainer computes it (cirkit_amd/training.py), n_blocks the exact total."""
    jt = np.zeros(len(jobs), dtype=JOB_DTYPE)
    assert jt.dtype.itemsize == 88
    first = 0
    for r, j in zip(jt, jobs):
        r["w"], r["dw"], r["dtheta"], r["rows"], r["len"], r["first"] = j.w_d.data_ptr(), j.dw_d.data_ptr(), j.dtheta.out.data_ptr(), j.rows, j.len, first
        r["part_stride"], r["n_part"] = j.stride, j.n_part
        if j.theta is not None:
            r["theta"] = j.theta.out.data_ptr()
            r["m1"] = 0 if j.m1 is None else j.m1.out.data_ptr()
            r["m2"] = 0 if j.m2 is None else j.m2.out.data_ptr()
            r["w_out"] = j.w_d.data_ptr() if j.alias_w else j.w_out.out.data_ptr()
        first += (j.rows + 3) // 4
    table = torch.from_numpy(jt.view(np.uint8).reshape(len(jobs), -1)).to(dev)
    _call(dev, "ck_param_softmax_bwd_batch", table.data_ptr(), len(jobs), first, opt_ptr)


@pytest.mark.parametrize("n_jobs", [1, 3, 17])
def test_softmax_bwd_batch_job_lists(hip_device, n_jobs):
    """Mixed row lengths (the len == 32 form, the generic loop below and above a wave) and row counts (less than, exactly and
    more than the four rows of a workgroup) in one launch: every job finds its own blocks."""
    g = torch.Generator().manual_seed(n_jobs)
    lens, rows = [5, 32, 33, 64, 100], [1, 4, 5, 130]
    jobs = [_BwdJob(hip_device, rows[(3 * i + i // 4) % 4], lens[i % 5], g, fam=("normal", "spread", "neginf")[i % 3]) for i in range(n_jobs)]
    _launch_jobs(hip_device, jobs)
    for i, j in enumerate(jobs):
        j.check_dtheta(f"jobs={n_jobs} #{i} len={j.len} rows={j.rows}")


@pytest.mark.parametrize("n_part", [2, 3, 15, 16, 17, 18, 31, 32, 33])
def test_softmax_bwd_batch_parted(hip_device, n_part):
    """len == 32 with the gradient spread over n_part slots: the 16-slot unrolled loop of the two half-waves (entered from
    n_part = 16 for the lower and 17 for the upper half-wave, twice from 32 / 33) and its tail; only the slots are read."""
    g = torch.Generator().manual_seed(n_part)
    jobs = [_BwdJob(hip_device, rows, 32, g, n_part=n_part) for rows in (1, 5, 130)] + [_BwdJob(hip_device, 5, 33, g)]
    _launch_jobs(hip_device, jobs)
    for j in jobs:
        j.check_dtheta(f"n_part={j.n_part} len={j.len} rows={j.rows}")


def _opt_fields(state):
    from cirkit_amd import _capi as capi

    raw = bytes(state.bytes.cpu().numpy().tobytes())
    return capi.OptState.from_buffer_copy(raw)


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_softmax_bwd_batch_optimizer_epilogue(hip_device, kind):
    """Three consecutive ticks of `ck_opt_tick` + the launch with the optimizer in its epilogue, on len == 32 jobs with and
    without parts, beside jobs without `theta`.  Stage one: dtheta against fp64.  Stage two: the fp64 optimizer restatement fed
    the logits and moments read back BEFORE the launch and the dtheta the launch WROTE: theta' - theta relative to lr, the
    moments relative to their maximum, w_out against the softmax of the theta' the launch wrote.  Row gradients of exactly 0,
    of order 1e-20 (g g underflows) and of order 1e3 are among the inputs.  A fourth tick with the bad-input flag raised must
    change nothing but dtheta."""
    from cirkit_amd.train_state import DeviceOptState

    dev, adam = hip_device, kind == "adam"
    g = torch.Generator().manual_seed(5 + adam)
    lr, betas, eps = 0.01, (0.9, 0.999), 1e-8
    state = DeviceOptState(dev).sync(lr, betas, eps, kind)
    rows = 6
    scale = torch.tensor([0.0, 1e-20, 1e3, 1.0, 1.0, 30.0])
    plain = _BwdJob(dev, rows, 32, g).with_opt(adam, alias_w=True)
    parted = _BwdJob(dev, rows, 32, g, n_part=3).with_opt(adam, alias_w=False)
    bystander, other = _BwdJob(dev, 5, 32, g), _BwdJob(dev, 3, 33, g)
    jobs = [plain, bystander, parted, other]
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    sticky = torch.zeros(1, dtype=torch.int32, device=dev)
    b32 = (float(np.float32(betas[0])), float(np.float32(betas[1])))  # (the device state holds the betas of the update in fp32)

    def snapshot(j):
        z = torch.zeros(rows, 32)
        return (j.theta.read().view(rows, 32).clone(), j.m1.read().view(rows, 32).clone() if adam else z,
                j.m2.read().view(rows, 32).clone() if adam else z)

    for tick in (1, 2, 3):
        for j in jobs:
            j.new_dw(g, scale if j.rows == rows else None)
        before = {id(j): snapshot(j) for j in (plain, parted)}
        w_before = plain.w_d.cpu().clone()
        _call(dev, "ck_opt_tick", state.ptr, flag.data_ptr(), sticky.data_ptr())
        _launch_jobs(dev, jobs, state.ptr)
        assert state.counters() == (tick, 0)
        bystander.check_dtheta(f"{kind} tick={tick} job without theta")
        other.check_dtheta(f"{kind} tick={tick} len=33 job")
        assert torch.equal(bystander.w_d.cpu(), bystander.w) and torch.equal(other.w_d.cpu(), other.w), "a job without theta was written to"
        for name, j in (("plain", plain), ("parted", parted)):
            case = f"{kind} tick={tick} {name}"
            dth = j.check_dtheta(case + " dtheta", w=w_before if j is plain else None)  # stage one
            th0, m10, m20 = before[id(j)]
            th1, m11, m21 = snapshot(j)
            ref = R.opt_step(kind, th0.double(), dth.double(), m10.double(), m20.double(), tick, lr, b32, eps)
            yard = R.opt_step(kind, th0, dth, m10, m20, tick, lr, b32, eps)
            step_scale = torch.full((1,), lr, dtype=torch.float64)
            _check("opt_epilogue", case + " (theta' - theta) / lr", (th1.double() - th0.double()), ref[0] - th0.double(),
                   yard[0].double() - th0.double(), step_scale)
            if adam:
                _check("opt_epilogue", case + " m1'", m11, ref[1], yard[1], _row_scale(ref[1].reshape(1, -1)).reshape(1, 1))
                _check("opt_epilogue", case + " m2'", m21, ref[2], yard[2], _row_scale(ref[2].reshape(1, -1)).reshape(1, 1))
                assert bool((m11[0] == 0).all()) and bool((m21[0] == 0).all()) and torch.equal(th1[0], th0[0]), "a zero gradient moved its row"
            w_new = (j.w_d.cpu() if j.alias_w else j.w_out.read()).view(rows, 32)
            wref = R.updated_row_softmax(th1.double())
            _check("opt_epilogue", case + " w_out", w_new, wref, R.updated_row_softmax(th1), _row_scale(wref))
    # a dropped step: the flag is raised, the tick latches it, the launch changes nothing but dtheta
    for j in jobs:
        j.new_dw(g, scale if j.rows == rows else None)
    bits = lambda t: t.view(torch.int32).clone()  # noqa: E731
    held = [bits(b.raw()) for j in (plain, parted) for b in (j.theta, j.m1, j.m2) if b is not None]
    held_w = [bits(plain.w_d.cpu()), bits(parted.w_out.raw())]
    w_before = plain.w_d.cpu().clone()
    flag.fill_(1)
    _call(dev, "ck_opt_tick", state.ptr, flag.data_ptr(), sticky.data_ptr())
    assert _opt_fields(state).skip_now == 1 and int(flag.item()) == 0 and int(sticky.item()) == 1
    _launch_jobs(dev, jobs, state.ptr)
    assert state.counters() == (3, 1), "a dropped step advanced the clock"
    now = [bits(b.raw()) for j in (plain, parted) for b in (j.theta, j.m1, j.m2) if b is not None]
    assert all(torch.equal(a, b) for a, b in zip(held, now)), "a dropped step changed the logits or the moments"
    assert torch.equal(held_w[0], bits(plain.w_d.cpu())) and torch.equal(held_w[1], bits(parted.w_out.raw())), "a dropped step wrote w_out"
    plain.check_dtheta(f"{kind} dropped step plain dtheta", w=w_before)
    parted.check_dtheta(f"{kind} dropped step parted dtheta")


# ---------------------------------------------------------------------------------------------- ck_param_log_table_bwd
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 3, 7), (2, 5, 11), (2, 32, 2), (2, 48, 9), (1, 96, 4), (1, 256, 3), (1, 300, 2),
                                   (2, 32, 256), (1, 64, 300)])
def test_log_table_bwd(hip_device, shape):
    """(F, K, C): K dividing the 256 threads and not (48, 96: threads past cstep K idle), K = 256 (one row group), K > 256 (the
    serial column sums), dynamic LDS below 48 KB, between (2, 32, 256: 66 KB) and near the 160 KB limit (1, 64, 300: 153 KB).
    Row C of dtable is NaN: a finite result proves it is ignored.  The column sums are LDS float atomics: nothing bit-exact."""
    Fo, K, C = shape
    g = torch.Generator().manual_seed(K * 1000 + C)
    for fam in ("normal", "neginf"):
        table = log_table(_logits((Fo, K, C), fam, g))  # (F, C + 1, K), row C = 0
        dT = torch.randn(Fo, C + 1, K, generator=g)
        dT[:, C] = float("nan")
        for acc in ACC:
            o, prior = _output(hip_device, (Fo, K, C), acc, g)
            _call(hip_device, "ck_param_log_table_bwd", table, dT, o.out.data_ptr(), Fo, K, C, acc)
            got = o.read().view(Fo, K, C)
            assert bool(torch.isfinite(got).all()), "row C of dtable was read"
            if not acc:
                dead = torch.isinf(table[:, :C]).transpose(1, 2)
                assert torch.equal(got[dead], dT[:, :C].transpose(1, 2)[dead]), "dtheta != dT at a category without mass"
            ref = R.log_table_bwd(table.double(), dT.double(), _d(prior))
            _check("log_table_bwd", f"{shape} {fam} acc={acc}", got, ref, R.log_table_bwd(table, dT, prior), None)


def test_log_table_bwd_refuses_what_does_not_fit(hip_device):
    """(1, 64, 320): 2 C (K + 1) + K words = 163 KB of LDS -> CK_ERR_UNSUPPORTED with its message, nothing written."""
    Fo, K, C = 1, 64, 320
    table, dT = torch.zeros(Fo * (C + 1) * K, device=hip_device), torch.zeros(Fo * (C + 1) * K, device=hip_device)
    o = _Guarded(Fo * K * C, hip_device)
    with pytest.raises(NotImplementedError, match="does not fit in LDS"):
        _call(hip_device, "ck_param_log_table_bwd", table.data_ptr(), dT.data_ptr(), o.out.data_ptr(), Fo, K, C, 0)
    torch.cuda.synchronize()
    assert bool((o.raw() == NAN_BITS).all()), "a refused launch wrote something"


# ------------------------------------------------------------------------------------- ck_param_unary_bwd / scaled sigmoid
UNARY_N = [1, 255, 256, 257, 2048 * 256 + 257]
CLAMP = (-0.5, 0.25)


def _unary_inputs(op, n, g):
    """x, y = op(x) in fp32, dy with exact zeros; from n >= 255 on the op's edge values sit in the first entries."""
    from cirkit_amd import _capi as capi

    x = torch.randn(n, generator=g) * (10 if op == "softplus" else 3)
    if op == "log":
        x = x.abs() + 0.1
    dy = torch.randn(n, generator=g)
    dy[torch.rand(n, generator=g) < 0.1] = 0.0
    if n >= 255:
        if op == "log":  # x == 0 with dy == 0 (exactly 0) and with dy != 0 (the signed infinity)
            x[:3], dy[:3] = 0.0, torch.tensor([0.0, 2.0, -3.0])
        elif op == "clamp":  # exactly on both bounds, and the neighbouring floats outside
            lo, hi = torch.tensor(CLAMP[0]), torch.tensor(CLAMP[1])
            x[:4] = torch.stack([lo, hi, torch.nextafter(lo, torch.tensor(-1.0)), torch.nextafter(hi, torch.tensor(1.0))])
            dy[:4] = torch.tensor([1.5, -2.5, 1.5, -2.5])
        elif op == "softplus":
            x[:4], dy[:4] = torch.tensor([19.5, 20.0, 20.5, -30.0]), 1.25
        elif op == "sigmoid":  # saturated: y == 1
            x[0], dy[0] = 40.0, 3.0
        elif op == "exp":  # y near FLT_MAX
            x[0], dy[0] = 88.7, 0.5
    y = {"sigmoid": torch.sigmoid, "exp": torch.exp, "log": torch.log, "square": torch.square, "softplus": torch.nn.functional.softplus,
         "clamp": lambda t: torch.clamp(t, CLAMP[0], CLAMP[1])}[op](x)
    code = {"sigmoid": capi.CK_UNARY_SIGMOID, "exp": capi.CK_UNARY_EXP, "log": capi.CK_UNARY_LOG, "square": capi.CK_UNARY_SQUARE,
            "clamp": capi.CK_UNARY_CLAMP, "softplus": capi.CK_UNARY_SOFTPLUS}[op]
    return code, x, y, dy


def _entry_scale(ref_grad, prior):
    """|prior| + |gradient| of every entry, in fp64: what an fp32 prior + gradient is rounded against."""
    s = torch.where(torch.isfinite(ref_grad), ref_grad.abs(), torch.zeros_like(ref_grad))
    return s if prior is None else s + prior.double().abs()


@pytest.mark.parametrize("n", UNARY_N)
@pytest.mark.parametrize("op", R.UNARY_OPS)
def test_unary_bwd(hip_device, op, n):
    """n on both sides of a workgroup and past the 2048 x 256 entries of the capped grid (the grid-stride loop)."""
    g = torch.Generator().manual_seed(n % 1000 + len(op))
    code, x, y, dy = _unary_inputs(op, n, g)
    kw = {"vmin": CLAMP[0], "vmax": CLAMP[1]} if op == "clamp" else {}
    xd, yd, dyd = x.to(hip_device), y.to(hip_device), dy.to(hip_device)
    for acc in ACC:
        o, prior = _output(hip_device, (n,), acc, g)
        _call(hip_device, "ck_param_unary_bwd", code, xd.data_ptr(), yd.data_ptr(), dyd.data_ptr(), o.out.data_ptr(), n, acc)
        got = o.read()
        grad = R.unary_bwd(op, x.double(), y.double(), dy.double(), **kw)
        ref = R.unary_bwd(op, x.double(), y.double(), dy.double(), _d(prior), **kw)
        if not acc:
            assert bool((got[dy == 0] == 0).all()), "dy == 0 does not give exactly 0"
            if n >= 255 and op == "log":
                assert got[:3].tolist() == [0.0, float("inf"), NEG_INF]
            if n >= 255 and op == "clamp":
                assert got[:4].tolist() == [1.5, -2.5, 0.0, 0.0]
            if n >= 255 and op == "sigmoid":
                assert float(y[0]) == 1.0 and float(got[0]) == 0.0
            if n >= 255 and op == "softplus":
                assert float(got[2]) == 1.25  # (above the threshold: the derivative is 1)
        _check(f"unary_bwd:{op}", f"n={n} acc={acc}", got, ref, R.unary_bwd(op, x, y, dy, prior, **kw), _entry_scale(grad, prior))


def test_unary_bwd_refuses_unknown_ops(hip_device):
    from cirkit_amd import _capi as capi

    x = torch.ones(8, device=hip_device)
    o = _Guarded(8, hip_device)
    for code in (capi.CK_UNARY_SCALED_SIGMOID, 7, -1):
        with pytest.raises(ValueError, match="ck_param_unary_bwd"):
            _call(hip_device, "ck_param_unary_bwd", code, x.data_ptr(), x.data_ptr(), x.data_ptr(), o.out.data_ptr(), 8, 0)
    assert bool((o.raw() == NAN_BITS).all())


@pytest.mark.parametrize("bounds", [(0.0, 1.0), (1e-4, 10.0), (-2.0, -0.5)])
def test_scaled_sigmoid_bwd(hip_device, bounds):
    vmin, vmax = (float(np.float32(b)) for b in bounds)  # (what the entry point receives: floats)
    g = torch.Generator().manual_seed(int(vmax * 10) + 50)
    for n in (1, 257, 2048 * 256 + 1):
        y = (torch.tensor(vmin) + (torch.tensor(vmax) - torch.tensor(vmin)) * torch.rand(n, generator=g)).clamp(vmin, vmax)
        dy = torch.randn(n, generator=g)
        if n > 1:
            y[0], y[1] = vmin, vmax
        yd, dyd = y.to(hip_device), dy.to(hip_device)
        for acc in ACC:
            o, prior = _output(hip_device, (n,), acc, g)
            _call(hip_device, "ck_param_scaled_sigmoid_bwd", yd.data_ptr(), dyd.data_ptr(), o.out.data_ptr(), n, vmin, vmax, acc)
            got = o.read()
            if n > 1 and not acc:
                assert got[:2].tolist() == [0.0, 0.0], "y on a bound does not give exactly 0"
            grad = R.scaled_sigmoid_bwd(y.double(), dy.double(), vmin, vmax)
            ref = R.scaled_sigmoid_bwd(y.double(), dy.double(), vmin, vmax, _d(prior))
            _check("scaled_sigmoid_bwd", f"[{vmin:g}, {vmax:g}] n={n} acc={acc}", got, ref, R.scaled_sigmoid_bwd(y, dy, vmin, vmax, prior),
                   _entry_scale(grad, prior))
    o = _Guarded(4, hip_device)
    for lo, hi in ((1.0, 1.0), (2.0, 1.0)):
        with pytest.raises(ValueError, match="vmax must exceed vmin"):
            _call(hip_device, "ck_param_scaled_sigmoid_bwd", yd.data_ptr(), dyd.data_ptr(), o.out.data_ptr(), 1, lo, hi, 0)
    assert bool((o.raw() == NAN_BITS).all())


# ------------------------------------------------------------------------------------------ ck_param_mixing_weight_bwd
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 5, 2), (2, 32, 4), (2, 64, 3), (1, 7, 9)])
def test_mixing_weight_bwd(hip_device, shape):
    """Every entry of dy off the block diagonal is NaN: dx is finite, and with accumulate = 0 the picks bit for bit."""
    Fo, K, H = shape
    g = torch.Generator().manual_seed(K * 10 + H)
    picks = torch.randn(Fo, K, H, generator=g)
    dy = torch.full((Fo, K, H, K), float("nan"))
    for k in range(K):
        dy[:, k, :, k] = picks[:, k]
    dy = dy.reshape(Fo, K, H * K)
    for acc in ACC:
        o, prior = _output(hip_device, shape, acc, g)
        _call(hip_device, "ck_param_mixing_weight_bwd", dy, o.out.data_ptr(), Fo, K, H, acc)
        got = o.read().view(shape)
        assert bool(torch.isfinite(got).all()), "an entry off the block diagonal was read"
        if not acc:
            assert torch.equal(got, picks)
        ref = R.mixing_weight_bwd(dy.double(), K, H, _d(prior))
        _check("mixing_weight_bwd", f"{shape} acc={acc}", got, ref, R.mixing_weight_bwd(dy, K, H, prior), _entry_scale(picks.double(), prior))


# --------------------------------------------------------------------------------- ck_param_scatter_add_folds / ck_axpy_f32
def _scatter_cases(per_fold):
    cases = [("permutation", 7, [4, 2, 6, 0, 5, 1, 3]), ("subset", 7, [5, 1, 3]), ("one destination n=2", 3, [1, 1]),
             ("mixed duplicates", 5, [3, 0, 3, 3, 1, 0, 4, 3, 1])]
    if per_fold <= 256:
        cases.append(("one destination n=64", 3, [2] * 64))
    if per_fold <= 255:
        cases.append(("one destination n=1000", 2, [0] * 1000))
    return cases


@pytest.mark.parametrize("per_fold", [1, 255, 256, 64 * 256 + 1])
def test_scatter_add_folds(hip_device, per_fold):
    """Float atomics with duplicate destinations; per_fold past the 64 x 256 entries of grid.x (the stride loop).  Bound: a
    destination receiving m addends, added in any order in fp32, is within m 2^-24 (|prior| + sum|addends|) of the exact sum."""
    g = torch.Generator().manual_seed(per_fold)
    for name, Fd, idx in _scatter_cases(per_fold):
        n = len(idx)
        src, prior = torch.randn(n, per_fold, generator=g), torch.randn(Fd, per_fold, generator=g)
        o = _Guarded(Fd * per_fold, hip_device)
        o.out.copy_(prior.reshape(-1))
        idx_t = torch.tensor(idx, dtype=torch.int64)
        _call(hip_device, "ck_param_scatter_add_folds", src, idx_t, o.out.data_ptr(), n, per_fold)
        got = o.read().view(Fd, per_fold)
        ref = R.scatter_add_folds(src.double(), idx_t, prior.double())
        yard = R.scatter_add_folds(src, idx_t, prior)
        m = torch.bincount(idx_t, minlength=Fd).double().view(Fd, 1)
        mass = R.scatter_add_folds(src.double().abs(), idx_t, prior.double().abs())
        unhit = (m == 0).view(-1)
        assert torch.equal(got[unhit].view(torch.int32), prior[unhit].view(torch.int32)), "a destination nobody adds to changed"
        bound = m * 2.0 ** -24 * mass
        assert bool(((got.double() - ref).abs() <= bound).all()), f"{name}: above m 2^-24 (|prior| + sum|addends|)"
        hit = ~unhit
        err = ((got.double() - ref).abs()[hit] / bound[hit]).max()  # (in units of the bound: at most 1)
        _report("scatter_add_folds", f"per_fold={per_fold} {name}", err, ((yard.double() - ref).abs()[hit] / bound[hit]).max(), bound=1.0)


def test_scatter_add_folds_refuses_more_rows_than_grid_y(hip_device):
    o = _Guarded(16, hip_device)
    src, idx = torch.zeros(16, device=hip_device), torch.zeros(16, dtype=torch.int64, device=hip_device)
    with pytest.raises(ValueError, match="n exceeds grid.y"):
        _call(hip_device, "ck_param_scatter_add_folds", src.data_ptr(), idx.data_ptr(), o.out.data_ptr(), 65536, 1)
    torch.cuda.synchronize()
    assert bool((o.raw() == NAN_BITS).all()), "a refused launch wrote something"


@pytest.mark.parametrize("a", [1.0, -0.5, 3e-8])
def test_axpy(hip_device, a):
    """Every entry within one fp32 ulp of the fp64 a x + y (a as the float the entry point receives)."""
    a = float(np.float32(a))
    g = torch.Generator().manual_seed(int(a * 100) % 97)
    for n in (1, 257, 2048 * 256 + 1):
        x, y = torch.randn(n, generator=g), torch.randn(n, generator=g)
        o = _Guarded(n, hip_device)
        o.out.copy_(y)
        _call(hip_device, "ck_axpy_f32", o.out.data_ptr(), x, a, n)
        got = o.read()
        ref = R.axpy(y.double(), x.double(), a)
        r32 = ref.float().abs()
        ulp = (torch.nextafter(r32, torch.full_like(r32, float("inf"))) - r32).double()
        assert bool(((got.double() - ref).abs() <= ulp).all()), "more than one ulp from the fp64 a x + y"
        err = ((got.double() - ref).abs() / ulp).max()  # (in ulps: at most 1)
        _report("axpy_f32", f"a={a:g} n={n}", err, ((R.axpy(y, x, a).double() - ref).abs() / ulp).max(), bound=1.0)


# ------------------------------------------------------------------------ ck_param_reduce_bwd / ck_param_outer_sum_bwd
REDUCE_SHAPES = [(1, 1, 1), (3, 6, 1), (2, 33, 3), (300, 2, 1), (1, 4, 300)]


@pytest.mark.parametrize("op", ["prod", "lse"])
@pytest.mark.parametrize("shape", REDUCE_SHAPES)
def test_reduce_bwd(hip_device, shape, op):
    """Lines by number modulo 4: plain; one zero (prod) / some -inf (lse); two zeros / all -inf; dy == 0."""
    outer, ln, inner = shape
    g = torch.Generator().manual_seed(outer + 7 * ln + (op == "lse"))
    x = torch.randn(shape, generator=g)
    dy = torch.randn(outer, inner, generator=g)
    line = (torch.arange(outer).view(-1, 1) * inner + torch.arange(inner).view(1, -1)) % 4  # (outer, inner)
    if outer * inner == 1:
        line[:] = 1  # (the only line carries the special value)
    if op == "prod":
        x = x.sign() * (x.abs() * 0.5 + 0.5)
        x[x == 0] = 1.0
    for o_ in range(outer):
        for r in range(inner):
            kind, at = int(line[o_, r]), int(torch.randint(ln, (1,), generator=g))
            if op == "prod" and kind in (1, 2):
                x[o_, at, r] = 0.0
                if kind == 2:
                    x[o_, (at + 1) % ln, r] = 0.0
            elif op == "lse" and kind == 1:  # (one entry of the line stays finite)
                x[o_, [j for j in range(ln) if j != at and j % 2 == 0], r] = NEG_INF
            elif op == "lse" and kind == 2:
                x[o_, :, r] = NEG_INF
    y = torch.prod(x, 1) if op == "prod" else torch.logsumexp(x, 1)
    dy[line == 3] = 0.0
    x = x.contiguous()
    o = _Guarded(outer * ln * inner, hip_device)
    _call(hip_device, "ck_param_reduce_bwd", 0 if op == "prod" else 1, x, y,
          dy, o.out.data_ptr(), outer, ln, inner)
    got = o.read().view(shape)
    ref = R.reduce_bwd(op, x.double(), y.double(), dy.double())
    assert bool(torch.isfinite(ref).all())
    quiet = ((line == 3) | ((line == 2) & (op == "lse"))).unsqueeze(1).expand(shape)
    assert bool((got[quiet] == 0).all()), "a dy == 0 line (or an all -inf line) does not have gradient exactly 0"
    _check(f"reduce_bwd:{op}", f"{shape}", got, ref, R.reduce_bwd(op, x, y, dy), _row_scale(ref, 1))


@pytest.mark.parametrize("shape", REDUCE_SHAPES)
def test_outer_sum_bwd(hip_device, shape):
    """Both operands, n1 != n2 (n1 = len of the shape list, 1 included)."""
    outer, n1, inner = shape
    n2 = 4 if n1 == 5 else 5
    g = torch.Generator().manual_seed(outer * 31 + n1)
    dout = torch.randn(outer, n1 * n2, inner, generator=g)
    for which, keep in ((0, n1), (1, n2)):
        o = _Guarded(outer * keep * inner, hip_device)
        _call(hip_device, "ck_param_outer_sum_bwd", dout, o.out.data_ptr(), outer, n1, n2, inner, which)
        got = o.read().view(outer, keep, inner)
        ref = R.outer_sum_bwd(dout.double(), n1, n2, which)
        _check("outer_sum_bwd", f"{shape} n2={n2} which={which}", got, ref, R.outer_sum_bwd(dout, n1, n2, which),
               R.outer_sum_bwd(dout.double().abs(), n1, n2, which))


# ------------------------------------------------------------------------------------------------- Gaussian products
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 4, 3), (2, 1, 33), (2, 64, 5), (300, 2, 2)])
def test_gaussian_product_bwd(hip_device, shape):
    """Standard deviations of 0.05, 1 and 20 mixed within a fold, means up to +-50; both ops of the mean / stddev kernel and the
    log-partition one.  A thread per (fold, unit) of either operand: 300 folds cross a workgroup."""
    Fo, K1, K2 = shape
    g = torch.Generator().manual_seed(Fo * 100 + K1 * 10 + K2)
    sds = torch.tensor([0.05, 1.0, 20.0])
    m1, m2 = torch.rand(Fo, K1, generator=g) * 100 - 50, torch.rand(Fo, K2, generator=g) * 100 - 50
    s1, s2 = sds[torch.randint(3, (Fo, K1), generator=g)], sds[torch.randint(3, (Fo, K2), generator=g)]
    dout = torch.randn(Fo, K1 * K2, generator=g)
    dev = [t.to(hip_device) for t in (m1, s1, m2, s2, dout)]
    p = [t.data_ptr() for t in dev]
    dbl = [t.double() for t in (m1, s1, m2, s2, dout)]

    def outs():
        return [_Guarded(Fo * K1, hip_device), _Guarded(Fo * K1, hip_device), _Guarded(Fo * K2, hip_device), _Guarded(Fo * K2, hip_device)]

    names = ("dm1", "ds1", "dm2", "ds2")
    o = outs()
    _call(hip_device, "ck_param_gaussian_product_ms_bwd", 0, p[0], p[1], p[2], p[3], p[4], *[b.out.data_ptr() for b in o], Fo, K1, K2)
    for nm, b, ref, yard in zip(names, o, R.gaussian_product_mean_bwd(*dbl), R.gaussian_product_mean_bwd(m1, s1, m2, s2, dout)):
        _check("gaussian_product_ms_bwd:mean", f"{shape} {nm}", b.read().view(ref.shape), ref, yard, _row_scale(ref))
    o = outs()
    _call(hip_device, "ck_param_gaussian_product_ms_bwd", 1, None, p[1], None, p[3], p[4], None, o[1].out.data_ptr(), None, o[3].out.data_ptr(),
          Fo, K1, K2)
    assert bool((o[0].raw() == NAN_BITS).all()) and bool((o[2].raw() == NAN_BITS).all())
    for nm, b, ref, yard in zip(("ds1", "ds2"), (o[1], o[3]), R.gaussian_product_stddev_bwd(dbl[1], dbl[3], dbl[4]),
                                R.gaussian_product_stddev_bwd(s1, s2, dout)):
        _check("gaussian_product_ms_bwd:stddev", f"{shape} {nm}", b.read().view(ref.shape), ref, yard, _row_scale(ref))
    o = outs()
    _call(hip_device, "ck_param_gaussian_product_logz_bwd", p[0], p[1], p[2], p[3], p[4], *[b.out.data_ptr() for b in o], Fo, K1, K2)
    for nm, b, ref, yard in zip(names, o, R.gaussian_product_logz_bwd(*dbl), R.gaussian_product_logz_bwd(m1, s1, m2, s2, dout)):
        _check("gaussian_product_logz_bwd", f"{shape} {nm}", b.read().view(ref.shape), ref, yard, _row_scale(ref))


# =============================================================================================== HipParameter.backward
F3 = 3


def _T(name, folds, shape):
    from cirkit_amd.plan import ParamNode

    return ParamNode("tensor", folds, tuple(shape), {"tensor": name}, [])


def _N(op, folds, shape, inputs, **config):
    """A node over `inputs`: producer ids (identity index) or (ids, fold array) pairs."""
    from cirkit_amd.plan import IDX_ARRAY, IDX_NONE, FoldIndex, ParamNode

    fis = []
    for i in inputs:
        if isinstance(i, int):
            fis.append(FoldIndex([i], IDX_NONE))
        else:
            fis.append(FoldIndex(list(i[0]), IDX_ARRAY, np.asarray(i[1], dtype=np.int64)))
    return ParamNode(op, folds, tuple(shape), dict(config), fis)


def _values(nodes, g, positive=(), extra=(), stored=None):
    """Random fp32 values of every stored tensor the nodes name (`positive`: kept above 0.3; `stored`: the fold count of a tensor
    whose pointer re-indexes it), plus `extra` (name, folds, shape) tensors nobody reads."""
    vals = {}
    for n in nodes:
        if n.op in ("tensor", "pointer") and n.config["tensor"] not in vals:
            name = n.config["tensor"]
            folds = (stored or {}).get(name, n.num_folds)
            v = torch.randn((folds, *n.shape), generator=g)
            vals[name] = v.abs() + 0.3 if name in positive else v
    for name, folds, shape in extra:
        vals[name] = torch.randn((folds, *shape), generator=g)
    return vals


def _autograd(graph, vals, dout, priors, dtype):
    """(value, {name: prior + gradient}) of the oracle's `eval_param` in `dtype` under torch autograd."""
    from oracle.torch_oracle import eval_param

    leaves = {k: v.to(dtype).requires_grad_(True) for k, v in vals.items()}
    torch.set_default_dtype(dtype)
    try:
        want = eval_param(graph, leaves)
        want.backward(dout.to(dtype))
    finally:
        torch.set_default_dtype(torch.float32)
    return want.detach(), {k: priors[k].to(dtype) + (torch.zeros_like(l) if l.grad is None else l.grad) for k, l in leaves.items()}, \
        {k for k, l in leaves.items() if l.grad is None}


def _run_graph(dev, case, nodes, output=None, *, positive=(), extra=(), upto=None, rounds=1, seed=0, calls=None, stored=None):
    """evaluate + backward of the graph on the GPU, `rounds` times on the same HipParameter with fresh stored values, every entry
    of `grads` pre-filled with a random prior (and guarded), against autograd through `eval_param`."""
    from cirkit_amd.parameters import HipParameter, TensorStore
    from cirkit_amd.plan import IDX_NONE, FoldIndex, ParamGraph

    g = torch.Generator().manual_seed(1000 + seed)
    out_fi = FoldIndex([len(nodes) - 1], IDX_NONE) if output is None else output
    out_folds = nodes[-1].num_folds if output is None else len(np.asarray(output.array).reshape(-1))
    graph = ParamGraph(nodes, out_fi, out_folds, nodes[-1].shape)
    ref_graph = graph if upto is None else ParamGraph(nodes[:upto + 1], FoldIndex([upto], IDX_NONE), nodes[upto].num_folds, nodes[upto].shape)
    store = TensorStore(dev)
    p = None
    stream = _stream(dev)
    for rnd in range(rounds):
        vals = _values(nodes, g, positive, extra, stored)
        store.update(vals)
        if p is None:
            p = HipParameter(graph, store)
        y = p.evaluate(stream, upto=upto)
        priors = {k: torch.randn(v.shape, generator=g) for k, v in vals.items()}
        bufs = {k: _Guarded(v.numel(), dev) for k, v in vals.items()}
        for k, b in bufs.items():
            b.out.copy_(priors[k].reshape(-1))
        grads = {k: b.out.view(vals[k].shape) for k, b in bufs.items()}
        dout = torch.randn(tuple(y.shape), generator=g)
        if calls is not None:
            calls.clear()
        p.backward(dout.to(dev), grads, stream, upto=upto)
        torch.cuda.synchronize()
        want, ref, unread = _autograd(ref_graph, vals, dout, priors, torch.float64)
        _, yard, _ = _autograd(ref_graph, vals, dout, priors, torch.float32)
        assert tuple(y.shape) == tuple(want.shape)
        assert float((y.cpu().double() - want).abs().max()) <= 1e-5 * (float(want.abs().max()) + 1.0), f"{case}: forward"
        for k in vals:
            got = bufs[k].read().view(vals[k].shape)
            if k in unread:
                assert torch.equal(got.view(torch.int32), priors[k].view(torch.int32)), f"{case}: the gradient of {k}, which the graph does not read, changed"
                continue
            _check("graph", f"{case} round={rnd} {k}", got, ref[k], yard[k], _row_scale(ref[k]))
    return p


UNARY_GRAPHS = {
    "softmax last axis": lambda: [_T("t0", F3, (4, 5)), _N("softmax", F3, (4, 5), [0], dim=1)],
    "softmax middle axis": lambda: [_T("t0", F3, (2, 4, 3)), _N("softmax", F3, (2, 4, 3), [0], dim=1)],
    "log_softmax": lambda: [_T("t0", F3, (4, 5)), _N("log_softmax", F3, (4, 5), [0], dim=1)],
    "log_softmax first axis": lambda: [_T("t0", F3, (4, 5)), _N("log_softmax", F3, (4, 5), [0], dim=0)],
    "sigmoid": lambda: [_T("t0", F3, (5, 7)), _N("sigmoid", F3, (5, 7), [0])],
    "exp": lambda: [_T("t0", F3, (5, 7)), _N("exp", F3, (5, 7), [0])],
    "log": lambda: [_T("t0", F3, (5, 7)), _N("log", F3, (5, 7), [0])],
    "square": lambda: [_T("t0", F3, (5, 7)), _N("square", F3, (5, 7), [0])],
    "scaled_sigmoid": lambda: [_T("t0", F3, (5, 7)), _N("scaled_sigmoid", F3, (5, 7), [0], vmin=0.25, vmax=4.0)],
    "mixing_weight": lambda: [_T("t0", F3, (5, 2)), _N("mixing_weight", F3, (5, 10), [0])],
    "matmul": lambda: [_T("t0", F3, (4, 6)), _T("t1", F3, (6, 5)), _N("matmul", F3, (4, 5), [0, 1])],
    "pointer": lambda: [_N("pointer", F3, (5, 7), [], tensor="t0")],
    "conj": lambda: [_T("t0", F3, (5, 7)), _N("conj", F3, (5, 7), [0])],
    "flatten": lambda: [_T("t0", F3, (2, 3, 4)), _N("flatten", F3, (6, 4), [0], start_dim=0, end_dim=1)],
    "gaussian_product_log_partition": lambda: [_T("t0", F3, (4,)), _T("t1", F3, (4,)), _T("t2", F3, (3,)), _T("t3", F3, (3,)),
                                               _N("gaussian_product_log_partition", F3, (12,), [0, 1, 2, 3])],
}


@pytest.mark.parametrize("name", list(UNARY_GRAPHS))
def test_graph_one_op(hip_device, name):
    """Every op without a direct test, one per graph at F = 3; a stored tensor the graph does not read keeps its bits."""
    _run_graph(hip_device, name, UNARY_GRAPHS[name](), positive=("t0",) if name == "log" else ("t1", "t3") if name.startswith("gaussian") else (),
               extra=[("unread", 2, (3,))], seed=len(name))


REINDEX_GRAPHS = {
    "permutation": lambda: ([_T("t0", 4, (3, 4)), _N("sigmoid", 4, (3, 4), [([0], [2, 0, 3, 1])])], None),
    "repeated folds": lambda: ([_T("t0", 4, (3, 4)), _N("sigmoid", 6, (3, 4), [([0], [0, 0, 2, 1, 2, 3])])], None),
    "strict subset": lambda: ([_T("t0", 4, (3, 4)), _N("sigmoid", 2, (3, 4), [([0], [3, 1])])], None),
    "two producers interleaved": lambda: ([_T("t0", 2, (3, 4)), _T("t1", 3, (3, 4)), _N("exp", 5, (3, 4), [([0, 1], [3, 0, 4, 1, 2])])], None),
    "two producers, softmax": lambda: ([_T("t0", 2, (3, 4)), _T("t1", 3, (3, 4)), _N("softmax", 6, (3, 4), [([0, 1], [3, 0, 4, 0, 1, 3])], dim=1)], None),
    "pointer with duplicates": lambda: ([_N("pointer", 5, (3, 4), [], tensor="t0", fold_idx=[1, 1, 0, 2, 1]),
                                         _N("square", 5, (3, 4), [0])], None),
    "output index": lambda: ([_T("t0", 3, (3, 4)), _N("exp", 3, (3, 4), [0])], ([1], [2, 2, 0])),
    "matmul operands re-indexed": lambda: ([_T("t0", 2, (4, 6)), _T("t1", 3, (6, 5)), _N("matmul", 4, (4, 5), [([0], [1, 0, 1, 1]), ([1], [2, 0, 0, 1])])], None),
}


@pytest.mark.parametrize("name", list(REINDEX_GRAPHS))
def test_graph_fold_reindexing(hip_device, name):
    """Operands read through an index array -- a permutation, repeats, a strict subset, rows of two producers interleaved (the
    non-contiguous gather of `scatter`), a pointer's own fold_idx, the graph's output index -- against autograd's index_add."""
    from cirkit_amd.plan import IDX_ARRAY, FoldIndex

    nodes, out = REINDEX_GRAPHS[name]()
    output = None if out is None else FoldIndex(list(out[0]), IDX_ARRAY, np.asarray(out[1], dtype=np.int64))
    _run_graph(hip_device, name, nodes, output, seed=len(name), rounds=2 if "interleaved" in name else 1,
               stored={"t0": 4} if name.startswith("pointer") else None)


FANOUT_GRAPHS = {
    "read twice": lambda: ([_T("t0", F3, (5, 7)), _N("exp", F3, (5, 7), [0]), _N("square", F3, (5, 7), [1]), _N("sigmoid", F3, (5, 7), [1]),
                            _N("sum", F3, (5, 7), [2, 3])], None),
    "read once": lambda: ([_T("t0", F3, (5, 7)), _N("exp", F3, (5, 7), [0]), _N("square", F3, (5, 7), [1])], None),
    "sum(a, b), a once and b twice": lambda: ([_T("t0", F3, (5, 7)), _N("exp", F3, (5, 7), [0]), _T("t1", F3, (5, 7)), _N("sigmoid", F3, (5, 7), [2]),
                                               _N("sum", F3, (5, 7), [1, 3]), _N("sum", F3, (5, 7), [4, 3])], None),
    "tensor read twice": lambda: ([_T("t0", F3, (5, 7)), _N("exp", F3, (5, 7), [0]), _N("sum", F3, (5, 7), [0, 1])], None),
    "conj flatten softmax matmul": lambda: ([_T("t0", F3, (2, 3, 4)), _N("conj", F3, (2, 3, 4), [0]), _N("flatten", F3, (6, 4), [1], start_dim=0, end_dim=1),
                                             _N("softmax", F3, (6, 4), [2], dim=1), _T("t1", F3, (4, 5)), _N("matmul", F3, (6, 5), [3, 4])], None),
    "upto an interior node": lambda: ([_T("t0", F3, (5, 7)), _N("exp", F3, (5, 7), [0]), _N("square", F3, (5, 7), [1]), _N("sigmoid", F3, (5, 7), [2])], 2),
}


@pytest.mark.parametrize("name", list(FANOUT_GRAPHS))
def test_graph_fan_out_and_aliasing(hip_device, name):
    """Which gradient buffer a node gets: its reader's (read once), a zeroed scratch that is added to (read twice), the caller's."""
    nodes, upto = FANOUT_GRAPHS[name]()
    _run_graph(hip_device, name, nodes, upto=upto, seed=len(name), rounds=2)


def _count_calls(monkeypatch):
    """Every `capi.call` of the parameter module, (name, args), through the real entry point."""
    from cirkit_amd import _capi as capi

    seen, real = [], capi.call

    def counted(name, *args):
        seen.append((name, args))
        return real(name, *args)

    monkeypatch.setattr(capi, "call", counted)
    return seen


def _bmm(seen):
    """(trans_a, trans_b, accumulate) of every ck_param_bmm call."""
    return [tuple(a[7:10]) for n, a in seen if n == "ck_param_bmm"]


def test_graph_einsum_routes(hip_device, monkeypatch):
    """The einsum backward's four routes, the one taken read off the launches: a per-fold matrix product whose operands are
    stored tensors (ck_param_bmm adding straight into `grads`: no axpy), the same through exp nodes (written, then handed
    down), the Gram pattern y = x x^T at M = N = 32 (one launch, trans_a = 2) and at M = 24 (the general path, two launches)."""
    seen = _count_calls(monkeypatch)
    mm = ((0, 1), (1, 2), (0, 2))
    _run_graph(hip_device, "einsum sink", [_T("t0", F3, (4, 6)), _T("t1", F3, (6, 5)), _N("einsum", F3, (4, 5), [0, 1], einsum=mm)], seed=1, calls=seen,
               rounds=2)
    assert [c[2] for c in _bmm(seen)] == [1, 1] and not [n for n, _ in seen if n in ("ck_axpy_f32", "ck_param_einsum")]
    _run_graph(hip_device, "einsum no sink", [_T("t0", F3, (4, 6)), _N("exp", F3, (4, 6), [0]), _T("t1", F3, (6, 5)), _N("exp", F3, (6, 5), [2]),
                                            _N("einsum", F3, (4, 5), [1, 3], einsum=mm)], seed=2, calls=seen)
    assert [c[2] for c in _bmm(seen)] == [0, 0] and not [n for n, _ in seen if n == "ck_param_einsum"]
    gram = ((0, 1), (2, 1), (0, 2))
    _run_graph(hip_device, "gram M=32", [_T("t0", F3, (32, 32)), _N("einsum", F3, (32, 32), [0, 0], einsum=gram)], seed=3, calls=seen, rounds=2)
    assert len(_bmm(seen)) == 1 and _bmm(seen)[0][0] == 2 and _bmm(seen)[0][2] == 1, _bmm(seen)
    _run_graph(hip_device, "gram M=24", [_T("t0", F3, (24, 32)), _N("einsum", F3, (24, 24), [0, 0], einsum=gram)], seed=4, calls=seen)
    assert len(_bmm(seen)) == 2 and all(c[0] != 2 and c[2] == 1 for c in _bmm(seen)), _bmm(seen)
    _run_graph(hip_device, "einsum generic", [_T("t0", F3, (3, 4)), _T("t1", F3, (2, 5)), _N("einsum", F3, (3, 2, 4, 5), [0, 1], einsum=((0, 1), (2, 3), (0, 2, 1, 3)))],
               seed=5, calls=seen)
    assert len([n for n, _ in seen if n == "ck_param_einsum"]) == 2 and not _bmm(seen)


def test_graph_complex_backward_is_refused(hip_device):
    """Complex-valued parameter backward is not implemented: a complex pointer and a complex einsum say so."""
    from cirkit_amd.parameters import HipParameter, TensorStore
    from cirkit_amd.plan import IDX_NONE, FoldIndex, ParamGraph

    g = torch.Generator().manual_seed(2)
    store = TensorStore(hip_device)
    z = torch.complex(torch.randn(F3, 4, 4, generator=g), torch.randn(F3, 4, 4, generator=g))
    store.set("t0", z)
    store.set("t1", z)
    stream = _stream(hip_device)
    for nodes, text in (([_N("pointer", F3, (4, 4), [], tensor="t0")], "complex pointer"),
                        ([_T("t0", F3, (4, 4)), _T("t1", F3, (4, 4)), _N("einsum", F3, (4, 4), [0, 1], einsum=((0, 1), (1, 2), (0, 2)))], "complex operands")):
        p = HipParameter(ParamGraph(nodes, FoldIndex([len(nodes) - 1], IDX_NONE), F3, (4, 4)), store)
        y = p.evaluate(stream)
        grads = {k: torch.zeros_like(store[k]) for k in ("t0", "t1")}
        with pytest.raises(NotImplementedError, match=text):
            p.backward(torch.ones_like(y), grads, stream)
    torch.cuda.synchronize()
