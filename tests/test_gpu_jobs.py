"""The job-form training step (cirkit_amd/csrc/ck_jobs.hip), kernel by kernel: `ck_jobs_sum64_fwd` / `_bwd`, `ck_jobs_mix_fwd` /
`_bwd`, `ck_jobs_mix_params`, `ck_jobs_nsum`, `ck_jobs_root`, `ck_jobs_cat_bwd`, `ck_jobs_gauss_bwd`, `ck_opt_step_range` and
`ck_opt_tick` through the C ABI on raw buffers against the fp64 run of tests/jobs_restatement.py (pinned to torch autograd by
tests/test_jobs_restatement.py), on both sides of every boundary of the launches and of the kernels.

The shapes are read off the kernels at this commit (line numbers of ck_jobs.hip; nothing asserts which kernel ran):
* `ck_jobs_sum64_fwd` (1260-1263): always 4 waves (1262); wave w of a unit takes the 32-row tiles at row0 + 32 w + 128 i (134,
  141); the rows of a ragged tile beyond row1 re-read row1 - 1 and store nothing (137, 144, 150); `xrow` selects the table row
  (74-78: negative -> C, >= C -> C - 1).
* `ck_jobs_sum64_bwd` (1265-1278): 4 or 8 waves (1267, 1270-1274), tiles as above with stride 32 waves (190, 207); the waves'
  accumulators meet in waves / 2 LDS buffers (171, 306-327); n_split > 1 goes through `part` and the ticket, the last arrival adds
  the slots in slot order (336-357), n_split == 1 stays in LDS (358-365); waves threads own a weight row in the epilogue (290-292,
  368-386); modes 0 / 1 / 2 (397, 404, 409); under a mixing fold (194, 217-230) with `mix_dw` (391-396).
* `ck_jobs_mix_fwd` (1280-1284): 16 rows per pass (495), four slots in flight (502-518).  `ck_jobs_mix_bwd` (1291-1301): the
  template 2 | 4 | 8 | 16 is the smallest that holds h_max (1296-1299) and sizes the `part` slots (613); 16 rows per pass (547); the
  split as above (612-628); modes (631, 637, 641).
* `ck_jobs_mix_params` (667-704, 1286-1289): one thread per unit, H <= 16 logits in registers (685).
* `ck_jobs_nsum` (1303-1307): min(ceil(elems / 1024), 64) workgroups per job (1305), each thread a float4 per 1024 gridDim.x words
  (712); four blocks of the list in flight, added in list order (716-725).
* `ck_jobs_root` (1309-1318): R <= 16, S <= 4, n_wg <= 64 (1311-1314); a wave per row, rows 4 blockIdx + wave + 4 n_wg i (767): a
  workgroup beyond ceil(B / 4) has no row and writes zeros to its slot; the last arrival adds the slots eight at a time in workgroup
  order (849-859); wave w differentiates the softmax of rows w, w + 4, ... (881), wave 0 that of the coefficients (901), both
  with the dot product in double (738-745).
* `ck_jobs_cat_bwd` (1320-1334): rows are sorted 512 at a time (932, 954); per = ceil((C + 1) / 16) categories per wave (938) steps
  at C = 15 | 16, 31 | 32, 255 | 256; a wave loads eight rows and four blocks of the list at a time (1005, 1015); C a power of two
  divides by shifts (949); 4096 entries per pass of the table walk and of the optimizer's (1065, 1087); the launch is refused above
  160 KB of LDS (1323-1324: (C + 1) 65 + 1152 words + 2 (16 per) + 1025 ints, from C = 578).
* `ck_jobs_gauss_bwd` (1336-1339): 16 row groups of 16 threads (1154-1159).
* `ck_opt_step_range` (1341-1345): min(ceil(n / 256), 2048) workgroups (1343) and the stride loop (1226).

Memory.  Every pointer a job may write is a `_Guarded` buffer between guard words of a NaN bit pattern no kernel produces; the
guards, every row outside [row0, row1) of `out` / `gx`, row C of `table_out`, the columns of `mix_dw` other than mix_h and every
buffer a mode does not write must keep the pattern.  A gathered Categorical table sits directly in front of guard words: a read
past row C would turn the output into NaN.  Every `ticket` word must be 0 again after a launch.

Mode 2 (the optimizer in the epilogue) writes no gradient, so every case follows the two-stage scheme of
`test_softmax_bwd_batch_optimizer_epilogue` with the launch issued twice: in mode 1 (stage one: dtheta against fp64) and, after
`ck_opt_tick`, in mode 2 on the same inputs (stage two: the fp64 optimizer restatement fed the logits and moments read back BEFORE
the launch and the dtheta the mode-1 launch WROTE -- the launches are deterministic, which the bit-identity cases establish:
theta' - theta relative to lr, the moments relative to their maximum -- `jobs_restatement.opt_step`, the optimizer restatement on
the device state's clock: moments with the fp32 betas the state holds, bias corrections 1 - b^t of its double betas --, the next
step's values against their restatement applied to the theta' the launch wrote).  Three ticks, row gradients of exactly 0, of order 1e-20 and of order 1e3 among the inputs
(the root has one gradient per row and batch: its rows are not scaled), then a tick with the flag raised: nothing may change.

Tolerance (the convention of tests/test_gpu_param_backward.py and tests/test_gpu_layer_backward.py).  The yardstick of a case is the
error of the SAME restated function run in fp32 by torch on the CPU against its fp64 run on the case's own inputs; the GPU must
be within 4 x that, with a floor of 1e-6.  Errors are relative to max|row| of the fp64 result (the last axis).  Nothing in a bar
comes from what the GPU returns, no entry is left out, a non-finite reference entry must be matched exactly.  `ck_jobs_nsum`:
bit equality with the fp32 run.  `ll[0]`: within B 2^-53 sum|out| of the fp64 sum of the `out` the launch wrote.  bc1 / bc2:
one fp32 rounding of 1 - b^t in fp64.

Rounding allowance of the sum job's gx (measured first without: LAB_NOTES.md, "Job kernels": 2 of 474 cases of
`ck_jobs_sum64_bwd` stood at 5.0 and 9.4 x their yardstick, both gx over spread blocks; nothing else took one, and no summation-order
term was needed).  gx_n = e_n sum_o W[o, n] G_o / y_o sums terms of both signs, and max|row| of a row that cancellation leaves small
compares two single draws of amplified rounding noise.  As in tests/test_gpu_layer_backward.py an entry of gx may additionally be
off by the first-order bound of ANY fp32 evaluation with a one-ulp exponential and a one-ulp reciprocal, from the fp64 terms of
the case alone (u = 2^-24): e_n is within eps_n = 2 u (1 + |v_n - m|), relative (the rounded difference, its product with log2 e,
the exponential); y_o = sum_n W e_n, all terms >= 0, within (sum_n W e_n eps_n) / y_o + 64 u; the reciprocal 2 u, the product with
G u: gy_o within kappa_o = (sum_n W e_n eps_n) / y_o + 67 u; sum_o W[o, n] gy_o: 64 u of summation on the sum of the |terms|, the
product with e_n u and eps_n:
  allowance(gx_n) = e_n sum_o W[o, n] |gy_o| (kappa_o + 65 u) + eps_n e_n sum_o W[o, n] |gy_o|.
Summation order (`ck_jobs_mix_bwd` dtheta, `ck_jobs_cat_bwd`; measured first without: 1 case of each stood at 5.4 and 8.1 x).
d w[k, h] = sum_b G e_h / y (m = the job's rows) and dT[c, k] = the sum of the m = rows of category c are sums in an order the
launch fixes differently from torch (row groups, waves and `part` slots; the rows of a category in the order LDS atomics
sorted them, which also differs from launch to launch), and with H = 1 or with every row in one category max|row| IS such a
sum, small where it cancels: an entry may additionally be off by m 2^-24 sum|addends|, the bound of `ck_param_scatter_add_folds`,
the addends' sizes from the fp64 run on |G| -- through the softmax backward W (a - <W, a>) that is W (allowance + <W, allowance>),
through the log-softmax allowance(dT[c, k]) + p[k, c] (sum_c' allowance(dT[c', k]) + C 2^-24 sum_c' sum|addends|), the last term for the
sum over the C categories, which the kernel also adds in an order of its own.
The 4 x bar stands for everything else, and for these on top of their allowance.  A forward output is a logarithm: its error is
relative to max(max|row|, 1).  Every case prints
`JOBS-KERNEL <kernel> <case> err yard ratio` (ratio = err / max(yard, floor / 4): a case passes iff ratio <= 4); the worst per
kernel are in LAB_NOTES.md, "Job kernels"."""
import ctypes as C

import numpy as np
import pytest
import torch

import jobs_restatement as J
import param_backward_restatement as P
from guarded_buffers import NAN_BITS, NEG_INF, _Guarded, _logits, _stream
from prologue_restatement import log_table

pytestmark = pytest.mark.gpu

FLOOR = 1e-6
EPS = 2.0 ** -24
K = 64
WORST: dict[str, tuple] = {}
CASES = [0]
LR, BETAS, OPT_EPS = 0.01, (0.9, 0.999), 1e-8
B32 = (float(np.float32(BETAS[0])), float(np.float32(BETAS[1])))  # (the device state holds the betas of the update in fp32)
ROW_SCALE = [0.0, 1e-20, 1e3]  # of units 0, 1, 2 in the mode-2 cases


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    for kernel in sorted(WORST):
        r, case, err, yard = WORST[kernel]
        print(f"\nJOBS-KERNEL-WORST {kernel}: ratio {r:.3f} (err {err:.3e}, yardstick {yard:.3e}) at {case}")
    print(f"\nJOBS-KERNEL-CASES {CASES[0]}")


def _call(dev, name, *args):
    """The entry point on the current stream, then a synchronize."""
    from cirkit_amd import _capi as capi

    capi.call(name, *args, _stream(dev))
    torch.cuda.synchronize()


def _report(kernel, case, err, yard):
    err, yard = float(err), float(yard)
    ratio = err / max(yard, FLOOR / 4)
    print(f"JOBS-KERNEL {kernel} {case} err {err:.3e} yard {yard:.3e} ratio {ratio:.3f}")
    CASES[0] += 1
    if kernel not in WORST or ratio > WORST[kernel][0]:
        WORST[kernel] = (ratio, case, err, yard)
    assert err <= max(4 * yard, FLOOR), f"{kernel} {case}: error {err:.3e} above 4 x the fp32 yardstick {yard:.3e} (floor {FLOOR})"


def _row_scale(ref):
    """max|row| of the fp64 result along the last axis over its finite entries (1 where that is 0: the error is then absolute)."""
    a = torch.where(torch.isfinite(ref), ref.abs(), torch.zeros_like(ref)).amax(dim=-1, keepdim=True)
    return torch.where(a > 0, a, torch.ones_like(a))


def _check(kernel, case, got, ref, yard, extra=None, scale=None):
    """got (fp32, from the GPU) against ref (fp64) with the fp32 yardstick run `yard`, relative to max|row| of ref (or `scale`);
    `extra` (fp64, from the inputs alone): the derived allowance of an entry, taken off its error first.  Non-finite reference entries are matched exactly; every other entry is compared."""
    got, yard = got.double().reshape(ref.shape), yard.double().reshape(ref.shape)
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), f"{kernel} {case}: NaN where the reference has none (or the reverse)"
    if not bool(fin.all()):
        inf = torch.isinf(ref)
        assert torch.equal(got[inf], ref[inf]), f"{kernel} {case}: an infinite reference entry is not matched"
    assert bool((torch.isfinite(got) | ~fin).all()), f"{kernel} {case}: non-finite where the reference is finite"
    assert bool((torch.isfinite(yard) | ~fin).all()), f"{kernel} {case}: the fp32 yardstick run is not finite where the fp64 run is"
    s = _row_scale(ref) if scale is None else (scale.expand_as(ref) if isinstance(scale, torch.Tensor) else torch.full_like(ref, scale))
    d = (got - ref).abs()
    if extra is not None:
        d = (d - extra.reshape(ref.shape)).clamp_(min=0)
    zero = torch.zeros((), dtype=torch.float64)
    _report(kernel, case, torch.where(fin, d / s, zero).max(), torch.where(fin, (yard - ref).abs() / s, zero).max())


def _log_scale(ref):
    """The scale of a forward output: max|row|, and 1 where that is smaller -- `out` is a logarithm, its error is absolute (a
    marginalised row over normalised weights is log 1: relative to itself its rounding has no size)."""
    return _row_scale(ref).clamp(min=1.0)


def _order_allowance(addends_mass, m, W=None):
    """m 2^-24 sum|addends| of a sum of m addends whose order the launch fixes differently from torch; through a softmax backward
    W (a - <W, a>) that is W (allowance + <W, allowance>)."""
    a = m * EPS * addends_mass
    return a if W is None else W * (a + (W * a).sum(-1, keepdim=True))


def _d(x):
    if x is None:
        return None
    if isinstance(x, (list, tuple)):
        return [_d(v) for v in x]
    return x.double() if x.is_floating_point() else x


# ------------------------------------------------------------------------------------------------------- shared pieces
def _blocks(n, B, fam, g):
    """(n, B, 64) fp32 activations of a value family: randn * 2; 'shift': the same 4000 nats down; 'spread': uniform over +-100
    (e underflows); 'neginf': about 30 % of the units -inf; 'infrows': rows 0 and B // 2 -inf in every block."""
    if fam == "spread":
        return _logits((n, B, K), "spread", g)
    if fam == "neginf":
        return _logits((n, B, K), "neginf", g) * 2
    x = _logits((n, B, K), "normal", g) * 2
    if fam == "shift":
        x = x - 4000.0
    if fam == "infrows":
        x[:, 0] = NEG_INF
        x[:, B // 2] = NEG_INF
    return x


def _weights(shape, fam, g):
    """(W, theta): rows summing to 1 over the last axis, the softmax of logits of the family; 'wzero': the last column 0, row 0
    zero and 10 % of the entries exactly 0 (no logits: modes 0 and 1 only)."""
    if fam == "wzero":
        w = torch.softmax(torch.randn(shape, generator=g), -1)
        w[torch.rand(shape, generator=g) < 0.1] = 0.0
        if shape[-1] > 1:
            w[..., -1] = 0.0
        w[0, :] = 0.0
        return w.contiguous(), None
    theta = _logits(shape, fam if fam in ("spread", "neginf") else "normal", g)
    return torch.softmax(theta, -1).contiguous(), theta


def _gout(n, B, fam, g):
    """(n, B, 64) gradient blocks; 'gzero': 20 % exact zeros and row B // 3 zero in every block; 'infrows': row 0 zero."""
    go = torch.randn(n, B, K, generator=g)
    if fam == "gzero":
        go[torch.rand(n, B, K, generator=g) < 0.2] = 0.0
        go[:, B // 3] = 0.0
    if fam == "infrows":
        go[:, 0] = 0.0
    return go


def _split_fam(fam):
    """(block family, weight / logit family, gradient family) of a case family.  'wspread' / 'wneginf' are the spread and -inf
    LOGITS behind the weights, over normal blocks: with both spread, y underflows in any fp32 evaluation and there is no yardstick."""
    if fam in ("wspread", "wneginf"):
        return "normal", fam[1:], "normal"
    if fam == "wzero":
        return "normal", "wzero", "normal"
    if fam == "gzero":
        return "normal", "normal", "gzero"
    return fam, "normal", fam


class _Pool:
    """The DEVICE array of block pointers of a launch."""

    def __init__(self, dev):
        self.dev, self.ptrs, self.held = dev, [], []

    def add(self, blocks):
        """Host blocks (or raw device pointers) appended; returns the offset of the first."""
        off = len(self.ptrs)
        for b in blocks:
            if isinstance(b, torch.Tensor):
                b = b.contiguous().to(self.dev)
                self.held.append(b)
                b = b.data_ptr()
            self.ptrs.append(int(b))
        return off

    def tensor(self):
        t = torch.from_numpy(np.asarray(self.ptrs, dtype=np.uint64).view(np.int64).copy()).to(self.dev)
        self.held.append(t)
        return t


def _table(dev, rows, dtype):
    """A job table (numpy records) on the device."""
    from cirkit_amd import _capi as capi

    dt = np.dtype(getattr(capi, dtype))
    jt = np.zeros(len(rows), dtype=dt)
    for r, fields in zip(jt, rows):
        for k, v in fields.items():
            r[k] = v
    return torch.from_numpy(jt.view(np.uint8).reshape(len(rows), -1).copy()).to(dev)


def _fill(*bufs):
    for b in bufs:
        if b is not None:
            b.bits.fill_(NAN_BITS)


def _untouched(buf, what):
    assert buf is None or bool((buf.raw() == NAN_BITS).all()), f"{what} was written"


def _row_mask(B, row0, row1, width=K):
    m = torch.zeros(B, width, dtype=torch.bool)
    m[row0:row1] = True
    return m


def _cuts(row0, row1, n_split, last=None):
    """Unit boundaries of a job's rows: n_split pieces, the last one `last` rows long (None: even pieces)."""
    n = row1 - row0
    if n_split == 1:
        return [row0, row1]
    if last is None:
        return [row0 + (n * i) // n_split for i in range(n_split)] + [row1]
    head = n - last
    return [row0 + (head * i) // (n_split - 1) for i in range(n_split - 1)] + [row1 - last, row1]


class _Opt:
    """The logits (or any tensor an epilogue updates) with Adam's moments in guarded buffers."""

    def __init__(self, dev, theta0, adam):
        self.shape, n = tuple(theta0.shape), theta0.numel()
        self.theta = _Guarded(n, dev)
        self.theta.out.copy_(theta0.reshape(-1))
        self.m1 = self.m2 = None
        if adam:
            self.m1, self.m2 = _Guarded(n, dev), _Guarded(n, dev)
            self.m1.out.zero_()
            self.m2.out.zero_()

    def ptrs(self):
        return {"theta": self.theta.out.data_ptr(), "m1": 0 if self.m1 is None else self.m1.out.data_ptr(),
                "m2": 0 if self.m2 is None else self.m2.out.data_ptr()}

    def snap(self):
        z = torch.zeros(self.shape)
        return (self.theta.read().view(self.shape).clone(), z if self.m1 is None else self.m1.read().view(self.shape).clone(),
                z if self.m2 is None else self.m2.read().view(self.shape).clone())

    def bits(self):
        return [b.raw().clone() for b in (self.theta, self.m1, self.m2) if b is not None]


def _opt_fields(state):
    from cirkit_amd import _capi as capi

    return capi.OptState.from_buffer_copy(bytes(state.bytes.cpu().numpy().tobytes()))


def _two_stage(dev, kernel, case, kind, fresh, launch, pars, scaled=True, on_state=None):
    """The mode-2 scheme of the docstring.  fresh(tick): new gradient inputs; launch(mode, opt_ptr); pars: (name, _Opt, dtheta(case)
    -> the gradient the mode-1 launch wrote (checked against fp64 there), nxt() -> (the next step's values read back, their guarded
    buffers), ref_next(theta') -> their restatement, not_written: buffers a mode-2 launch must leave alone).  on_state: called
    with the DeviceOptState before the first tick."""
    from cirkit_amd.train_state import DeviceOptState

    adam = kind == "adam"
    state = DeviceOptState(dev).sync(LR, BETAS, OPT_EPS, kind)
    if on_state is not None:
        on_state(state)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    sticky = torch.zeros(1, dtype=torch.int32, device=dev)
    for tick in (1, 2, 3):
        fresh(tick)
        launch(1, 0)
        dth = [p[2](f"{case} {kind} tick={tick} {p[0]} dtheta") for p in pars]
        before = [p[1].snap() for p in pars]
        _call(dev, "ck_opt_tick", state.ptr, flag.data_ptr(), sticky.data_ptr())
        launch(2, state.ptr)
        assert state.counters() == (tick, 0)
        for (name, opt, _, nxt, ref_next, quiet), d, (th0, m10, m20) in zip(pars, dth, before):
            what = f"{case} {kind} tick={tick} {name}"
            for b in quiet():
                _untouched(b, what + ": a gradient buffer in mode 2")
            th1, m11, m21 = opt.snap()
            ref = J.opt_step(kind, th0.double(), d.double(), m10.double(), m20.double(), tick, LR, B32, BETAS, OPT_EPS)
            yard = J.opt_step(kind, th0, d, m10, m20, tick, LR, B32, BETAS, OPT_EPS)
            _check(kernel, what + " (theta' - theta) / lr", th1.double() - th0.double(), ref[0] - th0.double(),
                   yard[0].double() - th0.double(), scale=LR)
            if adam:
                _check(kernel, what + " m1'", m11, ref[1], yard[1], scale=float(ref[1].abs().max()) or 1.0)
                _check(kernel, what + " m2'", m21, ref[2], yard[2], scale=float(ref[2].abs().max()) or 1.0)
            if scaled:
                flat = lambda t: t.reshape(th0.shape[0], -1)[0]  # noqa: E731
                assert torch.equal(flat(th1), flat(th0)) and bool((flat(m11) == 0).all()) and bool((flat(m21) == 0).all()), \
                    "a zero gradient moved its row"
            got = nxt()[0]
            want = ref_next(th1.double())
            _check(kernel, what + " next values", got, want, ref_next(th1))
    # a dropped step: the flag is raised, the tick latches it, the launch changes nothing
    fresh(4)
    held = [b for p in pars for b in p[1].bits()] + [b.raw().clone() for p in pars for b in p[3]()[1]]
    flag.fill_(1)
    _call(dev, "ck_opt_tick", state.ptr, flag.data_ptr(), sticky.data_ptr())
    assert _opt_fields(state).skip_now == 1 and int(flag.item()) == 0 and int(sticky.item()) == 1
    launch(2, state.ptr)
    assert state.counters() == (3, 1), "a dropped step advanced the clock"
    now = [b for p in pars for b in p[1].bits()] + [b.raw().clone() for p in pars for b in p[3]()[1]]
    assert all(torch.equal(a, b) for a, b in zip(held, now)), f"{case}: a dropped step changed a parameter, a moment or the next values"
    for p in pars:
        for b in p[5]():
            _untouched(b, f"{case}: a gradient buffer in a dropped step")


def _scale_units(go):
    """Units 0, 1, 2 of every gradient block scaled by 0, 1e-20, 1e3: the rows of the parameter gradients they feed."""
    go[..., 0] *= ROW_SCALE[0]
    go[..., 1] *= ROW_SCALE[1]
    go[..., 2] *= ROW_SCALE[2]
    return go


# ------------------------------------------------------------------------------------------- ck_jobs_sum64_fwd / _bwd
class _SumJob:
    """One sum job over rows [row0, row1) of B-row blocks, cut into units at `cuts`, with guarded out / gx / dtheta / part (and
    mix_dw, the optimizer's tensors).  C > 0: the input is a Categorical fold's (C + 1, 64) table gathered by an int32 column
    that holds -1 and an out-of-range category.  mix = (H, h, n_partner, with_dw, zero_coefficient)."""

    def __init__(self, dev, g, B, row0=0, row1=None, n_in=1, n_g=1, n_split=1, last=None, fam="normal", C=0, mix=None):
        self.dev, self.B, self.row0, self.row1 = dev, B, row0, B if row1 is None else row1
        self.cuts = _cuts(self.row0, self.row1, n_split, last)
        self.n_split, self.fam, self.C = n_split, fam, C
        bfam, wfam, self.gfam = _split_fam(fam)
        self.W, self.theta0 = _weights((K, K), wfam, g)
        self.x = self.table = self.tab = None
        if C:
            self.table = log_table(_logits((1, K, C), "normal", g))[0].contiguous()
            self.x = torch.randint(0, C, (B,), generator=g).to(torch.int32)
            for i, v in enumerate((-1, C + 3, C - 1, C, 0, -7)[:B]):
                self.x[(i * 7) % B] = v
            self.tab = _Guarded((C + 1) * K, dev)  # (the table ends where the guard words begin)
            self.tab.out.copy_(self.table.reshape(-1))
            self.x_d = self.x.to(dev)
            self.blocks = None
        else:
            self.blocks = list(_blocks(n_in, B, bfam, g))
        self.n_g = n_g
        self.mix = mix
        self.new_grads(g)
        if mix is not None:
            H, h, n_partner, with_dw, zero = mix
            self.mix_w = torch.softmax(torch.randn(K, H, generator=g), -1)
            if zero:
                self.mix_w[5, h] = 0.0
            self.partners = list(torch.randn(n_partner, B, K, generator=g))
            others = [[torch.randn(B, K, generator=g)] for _ in range(H)]
            xh = J.sum_job_fwd(_d(self.blocks), self.W.double())
            for p in self.partners:
                xh = xh + p.double()
            slots = [[xh] if k == h else _d(others[k]) for k in range(H)]
            self.mix_out = J.mix_job_fwd(slots, self.mix_w.double()).float()  # its exact value, as the fp32 block the forward stored
            self.mix_out_d, self.mix_w_d = self.mix_out.to(dev), self.mix_w.contiguous().to(dev)
            self.mix_dw = _Guarded(K * H, dev) if with_dw else None
        self.w_d = self.W.to(dev)
        self.out, self.gx, self.dtheta = _Guarded(B * K, dev), _Guarded(B * K, dev), _Guarded(K * K, dev)
        self.part = _Guarded(n_split * K * K, dev) if n_split > 1 else None
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.opt = self.w_out = None

    def new_grads(self, g, scaled=False):
        go = _gout(self.n_g, self.B, self.gfam, g)
        self.glist = list(_scale_units(go) if scaled else go)

    def with_opt(self, adam):
        self.opt, self.w_out = _Opt(self.dev, self.theta0, adam), _Guarded(K * K, self.dev)
        return self

    def units(self, pool, mode):
        in_off = pool.add([self.tab.out.data_ptr()] if self.C else self.blocks)
        g_off = pool.add(self.glist)
        f = {"w": self.w_d.data_ptr(), "out": self.out.out.data_ptr(), "gx": self.gx.out.data_ptr(), "dtheta": self.dtheta.out.data_ptr(),
             "part": 0 if self.part is None else self.part.out.data_ptr(), "ticket": self.ticket.data_ptr(), "in_off": in_off,
             "n_in": 1 if self.C else len(self.blocks), "g_off": g_off, "n_g": self.n_g, "n_split": self.n_split, "mode": mode,
             "C": self.C, "xrow": self.x_d.data_ptr() if self.C else 0}
        if self.opt is not None:
            f.update(self.opt.ptrs())
            f["w_out"] = self.w_out.out.data_ptr()
        if self.mix is not None:
            H, h, n_partner, _, _ = self.mix
            f.update({"mix_out": self.mix_out_d.data_ptr(), "mix_w": self.mix_w_d.data_ptr(), "mix_dw": 0 if self.mix_dw is None else self.mix_dw.out.data_ptr(),
                      "partner_off": pool.add(self.partners), "n_partner": n_partner, "mix_h": h, "mix_H": H})
        return [dict(f, row0=a, row1=b, split=i) for i, (a, b) in enumerate(zip(self.cuts[:-1], self.cuts[1:]))]

    def _args(self, dtype):
        rows = slice(self.row0, self.row1)
        cast = (lambda t: t.to(dtype))
        kw = {}
        if self.C:
            kw.update(xrow=self.x[rows], table=cast(self.table))
        if self.mix is not None:
            kw.update(mix_out=cast(self.mix_out[rows]), mix_w=cast(self.mix_w), mix_h=self.mix[1], partners=[cast(p[rows]) for p in self.partners])
        blocks = None if self.C else [cast(b[rows]) for b in self.blocks]
        return blocks, cast(self.W), [cast(t[rows]) for t in self.glist], kw

    def check_fwd(self, case):
        blocks, W, _, kw = self._args(torch.float64)
        b32, W32, _, kw32 = self._args(torch.float32)
        kw, kw32 = ({k: v for k, v in d.items() if k in ("xrow", "table")} for d in (kw, kw32))
        got = self.out.read(_row_mask(self.B, self.row0, self.row1)).view(self.B, K)[self.row0:self.row1]
        ref = J.sum_job_fwd(blocks, W, **kw)
        _check("sum64_fwd", case, got, ref, J.sum_job_fwd(b32, W32, **kw32), scale=_log_scale(ref))
        _untouched(self.gx, "gx in the forward")
        _untouched(self.dtheta, "dtheta in the forward")

    def check_bwd(self, case, mode, params=True):
        """gx, and with `params` dtheta (modes 0 / 1) and the mix_dw column; returns dtheta as read."""
        blocks, W, gl, kw = self._args(torch.float64)
        b32, W32, gl32, kw32 = self._args(torch.float32)
        m = 0 if mode == 0 else 1
        gx, dth, col = J.sum_job_bwd(blocks, W, gl, m, **kw)
        gx32, dth32, col32 = J.sum_job_bwd(b32, W32, gl32, m, **kw32)
        got = self.gx.read(_row_mask(self.B, self.row0, self.row1)).view(self.B, K)[self.row0:self.row1]
        _check("sum64_bwd", case + " gx", got, gx, gx32, None if self.mix is not None else _gx_rounding_allowance(blocks, W, gl, kw))
        _untouched(self.out, "out in the backward")
        if self.part is not None:
            self.part.raw()
        assert int(self.ticket.item()) == 0, f"{case}: the ticket is not 0 after the launch"
        if not params:
            return None
        got_dth = self.dtheta.read().view(K, K).clone()
        _check("sum64_bwd", case + f" dtheta mode {m}", got_dth, dth, dth32)
        if m == 1:
            dead = self.W == 0
            assert bool((got_dth[dead] == 0).all()), f"{case}: an entry with W == 0 does not have gradient exactly 0"
        if self.mix is not None and self.mix_dw is not None:
            H, h = self.mix[0], self.mix[1]
            own = torch.zeros(K, H, dtype=torch.bool)
            own[:, h] = True
            got_col = self.mix_dw.read(own).view(K, H)[:, h]
            assert bool((got_col[self.mix_w[:, h] == 0] == 0).all()), "a coefficient of exactly 0 does not give mix_dw = 0"
            _check("sum64_bwd", case + " mix_dw", got_col.view(1, K), col.view(1, K), col32.view(1, K))
        return got_dth


def _gx_rounding_allowance(blocks, W, gl, kw):
    """(rows, 64): the first-order rounding bound of gx of the module docstring, from the fp64 terms of the case."""
    e, y, _ = J._sum_terms(blocks, W, kw.get("xrow"), kw.get("table"))
    gy = J._guarded_ratio(J.nsum(gl), y).abs()
    pos = e > 0
    eps_e = 2 * EPS * (1 - torch.where(pos, torch.log(torch.where(pos, e, torch.ones_like(e))), torch.zeros_like(e)))
    eps_y = torch.where(y > 0, ((e * eps_e) @ W.t()) / torch.where(y > 0, y, torch.ones_like(y)), torch.zeros_like(y))
    return e * ((gy * (eps_y + (2 * K + 4) * EPS)) @ W) + (e * eps_e) * (gy @ W)


def _launch_sum(dev, jobs, which, mode=1, waves=4, opt_ptr=0, seed=0, modes=None):
    pool = _Pool(dev)
    units = [u for i, j in enumerate(jobs) for u in j.units(pool, mode if modes is None else modes[i])]
    order = torch.randperm(len(units), generator=torch.Generator().manual_seed(seed)).tolist()
    tab = _table(dev, [units[i] for i in order], "SUM_JOB_DTYPE")
    assert tab.shape[1] == 192
    pt = pool.tensor()
    if which == "fwd":
        _call(dev, "ck_jobs_sum64_fwd", tab.data_ptr(), len(units), pt.data_ptr())
    else:
        _call(dev, "ck_jobs_sum64_bwd", tab.data_ptr(), len(units), pt.data_ptr(), opt_ptr, waves)


SUM_ROWS = [1, 31, 32, 33, 127, 128, 129, 161]
FAMILIES = ["normal", "shift", "spread", "neginf", "infrows", "wzero", "gzero", "wspread", "wneginf"]


@pytest.mark.parametrize("n_in", [1, 2, 5])
def test_sum64_fwd_rows(hip_device, n_in):
    """Rows per unit on both sides of a tile (31 / 32 / 33) and of the four waves' stride (127 / 128 / 129, 161: a wave with two
    tiles beside waves with one), a unit whose row0 is not 0, in ONE launch."""
    g = torch.Generator().manual_seed(n_in)
    jobs = [_SumJob(hip_device, g, r, n_in=n_in, fam=FAMILIES[i % 4]) for i, r in enumerate(SUM_ROWS)]
    jobs.append(_SumJob(hip_device, g, 100, 32, 70, n_in=n_in))
    _launch_sum(hip_device, jobs, "fwd", seed=n_in)
    for j in jobs:
        j.check_fwd(f"rows=[{j.row0}, {j.row1}) of {j.B} n_in={n_in} {j.fam}")


@pytest.mark.parametrize("fam", FAMILIES)
def test_sum64_fwd_families_and_units(hip_device, fam):
    """Three jobs cut into 1 / 2 / 3 units (a one-row and a ragged last piece), the units in shuffled table order."""
    g = torch.Generator().manual_seed(len(fam))
    jobs = [_SumJob(hip_device, g, 161, n_in=2, fam=fam), _SumJob(hip_device, g, 130, n_in=1, n_split=2, last=1, fam=fam),
            _SumJob(hip_device, g, 300, 3, 298, n_in=3, n_split=3, last=37, fam=fam)]
    _launch_sum(hip_device, jobs, "fwd", seed=7)
    for j in jobs:
        j.check_fwd(f"{fam} units={j.n_split} rows=[{j.row0}, {j.row1})")


@pytest.mark.parametrize("C", [3, 256])
def test_sum64_fwd_gathers_table_rows(hip_device, C):
    g = torch.Generator().manual_seed(C)
    jobs = [_SumJob(hip_device, g, B, C=C, n_split=s) for B, s in ((1, 1), (33, 1), (161, 2))]
    _launch_sum(hip_device, jobs, "fwd")
    for j in jobs:
        j.check_fwd(f"xrow C={C} B={j.B}")


@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("n_in,n_g", [(1, 1), (2, 3), (5, 1)])
def test_sum64_bwd_rows(hip_device, waves, n_in, n_g):
    """The forward's row counts, and at 8 waves 255 / 256 / 257 (the stride of eight waves); modes 0 and 1 in one launch."""
    g = torch.Generator().manual_seed(10 * waves + n_in)
    rows = SUM_ROWS + ([255, 256, 257] if waves == 8 else [])
    fams = ["normal", "shift", "spread", "neginf", "wspread", "wneginf"]
    jobs = [_SumJob(hip_device, g, r, n_in=n_in, n_g=n_g, fam=fams[(i + n_in) % 6]) for i, r in enumerate(rows)]
    jobs.append(_SumJob(hip_device, g, 100, 32, 70, n_in=n_in, n_g=n_g))
    modes = [i % 2 for i in range(len(jobs))]
    _launch_sum(hip_device, jobs, "bwd", waves=waves, seed=n_in, modes=modes)
    for j, m in zip(jobs, modes):
        j.check_bwd(f"waves={waves} rows=[{j.row0}, {j.row1}) of {j.B} n_in={n_in} n_g={n_g} {j.fam}", m)


@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("fam", FAMILIES)
def test_sum64_bwd_families_and_splits(hip_device, waves, fam):
    """n_split 1, 2, 3, 16 with a one-row and a ragged last piece, jobs with and without a split in one launch, a unit with
    fewer tiles than waves (16 units over 300 rows), the Categorical gather at C = 3, 17 and 256; the same launch twice: dtheta bit for bit."""
    g = torch.Generator().manual_seed(len(fam) + waves)
    dev = hip_device
    jobs = [_SumJob(dev, g, 161, n_in=2, n_g=3, fam=fam), _SumJob(dev, g, 130, n_split=2, last=1, fam=fam),
            _SumJob(dev, g, 600, 3, 598, n_in=3, n_split=3, last=37, fam=fam), _SumJob(dev, g, 300, n_split=16, last=5, fam=fam),
            *[_SumJob(dev, g, B, C=C, n_split=s, fam=fam if fam in ("wzero", "gzero", "wspread", "wneginf") else "normal")
              for B, C, s in ((161, 17, 2), (33, 3, 1), (161, 256, 2))]]
    mode = 0 if fam == "wzero" else 1
    _launch_sum(dev, jobs, "bwd", mode=mode, waves=waves, seed=3)
    first = [j.check_bwd(f"waves={waves} {fam} units={j.n_split} rows=[{j.row0}, {j.row1}) C={j.C}", mode) for j in jobs]
    _launch_sum(dev, jobs, "bwd", mode=mode, waves=waves, seed=4)  # (another table order: the slots are added in slot order)
    for j, d in zip(jobs, first):
        assert torch.equal(j.dtheta.read().view(torch.int32), d.reshape(-1).view(torch.int32)), "dtheta differs between two launches"
        assert int(j.ticket.item()) == 0


@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("mix", [(2, 0, 0, True, False), (2, 1, 2, False, False), (5, 0, 2, True, True), (5, 4, 0, True, False)])
def test_sum64_bwd_under_a_mixing_fold(hip_device, waves, mix):
    """mix_H 2 and 5, the first and the last slot, with and without partners, mix_dw NULL and set, a coefficient of exactly 0."""
    g = torch.Generator().manual_seed(sum(mix[:3]) + waves)
    jobs = [_SumJob(hip_device, g, 161, n_in=2, n_g=2, mix=mix), _SumJob(hip_device, g, 70, n_split=3, last=1, mix=mix),
            _SumJob(hip_device, g, 33)]
    _launch_sum(hip_device, jobs, "bwd", waves=waves)
    for j in jobs:
        j.check_bwd(f"waves={waves} mix(H, h, partners, dw, zero)={mix if j.mix else None} units={j.n_split}", 1)


@pytest.mark.parametrize("kind", ["sgd", "adam"])
@pytest.mark.parametrize("waves", [4, 8])
def test_sum64_bwd_optimizer_epilogue(hip_device, waves, kind):
    dev = hip_device
    g = torch.Generator().manual_seed(40 + waves)
    jobs = [_SumJob(dev, g, 161, n_in=2, n_g=2).with_opt(kind == "adam"), _SumJob(dev, g, 130, n_split=3, last=1, fam="wspread").with_opt(kind == "adam")]

    def fresh(tick):
        for j in jobs:
            j.new_grads(g, scaled=True)
            _fill(j.dtheta, j.gx)

    def launch(mode, opt_ptr):
        _fill(*[j.gx for j in jobs])
        _launch_sum(dev, jobs, "bwd", mode=mode, waves=waves, opt_ptr=opt_ptr)

    def par(i, j):
        def dtheta(case):
            d = j.check_bwd(case, 1)
            _fill(j.dtheta)
            return d
        return (f"job{i}", j.opt, dtheta, lambda: (j.w_out.read().view(K, K), [j.w_out]), P.updated_row_softmax, lambda: [j.dtheta])

    _two_stage(dev, "sum64_bwd", f"waves={waves}", kind, fresh, launch, [par(i, j) for i, j in enumerate(jobs)])
    for j in jobs:
        j.check_bwd(f"waves={waves} {kind} dropped step", 1, params=False)


# --------------------------------------------------------------------------------------------- ck_jobs_mix_fwd / _bwd
def _hmax_template(h_max):
    return 2 if h_max <= 2 else 4 if h_max <= 4 else 8 if h_max <= 8 else 16


class _MixJob:
    """One mixing job: H slots of S blocks over rows [row0, row1) of B-row blocks; gx is ONE guarded buffer whose slot h starts at
    h gx_stride words."""

    def __init__(self, dev, g, B, H, S=1, row0=0, row1=None, n_g=1, n_split=1, last=None, fam="normal", gx_stride=None):
        self.dev, self.B, self.H, self.S, self.row0, self.row1 = dev, B, H, S, row0, B if row1 is None else row1
        self.cuts, self.n_split, self.fam, self.n_g = _cuts(self.row0, self.row1, n_split, last), n_split, fam, n_g
        bfam, wfam, self.gfam = _split_fam(fam)
        self.w, self.theta0 = _weights((K, H), wfam, g)
        x = _blocks(H * S, B, bfam, g)
        self.slots = [[x[h * S + s] for s in range(S)] for h in range(H)]
        self.new_grads(g)
        self.stride = B * K if gx_stride is None else gx_stride
        self.w_d = self.w.to(dev)
        self.out, self.gx, self.dtheta = _Guarded(B * K, dev), _Guarded((H - 1) * self.stride + B * K, dev), _Guarded(K * H, dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.part = self.opt = self.w_out = None

    def new_grads(self, g, scaled=False):
        go = _gout(self.n_g, self.B, self.gfam, g)
        self.glist = list(_scale_units(go) if scaled else go)

    def with_opt(self, adam):
        self.opt, self.w_out = _Opt(self.dev, self.theta0, adam), _Guarded(K * self.H, self.dev)
        return self

    def units(self, pool, mode, h_max):
        if self.n_split > 1 and self.part is None:
            self.part = _Guarded(self.n_split * K * _hmax_template(h_max), self.dev)
        f = {"w": self.w_d.data_ptr(), "out": self.out.out.data_ptr(), "gx": self.gx.out.data_ptr(), "dtheta": self.dtheta.out.data_ptr(),
             "part": 0 if self.part is None else self.part.out.data_ptr(), "ticket": self.ticket.data_ptr(),
             "in_off": pool.add([b for s in self.slots for b in s]), "H": self.H, "g_off": pool.add(self.glist), "n_g": self.n_g,
             "n_split": self.n_split, "mode": mode, "S": self.S}
        if self.opt is not None:
            f.update(self.opt.ptrs())
            f["w_out"] = self.w_out.out.data_ptr()
        return [dict(f, row0=a, row1=b, split=i) for i, (a, b) in enumerate(zip(self.cuts[:-1], self.cuts[1:]))]

    def _args(self, dtype):
        rows = slice(self.row0, self.row1)
        return [[b[rows].to(dtype) for b in s] for s in self.slots], self.w.to(dtype), [t[rows].to(dtype) for t in self.glist]

    def check_fwd(self, case):
        s64, w64, _ = self._args(torch.float64)
        s32, w32, _ = self._args(torch.float32)
        got = self.out.read(_row_mask(self.B, self.row0, self.row1)).view(self.B, K)[self.row0:self.row1]
        ref = J.mix_job_fwd(s64, w64)
        _check("mix_fwd", case, got, ref, J.mix_job_fwd(s32, w32), scale=_log_scale(ref))
        _untouched(self.gx, "gx in the forward")

    def check_bwd(self, case, mode, params=True):
        s64, w64, g64 = self._args(torch.float64)
        s32, w32, g32 = self._args(torch.float32)
        m = 0 if mode == 0 else 1
        gx, dth = J.mix_job_bwd(s64, w64, g64, m)
        gx32, dth32 = J.mix_job_bwd(s32, w32, g32, m)
        own = torch.zeros(self.gx.n, dtype=torch.bool)
        for h in range(self.H):
            own[h * self.stride + self.row0 * K:h * self.stride + self.row1 * K] = True
        raw = self.gx.read(own)
        got = torch.stack([raw[h * self.stride + self.row0 * K:h * self.stride + self.row1 * K].view(-1, K) for h in range(self.H)])
        _check("mix_bwd", case + " gx", got, gx, gx32)
        _untouched(self.out, "out in the backward")
        if self.part is not None:
            self.part.raw()
        assert int(self.ticket.item()) == 0, f"{case}: the ticket is not 0 after the launch"
        if not params:
            return None
        got_dth = self.dtheta.read().view(K, self.H).clone()
        mass = J.mix_job_bwd(s64, w64, [J.nsum(g64).abs()], 0)[1]  # (the addends of d w are G e_h / y: their sizes summed over the rows)
        _check("mix_bwd", case + f" dtheta mode {m}", got_dth, dth, dth32, _order_allowance(mass, self.row1 - self.row0, None if m == 0 else w64))
        return got_dth


def _launch_mix(dev, jobs, which, mode=1, opt_ptr=0, seed=0, h_max=None, gx_stride=None, modes=None):
    pool = _Pool(dev)
    h_max = max(j.H for j in jobs) if h_max is None else h_max
    units = [u for i, j in enumerate(jobs) for u in j.units(pool, mode if modes is None else modes[i], h_max)]
    order = torch.randperm(len(units), generator=torch.Generator().manual_seed(seed)).tolist()
    tab = _table(dev, [units[i] for i in order], "MIX_JOB_DTYPE")
    assert tab.shape[1] == 128
    pt = pool.tensor()
    if which == "fwd":
        _call(dev, "ck_jobs_mix_fwd", tab.data_ptr(), len(units), pt.data_ptr(), h_max)
    else:
        _call(dev, "ck_jobs_mix_bwd", tab.data_ptr(), len(units), pt.data_ptr(), h_max, jobs[0].stride if gx_stride is None else gx_stride, opt_ptr)


MIX_ROWS = [1, 15, 16, 17, 64, 100]


def _mix_jobs(dev, g, H, stride):
    """Six jobs of H slots: every row count, S 1 and 3, n_split 1 and 3, n_g 1 and 3, the value families in turn."""
    jobs = []
    for i, r in enumerate(MIX_ROWS):
        split = 3 if (i % 2 == 1 and r >= 3) else 1
        jobs.append(_MixJob(dev, g, r, H, S=(1, 3)[i % 2], n_g=(1, 3)[(i // 2) % 2], n_split=split, last=1 if r == 17 else None,
                            fam=FAMILIES[(i + H) % 9], gx_stride=stride))
    jobs.append(_MixJob(dev, g, 100, H, S=1, row0=16, row1=70, n_split=3, last=5, gx_stride=stride))
    return jobs


@pytest.mark.parametrize("H", [1, 2, 3, 4, 5, 8, 9, 16])
def test_mix_fwd_and_bwd(hip_device, H):
    """H on both sides of every backward template, rows on both sides of the 16-row pass, S 1 / 3, n_split 1 / 3, a gx_stride
    larger than the block; the backward twice: dtheta bit for bit, every ticket 0."""
    dev = hip_device
    g = torch.Generator().manual_seed(H)
    stride = 100 * K + 192
    jobs = _mix_jobs(dev, g, H, stride)
    _launch_mix(dev, jobs, "fwd", seed=H)
    for j in jobs:
        j.check_fwd(f"H={H} S={j.S} rows=[{j.row0}, {j.row1}) of {j.B} {j.fam}")
    modes = [0 if (j.fam == "wzero" or (i % 3 == 2 and j.fam not in ("wspread", "wneginf"))) else 1 for i, j in enumerate(jobs)]
    _fill(*[j.out for j in jobs])
    _launch_mix(dev, jobs, "bwd", seed=H + 1, modes=modes)
    first = [j.check_bwd(f"H={H} S={j.S} n_g={j.n_g} units={j.n_split} rows=[{j.row0}, {j.row1}) of {j.B} {j.fam}", m) for j, m in zip(jobs, modes)]
    _launch_mix(dev, jobs, "bwd", seed=H + 2, modes=modes)
    for j, d in zip(jobs, first):
        assert torch.equal(j.dtheta.read().view(torch.int32), d.reshape(-1).view(torch.int32)), "dtheta differs between two launches"
        assert int(j.ticket.item()) == 0


def test_mix_jobs_of_different_H_in_one_launch(hip_device):
    """H 2, 3, 9 with h_max = 9: the template of the LAUNCH sizes every job's part slots."""
    dev = hip_device
    g = torch.Generator().manual_seed(99)
    jobs = [_MixJob(dev, g, 100, 2, S=3, n_split=3, last=1), _MixJob(dev, g, 100, 9, n_g=3), _MixJob(dev, g, 100, 3, n_split=2, fam="wspread")]
    _launch_mix(dev, jobs, "fwd", h_max=9)
    for j in jobs:
        j.check_fwd(f"mixed H={j.H} h_max=9")
    _fill(*[j.out for j in jobs])
    _launch_mix(dev, jobs, "bwd", h_max=9)
    for j in jobs:
        j.check_bwd(f"mixed H={j.H} h_max=9 units={j.n_split}", 1)


@pytest.mark.parametrize("kind", ["sgd", "adam"])
@pytest.mark.parametrize("H", [3, 16])
def test_mix_bwd_optimizer_epilogue(hip_device, H, kind):
    dev = hip_device
    g = torch.Generator().manual_seed(50 + H)
    jobs = [_MixJob(dev, g, 100, H, S=2, n_g=2).with_opt(kind == "adam"), _MixJob(dev, g, 100, H, n_split=3, last=1, fam="wspread").with_opt(kind == "adam")]

    def fresh(tick):
        for j in jobs:
            j.new_grads(g, scaled=True)
            _fill(j.dtheta, j.gx)

    def launch(mode, opt_ptr):
        _fill(*[j.gx for j in jobs])
        _launch_mix(dev, jobs, "bwd", mode=mode, opt_ptr=opt_ptr)

    def par(i, j):
        def dtheta(case):
            d = j.check_bwd(case, 1)
            _fill(j.dtheta)
            return d
        return (f"job{i}", j.opt, dtheta, lambda: (j.w_out.read().view(K, H), [j.w_out]), P.updated_row_softmax, lambda: [j.dtheta])

    _two_stage(dev, "mix_bwd", f"H={H}", kind, fresh, launch, [par(i, j) for i, j in enumerate(jobs)])
    for j in jobs:
        j.check_bwd(f"H={H} {kind} dropped step", 1, params=False)


# ------------------------------------------------------------------------------------------------- ck_jobs_mix_params
@pytest.mark.parametrize("H", [2, 5, 16])
def test_mix_params(hip_device, H):
    """d w (64, H) in `part`: modes 0 and 1 over the logit families (one launch of several jobs), then mode 2."""
    dev = hip_device
    g = torch.Generator().manual_seed(60 + H)
    specs = [(m, fam) for m in (0, 1) for fam in ("normal", "spread", "neginf")]
    ws = [_weights((K, H), fam, g)[0] for _, fam in specs]
    dws = [torch.randn(K, H, generator=g) for _ in specs]
    outs = [_Guarded(K * H, dev) for _ in specs]
    held = [(w.to(dev), d.to(dev)) for w, d in zip(ws, dws)]
    tab = _table(dev, [{"w": w.data_ptr(), "part": d.data_ptr(), "dtheta": o.out.data_ptr(), "H": H, "mode": m}
                       for (w, d), o, (m, _) in zip(held, outs, specs)], "MIX_JOB_DTYPE")
    _call(dev, "ck_jobs_mix_params", tab.data_ptr(), len(specs), 0)
    for (m, fam), w, d, o in zip(specs, ws, dws, outs):
        _check("mix_params", f"H={H} mode={m} {fam}", o.read().view(K, H), J.mix_params(d.double(), w.double(), m), J.mix_params(d, w, m))
    for kind in ("sgd", "adam"):
        w, theta0 = _weights((K, H), "normal", g)
        opt, w_out, dth = _Opt(dev, theta0, kind == "adam"), _Guarded(K * H, dev), _Guarded(K * H, dev)
        w_d = w.to(dev)
        cur = {}

        def fresh(tick):
            cur["dw"] = _scale_units(torch.randn(H, K, generator=g)).t().contiguous()  # (64, H): rows 0, 1, 2 scaled
            cur["dw_d"] = cur["dw"].to(dev)

        def launch(mode, opt_ptr):
            t = _table(dev, [dict({"w": w_d.data_ptr(), "part": cur["dw_d"].data_ptr(), "dtheta": dth.out.data_ptr(), "H": H, "mode": mode,
                                   "w_out": w_out.out.data_ptr()}, **opt.ptrs())], "MIX_JOB_DTYPE")
            _call(dev, "ck_jobs_mix_params", t.data_ptr(), 1, opt_ptr)

        def dtheta(case):
            got = dth.read().view(K, H).clone()
            _check("mix_params", case, got, J.mix_params(cur["dw"].double(), w.double(), 1), J.mix_params(cur["dw"], w, 1))
            _fill(dth)
            return got

        _two_stage(dev, "mix_params", f"H={H}", kind, fresh, launch,
                   [("w", opt, dtheta, lambda: (w_out.read().view(K, H), [w_out]), P.updated_row_softmax, lambda: [dth])])


# ------------------------------------------------------------------------------------------------------- ck_jobs_nsum
@pytest.mark.parametrize("elems", [4, 1020, 1024, 64 * 1024 + 4])
def test_nsum(hip_device, elems):
    """n_in on both sides of the four blocks in flight, elems on both sides of a workgroup's 1024 words and past the 64
    workgroups of the capped grid; two jobs per launch.  Bit equality with the fp32 additions in list order."""
    dev = hip_device
    g = torch.Generator().manual_seed(elems % 997)
    for n_a, n_b in ((1, 3), (4, 5), (9, 1)):
        pool = _Pool(dev)
        lists = [[torch.randn(elems, generator=g) * 10.0 ** int(torch.randint(-3, 4, (1,), generator=g)) for _ in range(n)] for n in (n_a, n_b)]
        outs = [_Guarded(elems, dev) for _ in lists]
        tab = _table(dev, [{"out": o.out.data_ptr(), "in_off": pool.add(l), "n_in": len(l)} for o, l in zip(outs, lists)], "NSUM_JOB_DTYPE")
        _call(dev, "ck_jobs_nsum", tab.data_ptr(), 2, pool.tensor().data_ptr(), elems)
        for o, l in zip(outs, lists):
            assert torch.equal(o.read().view(torch.int32), J.nsum(l).view(torch.int32)), f"nsum elems={elems} n_in={len(l)}: not the fp32 sum in list order"
            CASES[0] += 1
            print(f"JOBS-KERNEL nsum elems={elems} n_in={len(l)} err 0 yard 0 ratio 0.000")
    WORST.setdefault("nsum", (0.0, "bit equality", 0.0, 0.0))


# ------------------------------------------------------------------------------------------------------- ck_jobs_root
class _Root:
    """One root launch: R folds of S blocks (the lists of folds with fewer real blocks padded with a block of zeros), guarded
    out / gx / ll / part / dtheta_w[r] / dtheta_c and, with_opt, the optimizer's tensors per weight row and of the coefficients."""

    def __init__(self, dev, g, R, S, B, n_wg, with_c=True, seeded=False, fam="normal", lfam="normal", with_gx=True):
        self.dev, self.R, self.S, self.B, self.n_wg = dev, R, S, B, n_wg
        x = _blocks(R * S, B, fam, g)
        self.folds = [[x[r * S + s] for s in range(S)] for r in range(R)]
        for r in range(R):  # folds with fewer real blocks: the tail of the list is the block of zeros
            for s in range(S - (r % S), S):
                if s > 0:
                    self.folds[r][s] = torch.zeros(B, K)
        self.W, self.theta_w0 = _weights((R, K), lfam, g)
        self.c, self.theta_c0 = _weights((1, R), lfam if R > 1 else "normal", g) if with_c else (None, None)
        if with_c:
            self.c, self.theta_c0 = self.c[0].contiguous(), self.theta_c0[0].contiguous()
        self.seed = torch.randn(B, generator=g) if seeded else None
        self.seed_const = float(np.float32(-1.0 / B))
        self.out, self.ll, self.part = _Guarded(B, dev), _Guarded(4, dev), _Guarded(n_wg * 1042, dev)
        self.gx = _Guarded(R * B * K, dev) if with_gx else None
        self.dth_w, self.dth_c = [_Guarded(K, dev) for _ in range(R)], _Guarded(R, dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.bad = torch.zeros(1, dtype=torch.int32, device=dev)
        self.bad_at_skip_now = False  # mode 2: bad_flag IS the optimizer state's skip_now word, as the trainer binds it
        self.opt_w = self.opt_c = self.w_out = self.c_out = None

    def with_opt(self, adam):
        self.opt_w = [_Opt(self.dev, self.theta_w0[r], adam) for r in range(self.R)]
        self.w_out = [_Guarded(K, self.dev) for _ in range(self.R)]
        if self.c is not None:
            self.opt_c, self.c_out = _Opt(self.dev, self.theta_c0, adam), _Guarded(self.R, self.dev)
        return self

    def launch(self, mode, opt_ptr=0):
        from cirkit_amd import _capi as capi

        dev = self.dev
        pool = _Pool(dev)
        offs = [pool.add(f) for f in self.folds]
        held = [pool.tensor(), torch.tensor(offs, dtype=torch.int32).to(dev), torch.full((self.R,), self.S, dtype=torch.int32).to(dev),
                self.W.to(dev)]
        ptr_array = lambda ps: torch.from_numpy(np.asarray(ps, dtype=np.uint64).view(np.int64).copy()).to(dev)  # noqa: E731
        w_ptrs = ptr_array([held[3].data_ptr() + 4 * K * r for r in range(self.R)])
        dth_ptrs = ptr_array([b.out.data_ptr() for b in self.dth_w])
        held += [w_ptrs, dth_ptrs]
        a = capi.RootLaunch()
        a.pool, a.in_off, a.n_in, a.w = held[0].data_ptr(), held[1].data_ptr(), held[2].data_ptr(), w_ptrs.data_ptr()
        if self.c is not None:
            held.append(self.c.to(dev))
            a.c = held[-1].data_ptr()
            a.dtheta_c = self.dth_c.out.data_ptr()
        a.out, a.ll, a.part, a.ticket = self.out.out.data_ptr(), self.ll.out.data_ptr(), self.part.out.data_ptr(), self.ticket.data_ptr()
        if self.gx is not None:
            a.gx = self.gx.out.data_ptr()
        if self.seed is not None:
            held.append(self.seed.to(dev))
            a.seed = held[-1].data_ptr()
        a.dtheta_w = dth_ptrs.data_ptr()
        if self.opt_w is not None:
            for field, ps in (("theta_w", [o.ptrs()["theta"] for o in self.opt_w]), ("m1_w", [o.ptrs()["m1"] for o in self.opt_w]),
                              ("m2_w", [o.ptrs()["m2"] for o in self.opt_w]), ("w_out", [b.out.data_ptr() for b in self.w_out])):
                held.append(ptr_array(ps))
                setattr(a, field, held[-1].data_ptr())
            if self.opt_c is not None:
                p = self.opt_c.ptrs()
                a.theta_c, a.m1_c, a.m2_c, a.c_out = p["theta"], p["m1"] or None, p["m2"] or None, self.c_out.out.data_ptr()
        a.opt = opt_ptr or None
        a.bad_flag = self.bad.data_ptr()
        if mode == 2 and self.bad_at_skip_now:
            a.bad_flag = opt_ptr + capi.OptState.skip_now.offset
        a.seed_const, a.R, a.B, a.mode, a.n_wg, a.S = self.seed_const, self.R, self.B, mode, self.n_wg, self.S
        _call(dev, "ck_jobs_root", C.byref(a))

    def _ref(self, dtype, mode, bad=False):
        c = None if self.c is None else self.c.to(dtype)
        seed = None if self.seed is None else self.seed.to(dtype)
        return J.root([[b.to(dtype) for b in f] for f in self.folds], self.W.to(dtype), c, mode, seed=seed, seed_const=self.seed_const, bad=bad)

    def check(self, case, mode, params=True, bad=False):
        ref, yard = self._ref(torch.float64, mode, bad), self._ref(torch.float32, mode, bad)
        out = self.out.read()
        ll = self.ll.raw().clone().view(torch.float64)
        self.part.raw()
        assert int(self.ticket.item()) == 0, f"{case}: the ticket is not 0 after the launch"
        assert float(ll[1]) == self.B
        if bad:
            assert bool(torch.isnan(out).all()) and bool(torch.isnan(ll[0])), f"{case}: a flagged launch wrote a likelihood"
        else:
            _check("root", case + " out", out.view(1, -1), ref[0].view(1, -1), yard[0].view(1, -1))
            fin = torch.isfinite(out)
            if bool(fin.all()):
                want = float(out.double().sum())
                assert abs(float(ll[0]) - want) <= self.B * 2.0 ** -53 * float(out.double().abs().sum()), f"{case}: ll[0] {float(ll[0])!r} != {want!r}"
            else:
                assert float(ll[0]) == float(out.double().sum()), f"{case}: ll[0] of non-finite rows"
        if self.gx is None:
            for b in self.dth_w + [self.dth_c]:
                _untouched(b, f"{case}: a gradient of a forward-only launch")
            return None
        _check("root", case + " gx", self.gx.read().view(self.R, self.B, K), ref[2], yard[2])
        if not params:
            return None
        m = 0 if mode == 0 else 1
        dw = torch.stack([b.read() for b in self.dth_w])
        _check("root", case + f" dtheta_w mode {m}", dw, ref[3], yard[3])
        dc = None
        if self.c is not None:
            dc = self.dth_c.read().clone()
            _check("root", case + f" dtheta_c mode {m}", dc.view(1, -1), ref[4].view(1, -1), yard[4].view(1, -1))
        else:
            _untouched(self.dth_c, f"{case}: dtheta_c without coefficients")
        return dw, dc


ROOT_SHAPES = [  # (R, with_c, S, B, n_wg, seeded)
    (1, False, 1, 1, 1, False), (1, True, 2, 3, 2, True), (2, True, 4, 4, 8, False), (4, True, 1, 5, 9, True), (5, True, 2, 255, 64, False),
    (16, True, 4, 257, 9, True), (16, True, 1, 3, 64, False), (1, False, 4, 257, 8, True), (2, True, 2, 255, 1, False), (5, True, 1, 4, 2, True),
]


@pytest.mark.parametrize("shape", ROOT_SHAPES)
def test_root(hip_device, shape):
    """R 1 (with and without c), 2, 4, 5, 16; S 1, 2, 4 with padding blocks; B on both sides of a workgroup's four rows and of
    64 workgroups' 256; n_wg 1 .. 64, more workgroups than groups of four rows among them; a seed vector and seed_const; modes 0
    and 1 over the value and logit families; forward only; the flag raised."""
    R, with_c, S, B, n_wg, seeded = shape
    dev = hip_device
    g = torch.Generator().manual_seed(R * 100 + B)
    for mode, fam, lfam in ((1, "normal", "normal"), (0, "shift", "normal"), (1, "normal", "spread"), (1, "infrows", "neginf"), (0, "neginf", "normal"), (1, "spread", "normal")):
        if fam == "infrows" and B < 3:
            continue
        r = _Root(dev, g, R, S, B, n_wg, with_c, seeded, fam, lfam)
        r.launch(mode)
        r.check(f"R={R} c={with_c} S={S} B={B} n_wg={n_wg} seed={seeded} {fam} logits={lfam}", mode)
    r = _Root(dev, g, R, S, B, n_wg, with_c, seeded, with_gx=False)
    r.launch(1)
    r.check(f"R={R} c={with_c} S={S} B={B} n_wg={n_wg} forward only", 1)
    r = _Root(dev, g, R, S, B, n_wg, with_c, seeded)
    r.bad.fill_(1)
    r.launch(1)
    r.check(f"R={R} c={with_c} S={S} B={B} n_wg={n_wg} bad flag", 1, bad=True)


@pytest.mark.parametrize("kind", ["sgd", "adam"])
@pytest.mark.parametrize("shape", [(1, False, 2, 37, 3), (5, True, 1, 130, 9)])
def test_root_optimizer_epilogue(hip_device, shape, kind):
    """Mode 2 per weight row and for the coefficients, `bad_flag` bound to the optimizer state's skip_now word as the trainer
    binds it (cirkit_amd/train_jobs.py): in the three steps that count the word is 0 and `out` is finite; in the dropped step
    `ck_opt_tick` has raised it, and the SAME mode-2 launch must write NaN to every `out` and to ll[0] and leave theta, m1, m2,
    w_out and c_out bit for bit (`_two_stage` compares them).  The kernel's parameters are protected by skip_now alone: a
    `bad_flag` raised while skip_now is 0 (mode 1, the circuit's own flag) poisons `out` and still writes the gradients."""
    R, with_c, S, B, n_wg = shape
    dev = hip_device
    g = torch.Generator().manual_seed(70 + R)
    r = _Root(dev, g, R, S, B, n_wg, with_c, seeded=True).with_opt(kind == "adam")
    r.bad_at_skip_now = True
    got = {}

    def fresh(tick):
        r.seed = torch.randn(B, generator=g)

    def launch(mode, opt_ptr):
        _fill(r.out, r.gx, r.ll)
        r.launch(mode, opt_ptr)
        if mode == 2:
            skipped = _opt_fields(got["state"]).skip_now != 0
            assert bool(torch.isnan(r.out.read()).all()) == skipped and bool(torch.isfinite(r.out.read()).all()) != skipped, \
                "out of a mode-2 launch does not follow skip_now"

    def row(i):
        def dtheta(case):
            if i == 0:
                got["d"] = r.check(case, 1)
                _fill(*r.dth_w, r.dth_c)
            return got["d"][0][i]
        return (f"w[{i}]", r.opt_w[i], dtheta, lambda: (r.w_out[i].read(), [r.w_out[i]]), P.updated_row_softmax, lambda: [r.dth_w[i]])

    pars = [row(i) for i in range(R)]
    if with_c:
        pars.append(("c", r.opt_c, lambda case: got["d"][1], lambda: (r.c_out.read(), [r.c_out]), P.updated_row_softmax, lambda: [r.dth_c]))
    _two_stage(dev, "root", f"R={R} B={B} n_wg={n_wg}", kind, fresh, launch, pars, scaled=False, on_state=lambda st: got.update(state=st))
    # (what the dropped step's mode-2 launch left, its flag the raised skip_now: NaN in every out and in ll[0], gx as ever)
    r.check(f"R={R} {kind} dropped step: bad_flag = skip_now", 1, params=False, bad=True)
    # the circuit's own flag in mode 1, skip_now not involved: the outputs are poisoned, the gradients written
    r.bad.fill_(1)
    launch(1, 0)
    r.check(f"R={R} {kind} bad flag, mode 1", 1, params=True, bad=True)


# ---------------------------------------------------------------------------------------------------- ck_jobs_cat_bwd
class _CatJob:
    def __init__(self, dev, g, B, C, n_g, column, lfam):
        self.dev, self.B, self.C, self.n_g = dev, B, C, n_g
        self.theta = _logits((K, C), lfam, g)
        if column == "uniform":
            self.x = torch.randint(-1, C + 1, (B,), generator=g).to(torch.int32)  # (-1 marginalised, C out of range)
        elif column == "one":
            self.x = torch.full((B,), C // 2, dtype=torch.int32)
        else:
            self.x = torch.full((B,), -1, dtype=torch.int32)
        self.x_d = self.x.to(dev)
        self.th, self.tab = _Guarded(K * C, dev), _Guarded((C + 1) * K, dev)  # (guard words directly behind row C of the table)
        self.set_theta(self.theta)
        self.dtheta = _Guarded(K * C, dev)
        self.new_grads(g)
        self.opt = self.th_out = self.tab_out = None

    def set_theta(self, theta):
        self.theta = theta.clone()
        self.th.out.copy_(theta.reshape(-1))
        self.tab.out.copy_(log_table(theta.unsqueeze(0))[0].reshape(-1))

    def new_grads(self, g, scaled=False):
        """scaled (the mode-2 cases): eighths of small integers, units 0, 1, 2 times 0, 2^-66 (1.4e-20) and 2^10 -- the rows of a
        category reach their wave in the order LDS atomics fix, which differs between the mode-1 and the mode-2 launch; with these
        values every partial sum is exact, so both launches differentiate the same gradient."""
        if scaled:
            go = torch.randint(-8, 9, (self.n_g, self.B, K), generator=g).float() / 8
            go[..., 0] *= 0.0
            go[..., 1] *= 2.0 ** -66
            go[..., 2] *= 2.0 ** 10
        else:
            go = torch.randn(self.n_g, self.B, K, generator=g)
        self.glist = list(go)

    def with_opt(self, adam, alias):
        """alias: theta_out / table_out ARE theta / table (as the trainer binds them); else buffers of their own, theta_out
        starting as a copy of theta."""
        self.alias = alias
        if alias:
            self.opt = _Opt(self.dev, self.theta, adam)
            self.opt.theta = self.th
        else:
            self.opt = _Opt(self.dev, self.theta, adam)
            self.tab_out = _Guarded((self.C + 1) * K, self.dev)
        return self

    def fields(self, pool, mode):
        f = {"x": self.x_d.data_ptr(), "theta": self.th.out.data_ptr(), "table": self.tab.out.data_ptr(), "dtheta": self.dtheta.out.data_ptr(),
             "g_off": pool.add(self.glist), "n_g": self.n_g, "mode": mode}
        if self.opt is not None:
            p = self.opt.ptrs()
            f.update({"theta_out": p["theta"], "m1": p["m1"], "m2": p["m2"],
                      "table_out": self.tab.out.data_ptr() if self.alias else self.tab_out.out.data_ptr()})
        return f

    def check(self, case):
        G = J.nsum(self.glist)
        ref = J.cat_job_bwd(G.double(), self.x, self.theta.double())
        yard = J.cat_job_bwd(G, self.x, self.theta)
        got = self.dtheta.read().view(K, self.C).clone()
        mass = J.cat_histogram(G.double().abs(), self.x, self.C)[:self.C]  # (C, 64): sum|addends| of dT[c, k]
        count = J.cat_histogram(torch.ones(self.B, 1, dtype=torch.float64), self.x, self.C)[:self.C]  # (C, 1): the rows of category c
        a = _order_allowance(mass, count)  # of dT; their sum over c', C addends in an order of its own: C 2^-24 sum|dT| more
        allow = a.t() + torch.softmax(self.theta.double(), -1) * (a.sum(0) + self.C * EPS * mass.sum(0)).unsqueeze(-1)
        _check("cat_bwd", case, got, ref, yard, allow)
        return got


def _launch_cat(dev, jobs, B, C, mode=1, opt_ptr=0):
    pool = _Pool(dev)
    tab = _table(dev, [j.fields(pool, mode) for j in jobs], "CAT_JOB_DTYPE")
    _call(dev, "ck_jobs_cat_bwd", tab.data_ptr(), len(jobs), pool.tensor().data_ptr(), B, C, opt_ptr)


CAT_C = [1, 2, 3, 15, 16, 17, 31, 32, 255, 256]
CAT_B = [1, 7, 8, 9, 511, 512, 513, 1025]
CAT_SHAPES = [(c, CAT_B[i % 8]) for i, c in enumerate(CAT_C)] + [(CAT_C[(3 * i + 5) % 10], b) for i, b in enumerate(CAT_B)] \
    + [(255, 513), (256, 512), (256, 1025)]  # (both sides of per = 16 | 17 with every category populated)


@pytest.mark.parametrize("C,B", CAT_SHAPES)
def test_cat_bwd(hip_device, C, B):
    """C on both sides of every step of `per` and of the powers of two, B on both sides of the eight rows a wave loads and of
    the 512 rows sorted at a time; n_g on both sides of the four blocks in flight; a uniform column (with marginalised and
    out-of-range rows), one category only, all marginalised; the logit families."""
    dev = hip_device
    g = torch.Generator().manual_seed(C * 10000 + B)
    specs = [(1, "uniform", "normal"), (3, "uniform", "spread"), (4, "one", "neginf"), (5, "none", "normal"), (1, "uniform", "neginf"), (3, "one", "spread")]
    jobs = [_CatJob(dev, g, B, C, n_g, col, lf) for n_g, col, lf in specs]
    _launch_cat(dev, jobs, B, C)
    for j, (n_g, col, lf) in zip(jobs, specs):
        got = j.check(f"C={C} B={B} n_g={n_g} column={col} logits={lf}")
        if col == "none":
            assert bool((got == 0).all()), "marginalised rows reached the logits"


@pytest.mark.parametrize("kind", ["sgd", "adam"])
@pytest.mark.parametrize("C,B", [(3, 9), (17, 513), (256, 100)])
def test_cat_bwd_optimizer_epilogue(hip_device, C, B, kind):
    """Mode 2 with theta_out / table_out aliased to theta / table (as the trainer binds them) and separate, in one launch."""
    dev = hip_device
    g = torch.Generator().manual_seed(80 + C)
    adam = kind == "adam"
    jobs = [_CatJob(dev, g, B, C, 2, "uniform", "normal").with_opt(adam, True), _CatJob(dev, g, B, C, 1, "uniform", "spread").with_opt(adam, False)]

    def fresh(tick):
        for j in jobs:
            j.new_grads(g, scaled=True)
            if j.alias:  # (the logits and the table are the ones the last step left)
                j.theta = j.th.read().view(K, C).clone()
            else:
                j.set_theta(j.opt.theta.read().view(K, C))

    def launch(mode, opt_ptr):
        _launch_cat(dev, jobs, B, C, mode, opt_ptr)

    def par(i, j):
        def dtheta(case):
            d = j.check(case)
            _fill(j.dtheta)
            return d

        def nxt():
            buf = j.tab if j.alias else j.tab_out
            own = _row_mask(C + 1, 0, C)
            return ((buf.read() if j.alias else buf.read(own)).view(C + 1, K)[:C], [buf])

        return (f"job{i} alias={j.alias}", j.opt, dtheta, nxt, lambda th: log_table(th.unsqueeze(0))[0][:C], lambda: [j.dtheta])

    _two_stage(dev, "cat_bwd", f"C={C} B={B}", kind, fresh, launch, [par(i, j) for i, j in enumerate(jobs)])
    assert bool((jobs[0].tab.read().view(C + 1, K)[C] == 0).all()), "row C of the aliased table changed"


def test_cat_bwd_refuses_what_does_not_fit(hip_device):
    """C = 578: (C + 1) 65 + 1152 words and 2 (16 per) + 1025 ints = 163 984 bytes of LDS, above 160 KiB = 163 840 ->
    CK_ERR_UNSUPPORTED, nothing launched; C = 577 (163 724 bytes) is taken."""
    dev = hip_device
    g = torch.Generator().manual_seed(1)
    j = _CatJob(dev, g, 9, 578, 1, "uniform", "normal")
    with pytest.raises(NotImplementedError, match="do not fit"):
        _launch_cat(dev, [j], 9, 578)
    torch.cuda.synchronize()
    _untouched(j.dtheta, "dtheta of a refused launch")
    j = _CatJob(dev, g, 9, 577, 1, "uniform", "normal")
    _launch_cat(dev, [j], 9, 577)
    j.check("C=577 B=9 the largest that fits")


# -------------------------------------------------------------------------------------------------- ck_jobs_gauss_bwd
class _GaussJob:
    def __init__(self, dev, g, B, n_g, has_ss, nan_rows):
        self.dev, self.B, self.n_g, self.has_ss = dev, B, n_g, has_ss
        self.vmin, self.vmax = float(np.float32(0.05)), float(np.float32(3.0))
        self.mean = torch.randn(K, generator=g) * 2
        self.th_sd0 = torch.randn(K, generator=g)
        self.set_sd(self.th_sd0)
        self.x = torch.randn(B, generator=g) * 3
        if nan_rows:
            self.x[::3] = float("nan")
        self.held = [self.x.to(dev)]
        self.dmean, self.dsd = _Guarded(K, dev), _Guarded(K, dev)
        self.new_grads(g)
        self.opt_m = self.opt_s = self.mean_out = self.sd_out = None

    def set_sd(self, th):
        """stddev from the tensor behind it, in fp32 as the forward's prologue leaves it."""
        self.sd = (self.vmin + (self.vmax - self.vmin) * torch.sigmoid(th)) if self.has_ss else th.abs() + 0.1

    def new_grads(self, g, scaled=False):
        go = torch.randn(self.n_g, self.B, K, generator=g)
        self.glist = list(_scale_units(go) if scaled else go)

    def with_opt(self, adam, with_mean_out):
        self.opt_m = _Opt(self.dev, self.mean, adam)
        self.opt_s = _Opt(self.dev, self.th_sd0 if self.has_ss else self.sd, adam)
        self.mean_out, self.sd_out = (_Guarded(K, self.dev) if with_mean_out else None), _Guarded(K, self.dev)
        return self

    def fields(self, pool, mode):
        self.held += [self.mean.to(self.dev), self.sd.to(self.dev)]
        f = {"mean": self.held[-2].data_ptr(), "stddev": self.held[-1].data_ptr(), "x": self.held[0].data_ptr(), "dmean": self.dmean.out.data_ptr(),
             "dsd": self.dsd.out.data_ptr(), "g_off": pool.add(self.glist), "n_g": self.n_g, "vmin": self.vmin, "vmax": self.vmax,
             "has_ss": int(self.has_ss), "mode": mode}
        if self.opt_m is not None:
            pm, ps = self.opt_m.ptrs(), self.opt_s.ptrs()
            f.update({"th_mean": pm["theta"], "m1_mean": pm["m1"], "m2_mean": pm["m2"], "th_sd": ps["theta"], "m1_sd": ps["m1"], "m2_sd": ps["m2"],
                      "mean_out": 0 if self.mean_out is None else self.mean_out.out.data_ptr(), "sd_out": self.sd_out.out.data_ptr()})
        return f

    def check(self, case):
        G = J.nsum(self.glist)
        ref = J.gauss_job_bwd(G.double(), self.x.double(), self.mean.double(), self.sd.double(), self.vmin, self.vmax, self.has_ss)
        yard = J.gauss_job_bwd(G, self.x, self.mean, self.sd, self.vmin, self.vmax, self.has_ss)
        dm, ds = self.dmean.read().clone(), self.dsd.read().clone()
        _check("gauss_bwd", case + " dmean", dm.view(1, K), ref[0].view(1, K), yard[0].view(1, K))
        _check("gauss_bwd", case + " dsd", ds.view(1, K), ref[1].view(1, K), yard[1].view(1, K))
        return dm, ds


def _launch_gauss(dev, jobs, B, mode=1, opt_ptr=0):
    pool = _Pool(dev)
    tab = _table(dev, [j.fields(pool, mode) for j in jobs], "GAUSS_JOB_DTYPE")
    assert tab.shape[1] == 128
    _call(dev, "ck_jobs_gauss_bwd", tab.data_ptr(), len(jobs), pool.tensor().data_ptr(), B, opt_ptr)


@pytest.mark.parametrize("B", [1, 15, 16, 17, 300])
def test_gauss_bwd(hip_device, B):
    """B on both sides of the 16 row groups; n_g 1 / 3, NaN rows, has_ss 0 / 1 in one launch."""
    dev = hip_device
    g = torch.Generator().manual_seed(90 + B)
    specs = [(1, False, False), (3, True, True), (1, True, False), (3, False, True)]
    jobs = [_GaussJob(dev, g, B, *s) for s in specs]
    _launch_gauss(dev, jobs, B)
    for j, s in zip(jobs, specs):
        j.check(f"B={B} (n_g, has_ss, NaN rows)={s}")


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_gauss_bwd_optimizer_epilogue(hip_device, kind):
    """Mode 2: has_ss 0 / 1, mean_out NULL and set; sd_out is the scaled sigmoid of the updated tensor (has_ss) or the tensor."""
    dev = hip_device
    B = 100
    g = torch.Generator().manual_seed(95)
    adam = kind == "adam"
    jobs = [_GaussJob(dev, g, B, 2, True, True).with_opt(adam, True), _GaussJob(dev, g, B, 1, False, False).with_opt(adam, False)]
    got = {}

    def fresh(tick):
        for j in jobs:
            j.new_grads(g, scaled=True)

    def launch(mode, opt_ptr):
        _launch_gauss(dev, jobs, B, mode, opt_ptr)

    def pars_of(i, j):
        def dmean(case):
            got[i] = j.check(case)
            _fill(j.dmean, j.dsd)
            return got[i][0]

        def sd_next(th):
            return j.vmin + (j.vmax - j.vmin) * torch.sigmoid(th) if j.has_ss else th

        mean_next = (lambda: (j.mean_out.read(), [j.mean_out])) if j.mean_out is not None else (lambda: (j.opt_m.theta.read(), []))
        return [(f"job{i} mean", j.opt_m, dmean, mean_next, lambda th: th, lambda: [j.dmean]),
                (f"job{i} sd", j.opt_s, lambda case: got[i][1], lambda: (j.sd_out.read(), [j.sd_out]), sd_next, lambda: [j.dsd])]

    # (the mean and stddev the kernel differentiates stay those of the job's construction: the forward's values are inputs)
    _two_stage(dev, "gauss_bwd", f"B={B}", kind, fresh, launch, [p for i, j in enumerate(jobs) for p in pars_of(i, j)])


# ------------------------------------------------------------------------------------ ck_opt_step_range / ck_opt_tick
@pytest.mark.parametrize("kind", ["sgd", "adam"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 2048 * 256 + 5])
def test_opt_step_range_and_tick(hip_device, n, kind):
    """n on both sides of a workgroup and past the 2048 x 256 entries of the capped grid; g2 NULL and set; SGD with NULL moments,
    Adam; three ticks and a dropped one; bc1 / bc2 of every tick within one fp32 rounding of 1 - b^t in fp64."""
    from cirkit_amd.train_state import DeviceOptState

    dev = hip_device
    adam = kind == "adam"
    g = torch.Generator().manual_seed(n % 1000 + adam)
    state = DeviceOptState(dev).sync(LR, BETAS, OPT_EPS, kind)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    opts = [_Opt(dev, torch.randn(n, generator=g), adam) for _ in range(2)]

    def grads():
        gr = torch.randn(n, generator=g)
        gr[::7] = 0.0
        gr[1::7] *= 1e-20
        gr[2::7] *= 1e3
        return gr

    def step(opt, g1, g2):
        p = opt.ptrs()
        held = [g1.to(dev), None if g2 is None else g2.to(dev)]
        _call(dev, "ck_opt_step_range", p["theta"], held[0].data_ptr(), None if g2 is None else held[1].data_ptr(), p["m1"] or None, p["m2"] or None,
              n, state.ptr)

    for tick in (1, 2, 3):
        _call(dev, "ck_opt_tick", state.ptr, flag.data_ptr(), None)
        o = _opt_fields(state)
        assert (o.step, o.skipped, o.skip_now) == (tick, 0, 0)
        for got, b in ((o.bc1, BETAS[0]), (o.bc2, BETAS[1])):
            want = 1.0 - b ** tick
            assert abs(got - want) <= 2.0 ** -24 * want * (1 + 1e-6), f"bias correction of tick {tick}: {got!r} against {want!r}"
        for opt, with_g2 in zip(opts, (False, True)):
            g1, g2 = grads(), (grads() if with_g2 else None)
            gsum = g1 if g2 is None else g1 + g2  # (the kernel adds the two in fp32 before the step)
            th0, m10, m20 = opt.snap()
            step(opt, g1, g2)
            th1, m11, m21 = opt.snap()
            ref = J.opt_step(kind, th0.double(), gsum.double(), m10.double(), m20.double(), tick, LR, B32, BETAS, OPT_EPS)
            yard = J.opt_step(kind, th0, gsum, m10, m20, tick, LR, B32, BETAS, OPT_EPS)
            case = f"n={n} {kind} tick={tick} g2={with_g2}"
            _check("opt_step_range", case + " (theta' - theta) / lr", th1.double() - th0.double(), ref[0] - th0.double(), yard[0].double() - th0.double(), scale=LR)
            if adam:
                _check("opt_step_range", case + " m1'", m11, ref[1], yard[1], scale=float(ref[1].abs().max()) or 1.0)
                _check("opt_step_range", case + " m2'", m21, ref[2], yard[2], scale=float(ref[2].abs().max()) or 1.0)
            assert torch.equal(th1[::7], th0[::7]), "a zero gradient moved its entry"
    held = [b for o in opts for b in o.bits()]
    flag.fill_(1)
    _call(dev, "ck_opt_tick", state.ptr, flag.data_ptr(), None)
    o = _opt_fields(state)
    assert (o.step, o.skipped, o.skip_now) == (3, 1, 1) and int(flag.item()) == 0
    for opt in opts:
        step(opt, grads(), grads())
    assert all(torch.equal(a, b) for a, b in zip(held, [b for o in opts for b in o.bits()])), "a dropped step changed a parameter or a moment"
